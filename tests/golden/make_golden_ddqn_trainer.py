#!/usr/bin/env python
"""Generate ``g21_ddqn_trainer.npz`` by running the REAL reference's DDQN ``Engine`` (``policies/DDQN/train.py``) on the CPU
(``python tests/golden/make_golden_ddqn_trainer.py``, build container only; ``make_golden_supervised.py``'s recipe:
``oracle.ref_shim``, stubbed simulator modules, ``StubSampler``, ``get_loaders`` a no-op, seeded models written to temporary
checkpoint directories, the injected-sample Chamfer distance, lists as loaders, a stub writer, the ``ave_*`` windows made on the CPU
by hand).

Settings, batches and sensor records are ``ddqn_trainer_util``'s (``env_util``'s case "b" models, latent policy, E = 2, budget 2, 700
surface points, 50 actions, hidden_dim 40, 3 layers; mem_capacity 8, train_batch_size 2, burn_in 2, target_update 3, gamma 0.9;
epsilon 0.5 / 0.5 / 0.05).  ``torch.manual_seed(policy_seed)`` before the policy and the target net are built, ``seed_loop()`` before
the reference's ``train`` runs over the three training batches (six steps: two of burn-in, four with an update each), then its
``validate`` over the one validation batch.

Stored (weights and images are NOT stored: the tests rebuild them from the seeds and check the checksums):
  policy_seed, sha:<kind>, bn:<key>, status:<batch>, face_idx|u|v            as in g20; sha:policy = the seeded policy learner
  step:action|random|epsilon|indices|loss|q|mask   per training step (6 rows): q = the Q rows a greedy choice saw (NaN at a random
                                                   step), indices = the replay draw of the step's update (-1 before burn-in)
  step:reward                                      the environment's reward of every step
  replay:position|count_seen|actions|rewards       the replay memory after training
  steps, episode, epsilon, target_copies, ave_reward, ave_recon (the first three window entries)
  wsum:policy:<key>, wsum:target:<key>, w:<key>    ``weight_sums`` of every tensor of both learners at the end; ``STORED_WEIGHTS`` whole
  valid:<i>:score|mask (i = 0 reset, 1, 2), valid:<i>:actions|q (i = 1, 2), current_loss
Asserted (margins printed): after burn-in at least one greedy and one random action occurred; at least one target copy occurred;
at every greedy decision (training and validation) the two highest open Q values of each element are more than ``MIN_CHOICE_GAP``
= 1e-2 apart (relative) — a hundred times the 1e-4 bound of the tests, so equal actions follow from the value bound.  The policy seed
is the first from 0 at which all of this holds."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import save, state_checksum  # noqa: E402  (installs the import shim)
from make_golden_env import reference_setup  # noqa: E402
import ddqn_trainer_util as dt  # noqa: E402
import supervised_util as su  # noqa: E402


def q_of(policy, obs):
    with torch.no_grad():
        return policy.model(obs).numpy().copy()


def run(policy_seed, mods, locations):
    """The fixture's sequence on the reference engine -> (log dict, smallest greedy gap, whether every condition held)."""
    train_mod, env_mod, replay_mod, ddqn_mod = mods
    args = dt.engine_args(**locations)
    engine = train_mod.Engine(args)
    engine.env = env_mod.ActiveTouch(engine.args)
    engine.replay_memory = replay_mod.ReplayMemory(args)
    torch.manual_seed(policy_seed)
    engine.policy = ddqn_mod.DDQN(args, engine.env.mesh_info, engine.replay_memory)
    engine.target_net = ddqn_mod.DDQN(args, engine.env.mesh_info, None)
    engine.target_net.load_state_dict(engine.policy.state_dict())
    engine.target_net.eval()
    out = {"sha:policy": state_checksum(engine.policy.state_dict())}
    engine.writer = types.SimpleNamespace(add_scalars=lambda *a, **k: None)
    engine.window_size = 1000
    engine.ave_reward, engine.ave_recon = torch.zeros(engine.window_size), torch.zeros(engine.window_size)

    log = dt.LoopLog(engine, q_of)
    sample = engine.replay_memory.sample

    def logged_sample():                      # (the reference's memory keeps no record of its draw: replay it from the state)
        state = np.random.get_state()
        batch = sample()
        if batch is not None:
            np.random.set_state(state)
            engine.replay_memory.last_indices = np.random.choice(min(engine.replay_memory.count_seen, args.mem_capacity), args.train_batch_size)
        return batch

    engine.replay_memory.sample = logged_sample
    copies, rewards = [], []
    load = engine.target_net.load_state_dict
    engine.target_net.load_state_dict = lambda sd: copies.append(engine.steps) or load(sd)
    step_fn = engine.env.step

    def logged_step(action):
        res = step_fn(action)
        rewards.append(res[1].numpy().copy())
        return res

    engine.env.step = logged_step
    dt.seed_loop()
    engine.train(su.batches("train"))
    rows = log.rows
    assert len(rows) == dt.STEPS and engine.steps == dt.STEPS and engine.episode == 3
    assert [r["epsilon"] for r in rows] == list(dt.EPSILONS) and tuple(copies) == dt.TARGET_COPIES
    assert all(r["random"] for r in rows[:2]) and all(np.isnan(r["loss"]) for r in rows[:2]) and not any(np.isnan(r["loss"]) for r in rows[2:])
    after = [r["random"] for r in rows[2:]]
    gap = min([dt.open_gap(r["q"], r["mask"]) for r in rows if not r["random"]], default=np.inf)
    ok = any(after) and not all(after) and len(copies) >= 1
    for k in ("action", "random", "epsilon", "indices", "loss", "mask"):
        out["step:" + k] = np.stack([np.asarray(r[k]) for r in rows])
    out["step:q"] = np.stack([r["q"] if not r["random"] else np.full_like(r["q"], np.nan) for r in rows]).astype(np.float32)
    out["step:reward"] = np.stack(rewards)
    m = engine.replay_memory
    out.update({"replay:position": np.int64(m.position), "replay:count_seen": np.int64(m.count_seen), "replay:actions": m.actions.numpy().copy(),
                "replay:rewards": m.rewards.numpy().copy(), "steps": np.int64(engine.steps), "episode": np.int64(engine.episode),
                "epsilon": np.float64(engine.epsilon), "target_copies": np.asarray(copies, dtype=np.int64),
                "ave_reward": engine.ave_reward[:3].numpy().copy(), "ave_recon": engine.ave_recon[:3].numpy().copy()})
    for name, learner in (("policy", engine.policy), ("target", engine.target_net)):
        for k, v in learner.state_dict().items():
            out[f"wsum:{name}:{k}"] = dt.weight_sums(v.numpy())
    for k in dt.STORED_WEIGHTS:
        out["w:" + k] = engine.policy.state_dict()[k].numpy().copy()
    # ---- validate ---------------------------------------------------------------------------------------------------------------
    engine.env.step = step_fn
    seen = []
    reset = engine.env.reset
    engine.env.reset = lambda batch: seen.append((reset(batch), None)) or seen[-1][0]
    engine.env.step = lambda a: (lambda r: seen.append((r[0], np.asarray(a).astype(np.int64))) or r)(step_fn(a))
    del rows[:]
    with torch.no_grad():
        engine.validate(su.batches("valid"))
    assert len(seen) == 1 + args.budget and len(rows) == args.budget and not any(r["random"] for r in rows)
    for i, (obs, actions) in enumerate(seen):
        out[f"valid:{i}:score"], out[f"valid:{i}:mask"] = obs["score"].numpy().copy(), obs["mask"].numpy().copy()
        if i:
            r = rows[i - 1]
            assert np.array_equal(r["action"], actions) and r["epsilon"] == -1
            gap = min(gap, dt.open_gap(r["q"], r["mask"]))
            out[f"valid:{i}:actions"], out[f"valid:{i}:q"] = actions, r["q"]
    out["current_loss"] = np.float64(engine.current_loss)
    print(f"policy seed {policy_seed}: random after burn-in {after}, target copies at {copies}, smallest relative gap between the two "
          f"highest open Q values of a greedy decision {gap:.3e}")
    return out, gap, ok


def main():
    tables = su.status_tables()
    with reference_setup(dt.ENV_CASE, tables=tables, records=su.records(tables)) as setup:
        mods = (importlib.import_module("pterotactyl.policies.DDQN.train"), setup.env_mod,
                importlib.import_module("pterotactyl.policies.replay"), importlib.import_module("pterotactyl.policies.DDQN.ddqn"))
        for policy_seed in range(20):
            with setup.workdir() as (_, locations):
                log, gap, ok = run(policy_seed, mods, locations)
            if ok and gap > dt.MIN_CHOICE_GAP:
                break
    assert ok and gap > dt.MIN_CHOICE_GAP, "no policy seed below 20 gives a greedy and a random action after burn-in with every greedy " \
                                           "decision's two highest open Q values 1e-2 apart"
    out = setup.out
    out.update(log)
    out["policy_seed"] = np.int64(policy_seed)
    for k in sorted(out):
        if k.startswith(("step:", "valid:", "replay:", "ave_", "current_loss", "epsilon", "steps", "episode")) and out[k].size <= 16:
            print(k, out[k].tolist())
    save(dt.FIXTURE, **out)


if __name__ == "__main__":
    main()
