#!/usr/bin/env python
"""Generate ``g20_supervised.npz`` by running the REAL reference's supervised ``Engine`` (``policies/supervised/train.py``) on
the CPU (``python tests/golden/make_golden_supervised.py``, build container only; ``make_golden_nn.py``'s recipe:
``oracle.ref_shim``, stubbed simulator modules, ``get_loaders`` a no-op, seeded models written to temporary checkpoint directories,
the injected-sample Chamfer distance).

Settings, batches and sensor records are ``supervised_util``'s: ``env_util``'s case "b" models, 50 actions, E = 2, budget 2, 700
surface points, a policy of hidden_dim 40 and 3 layers, ``torch.manual_seed(policy_seed)`` before the two ``Latent_Model``s are
built.  The reference's ``train``, ``save``, ``load`` and ``validate`` are driven directly, with lists as loaders, in a temporary
working directory:

  step 0    ``np.random.seed(NP_SEED)``, ``train`` over two batches (the second iteration's gradient is the sum of both: the
            reference never zeroes it), ``save``
  step 1    a fresh Adam, ``load(train=True)``, ``np.random.seed(NP_SEED + 1)``, ``train`` over one batch (model 0 moves first)
  validate  one batch, a whole episode

Stored (weights and images are NOT stored: the tests rebuild them from the seeds and check the checksums):
  policy_seed, sha:<kind>, bn:<key>, status:<batch>, face_idx|u|v            as in g19; sha:policy = the seeded policy models
  train:<n>:random_actions|target|values|loss|mask   iteration n (0, 1: step 0; 2: step 1); mask = obs["mask"] the model saw
  train:2:moved                                      the actions model 0 chose before iteration 2
  train_loss:<step>                                  ``engine.train_loss``
  w:<step>:<key>, wsum:<step>:<key>                  model <step> after its training: ``STORED_WEIGHTS`` whole, of every tensor
                                                     ``supervised_util.weight_sums``
  valid:<i>:score|mask (i = 0 reset, 1, 2), valid:<i>:actions|values (i = 1, 2: what model i - 1 saw and chose)
The policy seed is the first from 0 at which, at every decision (the move of iteration 2, both validation steps), the two lowest
open values of each element are more than ``MIN_CHOICE_GAP`` = 1e-2 apart (relative): asserted, the smallest printed."""
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
import env_util as eu  # noqa: E402
import supervised_util as su  # noqa: E402


def run(policy_seed, sup_mod, env_mod, locations, root):
    """The fixture's sequence on the reference engine -> (log dict, smallest decision gap)."""
    args = su.engine_args(**locations)
    engine = sup_mod.Engine(args)
    engine.env = env_mod.ActiveTouch(engine.args)
    engine.policy = types.SimpleNamespace(reset=lambda: None)
    torch.manual_seed(policy_seed)
    engine.models = [sup_mod.learning_model.Latent_Model(args) for _ in range(args.budget)]
    out = {"sha:policy": state_checksum({f"{i}.{k}": v for i, m in enumerate(engine.models) for k, v in m.state_dict().items()})}
    writer = types.SimpleNamespace(add_scalars=lambda *a, **k: None)
    seen, checks = [], []               # (model index, mask, values) of every model call; (actions, score, first_score) of every check_step
    for i, m in enumerate(engine.models):
        m.register_forward_hook(lambda mod, inp, res, i=i: seen.append((i, inp[0]["mask"].numpy().copy(), res.detach().numpy().copy())))
    check_step = engine.env.check_step

    def logged_check(actions):
        obs = check_step(actions)
        checks.append((np.asarray(actions).astype(np.int64), obs["score"].numpy().copy(), obs["first_score"].numpy().copy()))
        return obs

    engine.env.check_step = logged_check
    gap = np.inf
    n = 0
    for step, loader in ((0, su.batches("train")[:2]), (1, su.batches("train")[2:])):
        engine.step = step
        engine.optimizer = torch.optim.Adam(list(engine.models[step].parameters()), lr=args.lr, weight_decay=0)
        engine.load(train=True)
        for m in engine.models:
            m.eval()
        engine.epoch, engine.best_loss, engine.last_improvement = 0, 10000, 0
        np.random.seed(su.NP_SEED + step)
        del seen[:], checks[:]
        engine.train(loader, writer)
        engine.save()
        per = step + 1                                                  # model calls per iteration
        assert len(seen) == per * len(loader) and len(checks) == 5 * len(loader)
        for j in range(len(loader)):
            calls, tried = seen[per * j:per * (j + 1)], checks[5 * j:5 * (j + 1)]
            key = f"train:{n}:"
            if step:
                moved = su.choose(calls[0][2].astype(np.float64), calls[0][1])
                gap = min(gap, su.eligible_gap(calls[0][2].astype(np.float64), calls[0][1]))
                assert np.array_equal(np.where(calls[1][1] != 0)[1], moved)          # the mask the next model saw holds that move
                out[key + "moved"] = moved
            assert calls[-1][0] == step
            out[key + "mask"], out[key + "values"] = calls[-1][1], calls[-1][2]
            out[key + "random_actions"] = np.stack([t[0] for t in tried])
            out[key + "target"] = np.stack([t[2] - t[1] for t in tried])
            pred = np.stack([calls[-1][2][np.arange(eu.E), t[0]] for t in tried])
            out[key + "loss"] = np.float32(((torch.from_numpy(out[key + "target"]) - torch.from_numpy(pred)) ** 2).mean())
            n += 1
        losses = [float(out[f"train:{k}:loss"]) for k in range(n - len(loader), n)]
        assert abs(engine.train_loss - sum(losses) / len(losses)) <= 1e-5 * abs(engine.train_loss), (engine.train_loss, losses)
        out[f"train_loss:{step}"] = np.float64(engine.train_loss)
        for k, v in engine.models[step].state_dict().items():
            if k in su.STORED_WEIGHTS:
                out[f"w:{step}:{k}"] = v.numpy().copy()
            out[f"wsum:{step}:{k}"] = su.weight_sums(v.numpy())
    # ---- validate ---------------------------------------------------------------------------------------------------------------
    log = []
    reset, step_fn = engine.env.reset, engine.env.step

    def logged_reset(batch):
        obs = reset(batch)
        log.append((obs, None))
        return obs

    def logged_step(action):
        res = step_fn(action)
        log.append((res[0], np.asarray(action).astype(np.int64)))
        return res

    engine.env.reset, engine.env.step = logged_reset, logged_step
    del seen[:]
    with torch.no_grad():
        engine.validate(su.batches("valid"), writer)
    assert len(log) == 1 + args.budget and len(seen) == args.budget
    for i, (obs, actions) in enumerate(log):
        out[f"valid:{i}:score"], out[f"valid:{i}:mask"] = obs["score"].numpy(), obs["mask"].numpy()
        if i:
            idx, mask, values = seen[i - 1]
            assert idx == i - 1 and np.array_equal(su.choose(values.astype(np.float64), mask), actions)
            gap = min(gap, su.eligible_gap(values.astype(np.float64), mask))
            out[f"valid:{i}:actions"], out[f"valid:{i}:values"] = actions, values
    out["current_loss"] = np.float64(engine.current_loss)
    return out, gap


def main():
    tables = su.status_tables()
    with reference_setup(su.ENV_CASE, tables=tables, records=su.records(tables)) as setup:
        sup_mod = importlib.import_module("pterotactyl.policies.supervised.train")
        for policy_seed in range(20):
            with setup.workdir() as (root, locations):
                log, gap = run(policy_seed, sup_mod, setup.env_mod, locations, root)
            print(f"policy seed {policy_seed}: smallest relative gap between the two lowest open values of a decision {gap:.3e}")
            if gap > su.MIN_CHOICE_GAP:
                break
    assert gap > su.MIN_CHOICE_GAP, "no policy seed below 20 keeps every decision's two lowest open values 1e-2 apart"
    out = setup.out
    out.update(log)
    out["policy_seed"] = np.int64(policy_seed)
    for k in sorted(out):
        if k.startswith(("train:", "valid:", "train_loss")) and out[k].size <= 12:
            print(k, out[k].tolist())
    save(su.FIXTURE, **out)


if __name__ == "__main__":
    main()
