"""This package's DDQN ``Engine`` replays ``g21_ddqn_trainer.npz`` — what the REFERENCE engine did on the CPU
(``golden/make_golden_ddqn_trainer.py``): six training steps (two of burn-in, four with an update each, the target copy at step 3)
and one validation episode — with ``fused_q_latent`` on and off, with host and device replay.

Bounds: equal random flags, actions, epsilons, sampled indices, replay bookkeeping and validation actions; losses, Q rows, rewards,
weight sums, scores and ``current_loss`` within 1e-4 relative (``helpers.rel_err``: the largest difference over the largest
reference entry), the bound of the g18 - g20 tests.  The generator asserts that at every greedy decision of the fixture the two
highest open Q values are more than 1e-2 apart, one hundred times that, so equal actions follow from the value bound.  Every test
prints the worst differences it measured; on an MI355X, the worst over the four combinations: losses 1.6e-6, Q rows 3.1e-7, rewards
2.5e-6, the ``ave_*`` windows 8.3e-7, weight sums 7.7e-9 of the sum of magnitudes, stored weights 7.9e-7, scores 1.2e-7,
``current_loss`` below 1e-7."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ddqn_trainer_util as dt
import env_util as eu
import supervised_util as su

pytestmark = pytest.mark.gpu

from a3vt_amd import ops  # noqa: E402

TOL = 1e-4


@pytest.fixture(scope="module")
def golden():
    from golden_util import load
    return load(dt.FIXTURE)


@pytest.fixture(autouse=True)
def restore_process_flags():
    yield from eu.kept_process_flags()


@pytest.fixture(scope="module")
def locations(cuda, golden, tmp_path_factory):
    """The checkpoint directories of this package's models built by the fixture's recipe (checksums asserted)."""
    return eu.package_models(dt.ENV_CASE, golden, tmp_path_factory.mktemp("g21"))


@pytest.fixture(scope="module")
def sensor_records(golden):
    tables = su.status_tables()
    for name, t in tables.items():
        assert np.array_equal(t, golden["status:" + name])
    return su.records(tables)


def q_of(policy, obs):
    """The Q rows a greedy choice of this learner sees: the kernel's on the fused path (``ddqn_latent_q`` returns the bits its own
    argmax read), the modules' otherwise."""
    net = policy.model
    mask, latent, first = net.inputs(obs)
    with torch.no_grad():
        q = ops.ddqn_latent_q(net.table(), mask, latent, first)[0] if net.fused_ok(mask) else net(obs)
    return q.cpu().numpy().copy()


def setup(engine, env, seed):
    """What ``Engine.__call__`` does before its loop, with the learners drawn under ``seed`` (after the environment is built, as the
    generator draws them)."""
    engine.env = env
    torch.manual_seed(seed)
    engine.make_learners()
    engine.writer = SimpleNamespace(add_scalars=lambda *a, **k: None)
    engine.window_size = 1000
    engine.ave_reward = torch.zeros(engine.window_size, device=engine.policy_device())
    engine.ave_recon = torch.zeros(engine.window_size, device=engine.policy_device())


def replay(golden, locations, sensor_records, monkeypatch, tmp_path, **knobs):
    """The fixture's sequence on this package's engine."""
    from golden_util import state_sha256
    from a3vt_amd.pterotactyl.policies import environment, recorded
    from a3vt_amd.pterotactyl.policies.DDQN import train as dtr
    monkeypatch.setattr(environment.ActiveTouch, "get_loaders", lambda self: None)
    monkeypatch.chdir(tmp_path)                                   # results/ and experiments/checkpoint/ are made in the working directory
    engine = dtr.Engine(dt.engine_args(**knobs, **locations), sampler=recorded.RecordedSampler(sensor_records))
    setup(engine, environment.ActiveTouch(engine.args, sampler=engine.sampler), int(golden["policy_seed"]))
    engine.env.score_samples = eu.score_samples(golden)
    sd = {k: v.cpu() for k, v in engine.policy.state_dict().items()}
    assert (state_sha256(sd) == golden["sha:policy"]).all(), "the seeded policy is not the fixture's"
    assert engine.policy.model.fused_q_latent is bool(knobs["fused_q_latent"])
    log = dt.LoopLog(engine, q_of)
    rewards = []
    step_fn = engine.env.step

    def logged_step(action):
        res = step_fn(action)
        rewards.append(res[1].cpu().numpy().copy())
        return res

    engine.env.step = logged_step
    dt.seed_loop()
    engine.train(su.batches("train"))
    rows = list(log.rows)
    end = {"policy": {k: v.detach().cpu() for k, v in engine.policy.state_dict().items()},
           "target": {k: v.detach().cpu() for k, v in engine.target_net.state_dict().items()}}
    seen = []
    reset = engine.env.reset
    engine.env.reset = lambda batch: seen.append(reset(batch)) or seen[-1]
    engine.env.step = lambda a: (lambda r: seen.append(r[0]) or r)(step_fn(a))
    del log.rows[:]
    with torch.no_grad():
        engine.validate(su.batches("valid"))
    engine.env.reset, engine.env.step = reset, step_fn
    return SimpleNamespace(engine=engine, rows=rows, rewards=rewards, end=end, seen=seen, valid_rows=list(log.rows))


def compare(golden, r, what):
    from helpers import rel_err
    worst = {}

    def within(name, got, want):
        e = rel_err(torch.as_tensor(np.asarray(got)).float(), torch.from_numpy(np.asarray(want)).float())
        worst[name] = max(worst.get(name, 0.0), e)
        assert e < TOL, f"{what}: {name} differs by {e:.2e} (relative)"

    engine, rows = r.engine, r.rows
    assert len(rows) == dt.STEPS
    assert [x["random"] for x in rows] == golden["step:random"].tolist()
    assert np.array_equal(np.stack([x["action"] for x in rows]), golden["step:action"])
    assert [x["epsilon"] for x in rows] == golden["step:epsilon"].tolist() == list(dt.EPSILONS)
    assert np.array_equal(np.stack([x["indices"] for x in rows]), golden["step:indices"])
    assert np.array_equal(np.stack([x["mask"] for x in rows]), golden["step:mask"])
    updated = ~np.isnan(golden["step:loss"])
    assert updated.tolist() == [not np.isnan(x["loss"]) for x in rows] == [False, False, True, True, True, True]
    within("loss", np.array([x["loss"] for x in rows])[updated], golden["step:loss"][updated])
    for n, x in enumerate(rows):
        if not x["random"]:
            within("q", x["q"], golden["step:q"][n])
    within("reward", np.stack(r.rewards), golden["step:reward"])
    m = engine.replay_memory
    assert (m.position, m.count_seen) == (int(golden["replay:position"]), int(golden["replay:count_seen"]))
    assert np.array_equal(m.actions.cpu().numpy(), golden["replay:actions"])
    within("reward", m.rewards.cpu().numpy(), golden["replay:rewards"])
    assert (engine.steps, engine.episode, engine.epsilon) == (int(golden["steps"]), int(golden["episode"]), float(golden["epsilon"]))
    assert engine.target_updates == golden["target_copies"].tolist() == list(dt.TARGET_COPIES)
    within("ave", engine.ave_reward[:3].cpu().numpy(), golden["ave_reward"])
    within("ave", engine.ave_recon[:3].cpu().numpy(), golden["ave_recon"])
    assert float(engine.ave_recon[3:].abs().sum()) == 0.0
    for name, sd in r.end.items():
        for k, v in sd.items():
            want = golden[f"wsum:{name}:{k}"]
            e = float(np.abs(dt.weight_sums(v.numpy()) - want).max() / want[1])
            worst["weight sums"] = max(worst.get("weight sums", 0.0), e)
            assert e < TOL, f"{what}: the sums of {k} of the {name} net differ by {e:.2e} of the sum of magnitudes"
    for k in dt.STORED_WEIGHTS:
        within("weights", r.end["policy"][k].numpy(), golden["w:" + k])
    assert len(r.seen) == 1 + dt.BUDGET and len(r.valid_rows) == dt.BUDGET
    for i, obs in enumerate(r.seen):
        within("score", obs["score"].cpu().numpy(), golden[f"valid:{i}:score"])
        assert torch.equal(obs["mask"].cpu(), torch.from_numpy(golden[f"valid:{i}:mask"]))
        if i:
            row = r.valid_rows[i - 1]
            assert not row["random"] and row["epsilon"] == -1 and np.array_equal(row["action"], golden[f"valid:{i}:actions"]), (i, row["action"])
            within("q", row["q"], golden[f"valid:{i}:q"])
    assert np.array_equal(engine.chosen.numpy(), np.stack([golden[f"valid:{i}:actions"] for i in (1, 2)], axis=1).astype(np.float32))
    e = abs(float(engine.current_loss) - float(golden["current_loss"])) / float(golden["current_loss"])
    worst["current_loss"] = e
    assert e < TOL
    print(f"\n{what}: worst relative differences {({k: f'{v:.2e}' for k, v in worst.items()})}")
    return worst


@pytest.mark.parametrize("device_replay", [False, True], ids=["host_replay", "device_replay"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "modules"])
def test_engine_replays_the_reference(cuda, golden, locations, sensor_records, monkeypatch, tmp_path, fused, device_replay):
    """Measured on an MI355X (relative; bound 1e-4), fused / modules, the same with host and device replay: losses 1.62e-6 / 1.62e-6,
    Q rows 3.06e-7 / 2.30e-7, rewards 2.48e-6 / 2.48e-6, ``ave_*`` 8.27e-7 / 8.27e-7, weight sums 7.52e-9 / 7.74e-9, stored weights
    6.80e-7 / 7.85e-7, scores 1.16e-7 / 1.16e-7, ``current_loss`` 0 / 0 (to the printed digits)."""
    from a3vt_amd.pterotactyl.policies import recorded
    from a3vt_amd.pterotactyl.policies.DDQN import train as dtr
    ops.ddqn_latent_launches(reset=True)
    r = replay(golden, locations, sensor_records, monkeypatch, tmp_path, fused_q_latent=fused, replay_device="cuda" if device_replay else None)
    counts = ops.ddqn_latent_launches()
    engine = r.engine
    assert engine.replay_memory.mask.is_cuda is device_replay
    compare(golden, r, f"fused_q_latent={fused} device_replay={device_replay}")
    # the learner's own launches: four updates of three launches, and one per greedy choice (three in training, two in validation);
    # logging the Q rows adds one q launch per logged decision (6 + 2)
    greedy = sum(not x["random"] for x in r.rows) + dt.BUDGET
    assert counts == ({"q": greedy + dt.STEPS + dt.BUDGET, "update": 4 * 3} if fused else {"q": 0, "update": 0})
    assert engine.policy.optimizer.library_steps == 4
    assert engine.policy.copied == ([((2,), torch.int32)] * greedy if fused else [])
    # checkpoint, then a second engine resumes and goes on with the stored steps / epsilon
    engine.check_values_and_save()
    for name in ("best_model", "recent_model", "best_replay_buffer.pt", "recent_replay_buffer.pt"):
        assert os.path.exists(os.path.join(engine.checkpoint_dir, name)), name
    second = dtr.Engine(dt.engine_args(fused_q_latent=fused, replay_device="cuda" if device_replay else None, **locations),
                        sampler=recorded.RecordedSampler(sensor_records))
    setup(second, engine.env, 77)
    second.resume()
    assert (second.steps, second.epsilon, second.episode, second.epoch) == (engine.steps, engine.epsilon, engine.episode + 1, engine.epoch + 1)
    for a, b in ((second.policy, engine.policy), (second.target_net, engine.target_net)):
        assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))
    assert second.replay_memory.mask.is_cuda is device_replay and second.replay_memory.count_seen == engine.replay_memory.count_seen
    assert torch.equal(second.replay_memory.latent.cpu(), engine.replay_memory.latent.cpu())
    log = dt.LoopLog(second, q_of)
    second.train(su.batches("train")[:1])
    assert second.steps == engine.steps + dt.BUDGET and [x["epsilon"] for x in log.rows] == [0.05, 0.05]
    assert not any(np.isnan(x["loss"]) for x in log.rows) and second.policy.optimizer.library_steps == 2
