"""``ActiveTouch`` with ``args.touch_table`` on the GPU: one ``sample_table`` call and one touch-encoder forward per episode, then every
step, check and candidate phase gathered from the table by ``ops.touch_assemble``.  Fixture ``golden/g18_active_touch.npz`` and the
recipe of ``env_util.py``, as ``test_gpu_active_touch.py`` uses them.

Bounds: against the fixture that file's 1e-4 relative (``helpers.rel_err``); between the table and the plain path 1e-5 on vertices and
1e-4 on scores, rewards and candidate tables, the bounds ``test_batched_against_the_loop`` holds for the same arithmetic in a batch of
another composition — the charts of the two paths come from touch-encoder forwards of different batch sizes (E * A * F views at once
against E * F or K * E * F) and are otherwise the same numbers.  Everything that involves no such difference is compared with
``torch.equal``.

Seen on an MI355X: against the fixture at most 2.6e-6 (rewards; vertices 1.2e-6, scores 1.6e-7, tables 2.4e-7); table against
plain path vertices 5.2e-7, scores 1.2e-7, rewards 2.4e-6, candidate tables equal.  15 tests, 6 s."""
import random

import numpy as np
import pytest
import torch

import env_util as eu
import touch_render_util as tu
from a3vt_amd import mesh
from golden_util import load
from helpers import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load(eu.FIXTURE)


@pytest.fixture(autouse=True)
def restore_process_flags():
    yield from eu.kept_process_flags()


@pytest.fixture(scope="module")
def checkpoints(cuda, golden, tmp_path_factory):
    return {case: eu.package_models(case, golden, tmp_path_factory.mktemp(f"table_{case}"), prefix=f"{case}:") for case in eu.CASES}


@pytest.fixture
def candidates_seen(monkeypatch):
    """Every ``(K, E)`` candidate array ``environment.candidate_actions`` returned, in order (the table asks no sampler, so no
    sampler log holds them)."""
    from a3vt_amd.pterotactyl.policies import environment
    seen, real = [], environment.candidate_actions

    def recording(mask, num_actions, greedy_checks=None):
        out = real(mask, num_actions, greedy_checks)
        seen.append(np.array(out[0]))
        return out
    monkeypatch.setattr(environment, "candidate_actions", recording)
    return seen


def make_env(case, golden, checkpoints, monkeypatch, sampler=None, **knobs):
    from a3vt_amd.pterotactyl.policies import environment, recorded

    class CountingSampler(recorded.RecordedSampler):
        samples = tables = 0

        def sample(self, actions, touch_point_cloud=False, **kw):
            self.samples += 1
            return super().sample(actions, touch_point_cloud=touch_point_cloud, **kw)

        def sample_table(self, num_actions, fingers=None, to_host=None):
            self.tables += 1
            return super().sample_table(num_actions, fingers=fingers, to_host=to_host)

    monkeypatch.setattr(environment.ActiveTouch, "get_loaders", lambda self: None)
    sampler = CountingSampler(eu.case_records(case, golden[f"{case}:status"])) if sampler is None else sampler
    env = environment.ActiveTouch(eu.env_args(case, **checkpoints[case], **knobs), sampler=sampler)
    env.score_samples = eu.score_samples(golden, prefix=f"{case}:")
    return env


def batch(case, golden):
    return eu.batch_of(torch.from_numpy(golden[f"{case}:gt"]))


def run_calls(env, case, golden, seen):
    """The fixture's call sequence of a case: [(obs, reward, done, actions, table, candidates)]."""
    c = eu.CASES[case]
    out = []
    random.seed(0)
    for i, call in enumerate(c["calls"]):
        reward = done = actions = table = cands = None
        if call == "reset":
            obs = env.reset(batch(case, golden))
        elif call == "best":
            actions, obs, reward, done = env.best_step(greedy_checks=c["greedy_checks"])
            table, cands = env.candidate_scores, seen[-1]
        else:
            actions = torch.from_numpy(golden[f"{case}:{i}:actions"]).numpy()
            obs, reward, done = env.step(actions)
        out.append((obs, reward, done, actions, table, cands))
    return out


@pytest.mark.parametrize("batched", [True, False], ids=["batched", "loop"])
@pytest.mark.parametrize("case", sorted(eu.CASES))
def test_replays_the_reference_from_the_table(cuda, golden, checkpoints, monkeypatch, candidates_seen, case, batched):
    """Test 1: the reference's observations, rewards, decisions and candidate score tables with ``touch_table=True``."""
    c, z = eu.CASES[case], golden
    env = make_env(case, z, checkpoints, monkeypatch, batched_greedy=batched, touch_table=True)
    worst = {}

    def close(what, got, want, tol=1e-4):
        e = rel_err(torch.as_tensor(got), torch.from_numpy(np.asarray(want)))
        worst[what] = max(worst.get(what, 0.0), e)
        assert e < tol, f"case {case} call {i}: {what} differs by {e:.2e} (relative)"

    calls = run_calls(env, case, z, candidates_seen)
    assert env.sampler.samples == 0 and env.sampler.tables == 1
    for i, (obs, reward, done, actions, table, cands) in enumerate(calls):
        key = f"{case}:{i}:"
        assert set(obs) == {"score", "first_score", "mask", "names", "mesh"} | ({"latent", "first_latent"} if c["use_latent"] else set())
        assert all(not t.is_cuda for t in obs.values() if isinstance(t, torch.Tensor))
        assert torch.equal(obs["mask"], torch.from_numpy(z[key + "mask"]))
        close("score", obs["score"], z[key + "score"])
        close("first_score", obs["first_score"], z[key + "first_score"])
        close("verts", obs["mesh"][:, ::16, :3], z[key + "mesh_sub"][..., :3])
        assert torch.equal(obs["mesh"][:, ::16, 3], torch.from_numpy(z[key + "mesh_sub"][..., 3]))
        if c["use_latent"]:
            close("latent", obs["latent"], z[key + "latent"])
            close("first_latent", obs["first_latent"], z[key + "first_latent"])
        if reward is not None:
            close("reward", reward, z[key + "reward"])
            assert bool(done) == bool(z[key + "done"])
            assert np.array_equal(np.asarray(actions), z[key + "actions"]), (i, actions, z[key + "actions"])
        if table is not None:
            assert np.array_equal(cands, z[key + "cands"]), "the candidates are not the reference's"
            assert tuple(table.shape) == z[key + "table"].shape and not table.is_cuda
            close("table", table, z[key + "table"])
    final = calls[-1][0]["mesh"]
    close("final verts", final[..., :3], z[f"{case}:mesh"][..., :3])
    assert torch.equal(final[..., 3], torch.from_numpy(z[f"{case}:mesh"][..., 3]))
    print(f"case {case} {'batched' if batched else 'loop'} table: worst relative errors " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_table_against_the_plain_path(cuda, golden, checkpoints, monkeypatch, candidates_seen):
    """Test 2: case (a), the same calls with the knob on and off."""
    runs = {on: run_calls(make_env("a", golden, checkpoints, monkeypatch, touch_table=on), "a", golden, candidates_seen) for on in (False, True)}
    for i, (got, want) in enumerate(zip(runs[True], runs[False])):
        e_v, e_s = rel_err(got[0]["mesh"][..., :3], want[0]["mesh"][..., :3]), rel_err(got[0]["score"], want[0]["score"])
        print(f"table call {i}: verts {e_v:.2e} score {e_s:.2e}")
        assert e_v < 1e-5 and e_s < 1e-4
        assert torch.equal(got[0]["mesh"][..., 3], want[0]["mesh"][..., 3]) and torch.equal(got[0]["mask"], want[0]["mask"])
        if want[3] is not None:
            assert np.array_equal(got[3], want[3]) and got[2] == want[2]
            e_r, e_t = rel_err(got[1], want[1]), rel_err(got[4], want[4])
            print(f"table call {i}: reward {e_r:.2e} candidate table {e_t:.2e}")
            assert e_r < 1e-4 and e_t < 1e-4 and np.array_equal(got[5], want[5])


def test_the_sampler_leaves_the_loop(cuda, golden, checkpoints, monkeypatch):
    """Test 3: one ``sample_table`` call per ``reset`` and no ``sample`` call at all; a step, a check and a greedy step are library
    launches (one per call or candidate chunk)."""
    from a3vt_amd import ops
    env = make_env("a", golden, checkpoints, monkeypatch, touch_table=True)
    count = lambda: (env.sampler.tables, env.sampler.samples)  # noqa: E731
    assert count() == (0, 0)
    env.reset(batch("a", golden))
    assert count() == (1, 0)
    ops.touch_assemble_launches(reset=True)
    env.best_step()
    assert ops.touch_assemble_launches() == {"calls": 2}             # the four candidates in one launch, the step in another
    env.check_step(np.array([2, 3]))
    env.step(np.array([3, 2]))
    assert count() == (1, 0) and ops.touch_assemble_launches() == {"calls": 4}
    env.reset(batch("a", golden))
    assert count() == (2, 0)
    # the plain path, for contrast: the same calls ask the sampler every time
    plain = make_env("a", golden, checkpoints, monkeypatch)
    plain.reset(batch("a", golden))
    plain.best_step()
    assert (plain.sampler.tables, plain.sampler.samples) == (0, 4 + 1)


@pytest.mark.parametrize("case", sorted(eu.CASES))
def test_the_table_is_what_one_encoder_call_makes(cuda, golden, checkpoints, monkeypatch, case):
    """Test 4: ``table_charts`` / ``table_codes`` against ``scoring.touch_slots`` on the sampler's ``sample([a] * E)`` signals of all
    actions, stacked in (e, a, f) order, through ``_signals``' image arithmetic, as one batch.  Case (a) is the ``finger``
    topology, (b) the four fingers."""
    from a3vt_amd.pterotactyl.policies import scoring
    c = eu.CASES[case]
    F, A = (1 if c["finger"] else 4), c["num_actions"]
    fingers = [1] if c["finger"] else [0, 1, 2, 3]
    env = make_env(case, golden, checkpoints, monkeypatch, touch_table=True)
    env.reset(batch(case, golden))
    assert env.table_charts.shape == (eu.E, A, F, 25, 3) and env.table_codes.shape == (eu.E, A, F)
    assert env.table_codes.dtype == torch.int32 and env.table_charts.is_cuda and env.table_codes.is_cuda
    per_action = [env.sampler.sample([a] * eu.E) for a in range(A)]
    stack = lambda key: torch.stack([r[key][:, fingers] for r in per_action], dim=1)  # noqa: E731
    status = [[[r["touch_status"][e][f] for f in fingers] for r in per_action] for e in range(eu.E)]
    charts, masks = scoring.touch_slots(env.touch_prediction, env._images(stack("touch_signal")),
                                        {"rot": stack("finger_transform_rot_M").to(cuda), "pos": stack("finger_transfrom_pos").to(cuda)},
                                        status, env.touch_verts)
    assert torch.equal(env.table_charts, charts)
    assert torch.equal(env.table_codes, masks[..., 0, 0].to(torch.int32)) and len(torch.unique(env.table_codes)) == 3
    # ... and _signals of one sample is that arithmetic
    assert torch.equal(env._signals(per_action[1])[0], env._images(per_action[1]["touch_signal"][:, fingers]))


@pytest.mark.parametrize("batched", [True, False], ids=["batched", "loop"])
@pytest.mark.parametrize("case", sorted(eu.CASES))
def test_candidates_leave_no_trace(cuda, golden, checkpoints, monkeypatch, candidates_seen, case, batched):
    """Test 5: ``check_step`` and ``greedy_choice`` leave the touch state, the table and ``steps`` bit-identical."""
    c = eu.CASES[case]
    env = make_env(case, golden, checkpoints, monkeypatch, batched_greedy=batched, touch_table=True)
    random.seed(0)
    env.reset(batch(case, golden))
    env.step(np.array([1, 0]))

    def state():
        return (env.touch_charts.clone(), env.touch_masks.clone(), env.table_charts.clone(), env.table_codes.clone(),
                env.current_data["mask"].clone(), env.current_data["score"].clone(), env.current_data["first_score"].clone(), env.steps)

    before = state()
    assert before[0].abs().sum() > 0 and env.steps == 1
    obs = env.check_step(np.array([2, 3]))
    after_check = state()
    actions, table = env.greedy_choice(c["greedy_checks"])
    after_choice = state()
    for after in (after_check, after_choice):
        assert all(torch.equal(a.view(torch.int32) if a.is_floating_point() else a, b.view(torch.int32) if b.is_floating_point() else b)
                   for a, b in zip(before[:7], after[:7])) and after[7] == before[7]
    assert obs["score"].shape == (eu.E,) and table.shape[1] == eu.E and len(actions) == eu.E
    # the step that follows sees what the candidates saw: its score is the chosen candidate's
    k = [candidates_seen[-1][:, e].tolist().index(int(actions[e])) for e in range(eu.E)]
    nxt, _, _ = env.step(actions)
    assert rel_err(nxt["score"], torch.stack([table[k[e], e] for e in range(eu.E)])) < 1e-4
    assert env.steps == 2 and env.touch_charts.shape == before[0].shape and env.touch_masks.shape == before[1].shape


def sphere(level, radius, ahead):
    v, f = mesh.icosphere(level, radius)
    return (v.astype(np.float64) + tu.POS + ahead * tu.ROT[:, 0]).astype(np.float32), f.astype(np.int32)


@pytest.mark.parametrize("to_host", [True, False], ids=["to_host", "on_device"])
def test_rendered_and_recorded_agree(cuda, golden, checkpoints, monkeypatch, to_host):
    """Test 6: the scene and frames of ``test_gpu_rendered_env.py``, knob on: an environment on ``RenderedSampler`` and one on a
    ``RecordedSampler`` that replays the same signals are the same environment."""
    from a3vt_amd.pterotactyl.policies import recorded, rendered
    A = eu.CASES["a"]["num_actions"]
    geometry = dict(zip(eu.OBJECTS, (sphere(1, 0.004, 0.015), sphere(2, 0.006, 0.02))))
    pos, rot = np.tile(tu.POS, (4, 1)), np.tile(tu.ROT, (4, 1, 1))
    frames = {(o, a): (pos + 0.0004 * a, rot, np.array([True, True, a != 2, True])) for o in eu.OBJECTS for a in range(A)}
    sampler = rendered.RenderedSampler(frames, geometry, to_host=to_host)
    env = make_env("a", golden, checkpoints, monkeypatch, sampler=sampler, touch_table=True)
    env.reset(batch("a", golden))
    assert env.table_codes.shape == (eu.E, A, 1) and (env.table_codes == 2).any()
    signals = rendered.RenderedSampler(frames, geometry)
    signals.load_objects(batch("a", golden)["names"])
    signals = signals.sample_many([[a] * eu.E for a in range(A)])
    records = {(o, a): {"touch": signals[a]["touch_signal"][e], "pos": signals[a]["finger_transfrom_pos"][e],
                        "rot": signals[a]["finger_transform_rot_M"][e], "status": signals[a]["touch_status"][e]}
               for e, o in enumerate(eu.OBJECTS) for a in range(A)}
    replay = make_env("a", golden, checkpoints, monkeypatch, sampler=recorded.RecordedSampler(records), touch_table=True)
    replay.reset(batch("a", golden))
    assert torch.equal(env.table_charts, replay.table_charts) and torch.equal(env.table_codes, replay.table_codes)
    actions = np.array([1, 3])
    (obs, reward, _), (obs_r, reward_r, _) = env.step(actions), replay.step(actions)
    assert torch.isfinite(obs["mesh"]).all() and torch.equal(obs["mesh"], obs_r["mesh"]) and torch.equal(reward, reward_r)
    (choice, table), (choice_r, table_r) = env.greedy_choice(), replay.greedy_choice()
    assert torch.equal(table, table_r) and np.array_equal(choice, choice_r) and table.shape == (A, eu.E)


def test_the_knob_needs_a_sampler_that_builds_tables(cuda, golden, checkpoints, monkeypatch):
    """Test 7: ``touch_table=True`` with a sampler without ``sample_table`` is a ``ValueError`` naming both; unset, the same sampler
    is accepted."""
    class Plain:
        def load_objects(self, *a, **k):
            pass
        sample = disconnect = load_objects

    with pytest.raises(ValueError, match="touch_table.*Plain.*sample_table"):
        make_env("a", golden, checkpoints, monkeypatch, sampler=Plain(), touch_table=True)
    env = make_env("a", golden, checkpoints, monkeypatch, sampler=Plain())
    assert not env._use_table() and not hasattr(env, "table_charts")
