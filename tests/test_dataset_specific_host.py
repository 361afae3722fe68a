"""Host-side parts of the dataset-specific policies LEBA and MFBA (no GPU): the NumPy form of ``ops.candidate_tally`` against the
literal restatement ``tally_util.contract`` on the kernel tests' cases, its refusals, and the engines on a stub environment —
checkpoints in both directions and under both file names, resume at ``spot``, the pretrained file names, the swept batches, the
draws of LEBA's limited search, the two forms of a swept batch against each other, and the reference's import names."""
import os
import random
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tally_util as tu
from a3vt_amd import ops
from a3vt_amd.pterotactyl.policies import environment
from a3vt_amd.pterotactyl.policies.dataset_specific import LEBA, MFBA

CASES = tu.cases()
ENGINES = {"LEBA": LEBA, "MFBA": MFBA}


def t(x, dtype):
    return None if x is None else torch.as_tensor(np.array(x), dtype=dtype)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_host_form_matches_the_restatement_bit_for_bit(c):
    if c["taken"] is None and c["sums"] is None and c["votes"] is None:
        pytest.fail("a case without a way to know A")
    sums, checks, votes = (t(c[n], torch.float64) for n in ("sums", "checks", "votes"))
    taken = t(c["taken"], torch.float32)
    best, best_score = ops.candidate_tally(t(c["scores"], torch.float32), t(c["candidates"], torch.int32), t(c["first"], torch.float32),
                                           taken, sums=sums, checks=checks, votes=votes)
    want = tu.contract(c["scores"], c["candidates"], c["first"], c["taken"], c["A"], c["sums"], c["checks"], c["votes"])
    assert best.dtype == torch.int32 and best_score.dtype == torch.float32
    assert np.array_equal(best.numpy(), want[0]) and np.array_equal(tu.bits(best_score.numpy()), tu.bits(want[1]))
    for got, w in zip((sums, checks, votes), want[2:]):
        assert (got is None) == (w is None)
        if got is not None:
            assert np.array_equal(got.numpy(), w)


def test_the_reference_s_add_is_an_fp32_add():
    """``np.float64 + <0-d fp32 tensor>`` defers to torch and gives an fp32 tensor: what the contract's tally restates."""
    a = np.array([1.0, 0.1])
    s = torch.tensor([0.1, 0.7], dtype=torch.float32)
    a[1] += s[1]
    assert a[1] == np.float64(np.float32(np.float32(0.1) + np.float32(0.7))) and a[1] != 0.1 + float(np.float32(0.7))


def test_refusals():
    c = next(c for c in CASES if c["id"] == "shape-6x2x6")
    good = dict(scores=t(c["scores"], torch.float32), candidates=t(c["candidates"], torch.int32), first_score=t(c["first"], torch.float32),
                taken=t(c["taken"], torch.float32), sums=t(c["sums"], torch.float64), checks=t(c["checks"], torch.float64),
                votes=t(c["votes"], torch.float64))
    ops.candidate_tally(**{k: (v.clone() if v is not None else v) for k, v in good.items()})
    outside = c["candidates"].copy()
    outside[2, 1] = 6
    below = c["candidates"].copy()
    below[0, 0] = -1
    bad = [("scores", good["scores"].double(), "scores"), ("candidates", good["candidates"].long(), "candidates"),
           ("candidates", good["candidates"][:5], r"\(K, E\)"), ("first_score", good["first_score"][:1], "first_score"),
           ("first_score", None, "first_score"), ("taken", good["taken"][:1], "taken"), ("taken", good["taken"].double(), "taken"),
           ("sums", good["sums"].float(), "sums"), ("checks", None, "together"), ("sums", None, "together"),
           ("votes", good["votes"][:5], "number of actions"), ("votes", good["votes"].view(2, 3), "votes"),
           ("candidates", t(outside, torch.int32), r"outside \[0, 6\): min 0, max 6"),
           ("candidates", t(below, torch.int32), r"outside \[0, 6\): min -1")]
    for name, value, match in bad:
        with pytest.raises(ValueError, match=match):
            ops.candidate_tally(**dict(good, **{name: value}))
    with pytest.raises(ValueError, match="number of actions A"):
        ops.candidate_tally(good["scores"], good["candidates"], None, None)
    for K, E, A, match in ((305, 1, 4, "K=305"), (1, 1025, 4, "E=1025"), (1, 1, 305, "A=305")):
        with pytest.raises(ValueError, match=match):
            ops.candidate_tally(torch.ones(K, E), torch.zeros(K, E, dtype=torch.int32), None, torch.zeros(E, A))
    assert np.array_equal(good["sums"].numpy(), c["sums"])                        # a refused call changes nothing


# ---- the engines on a stub environment --------------------------------------------------------------------------------------------

def engine_args(**kw):
    d = dict(num_actions=6, num_grasps=5, env_batch_size=2, budget=3, greedy_checks=6, seed=0, eval=False, pretrained=False,
             use_img=False, finger=False, exp_type="t", visualize=False, fused_tally=False)
    d.update(kw)
    return SimpleNamespace(**d)


class StubEnv:
    """Scores that are a seeded function of (batch, steps taken, element, action); the table is fp32 on the "device" (the CPU)."""
    device = torch.device("cpu")

    def __init__(self, args):
        self.args, self.log = args, []

    def _score(self, actions):
        g = np.random.default_rng([self.batch, self.steps] + [int(a) for a in actions])
        return torch.from_numpy(g.uniform(0.5, 3.0, self.args.env_batch_size).astype(np.float32))

    def reset(self, batch):
        self.batch, self.steps = batch["id"], 0
        self.log.append(("reset", self.batch))
        g = np.random.default_rng(1000 + self.batch)
        self.current_data = {"first_score": torch.from_numpy(g.uniform(3.0, 6.0, self.args.env_batch_size).astype(np.float32)),
                             "mask": torch.zeros(self.args.env_batch_size, self.args.num_actions)}
        return {"score": self.current_data["first_score"].clone()}

    def step(self, actions):
        self.log.append(("step", self.batch, list(actions)))
        for e, a in enumerate(actions):
            self.current_data["mask"][e, a] = 1
        self.steps += 1
        return {"score": self._score(actions)}, None, self.steps == self.args.budget

    def score_candidates(self, candidates, to_host=True):
        self.log.append(("score", self.batch, [list(row) for row in candidates], to_host))
        return torch.stack([self._score(row) for row in candidates])

    def greedy_choice(self, greedy_checks=None):
        candidates, full = environment.candidate_actions(self.current_data["mask"], self.args.num_actions, greedy_checks)
        scores = self.score_candidates(candidates)
        return environment.choose_actions(scores, candidates, self.current_data["mask"], full), scores


def stub_engine(module, tmp_path, **kw):
    args = engine_args(**kw)
    engine = module.Engine(args)
    engine.env = StubEnv(args)
    engine.checkpoint_dir = str(tmp_path / "experiments" / "checkpoint" / module.Engine.name / "t")
    os.makedirs(engine.checkpoint_dir, exist_ok=True)
    engine.checkpoint = os.path.join(engine.checkpoint_dir, "actions.npy")
    engine.chosen_actions, engine.step, engine.spot = [], 0, 0
    engine.reset_state()
    return engine


BATCHES = [{"id": v, "names": [f"o{v}_0", f"o{v}_1"]} for v in range(10)]


@pytest.mark.parametrize("seed", [0, 3])
@pytest.mark.parametrize("name", ["LEBA", "MFBA"])
def test_train_sweeps_the_reference_s_batches_and_saves_every_twenty(tmp_path, name, seed):
    n = 60
    random.seed(seed)
    swept = random.sample(range(n), int(n * 0.4))                                 # reference LEBA.py:87-90
    engine = stub_engine(ENGINES[name], tmp_path, seed=seed)
    saves = []
    engine.save = lambda: saves.append(engine.spot)
    engine.train([{"id": v} for v in range(n)])
    assert [e[1] for e in engine.env.log if e[0] == "reset"] == sorted(swept)
    assert saves == [v for v in sorted(swept) if v % 20 == 0]
    assert len(engine.chosen_actions) == 1 and engine.step == 1 and engine.spot == 0


def run_sweeps(module, tmp_path, fused, sweeps=3, greedy_checks=(6, 3, 6)):
    engine = stub_engine(module, tmp_path, fused_tally=fused)
    history = []
    for s in range(sweeps):
        engine.args.greedy_checks = greedy_checks[s]
        engine.train(BATCHES)
        engine.save()
        history.append(np.load(engine.checkpoint, allow_pickle=True).item())
    return engine, history


@pytest.mark.parametrize("name", ["LEBA", "MFBA"])
def test_the_two_forms_of_a_swept_batch_agree_bit_for_bit(tmp_path, name):
    """Knob on (here: ``ops.candidate_tally``'s host form on CPU tensors) against the reference's loop: the same candidates drawn,
    the same state after every sweep, the same checkpoints."""
    module = ENGINES[name]
    on, saved_on = run_sweeps(module, tmp_path / "on", True)
    off, saved_off = run_sweeps(module, tmp_path / "off", False)
    assert [e for e in on.env.log if e[0] != "score"] == [e for e in off.env.log if e[0] != "score"]
    assert [e[:3] for e in on.env.log if e[0] == "score"] == [e[:3] for e in off.env.log if e[0] == "score"]
    assert all(e[3] is False for e in on.env.log if e[0] == "score") and all(e[3] for e in off.env.log if e[0] == "score")
    assert on.chosen_actions == off.chosen_actions and len(set(on.chosen_actions)) == 3
    for a, b in zip(saved_on, saved_off):
        assert set(a) == set(b)
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    state = on._state[module.Engine.state_names[0]]
    assert isinstance(state, torch.Tensor) and state.dtype == torch.float64
    assert isinstance(off._state[module.Engine.state_names[0]], np.ndarray)
    for attr in module.Engine.state_names:
        got = getattr(on, attr)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and np.array_equal(got, getattr(off, attr))


def test_leba_tally_is_the_reference_s_loop(tmp_path):
    """One sweep by hand: reference LEBA.py:103-134 on the stub's numbers."""
    engine = stub_engine(LEBA, tmp_path, greedy_checks=3)
    engine.chosen_actions = [np.int64(4)]
    engine.reset_state()
    engine.train(BATCHES)
    env = StubEnv(engine.args)
    scores = np.array([1e10 if i != 4 else 1e20 for i in range(6)])
    checks = np.ones(6)
    random.seed(0)
    swept = random.sample(range(10), 4)                                           # :87-90; the candidates' draws follow it
    for v in sorted(swept):
        env.reset({"id": v})
        env.step(np.array([4, 4]))
        remaining = [[i for i in range(6) if i != 4] for _ in range(2)]
        remaining = [random.sample(r, 3) for r in remaining]                       # :109-113, element order
        for i in range(3):
            actions = [remaining[j][i] for j in range(2)]
            ratio = env._score(actions) / env.current_data["first_score"]
            for action, score in zip(actions, ratio):
                if scores[action] == 1e10:
                    scores[action] = score
                else:
                    scores[action] += score
                checks[action] += 1.0
    assert engine.chosen_actions == [4, int(np.argmin(scores / checks))]
    assert list(engine.action_scores) == [1e10 if i not in engine.chosen_actions else 1e20 for i in range(6)]
    assert list(engine.checks) == [1.0] * 6 and engine.spot == 0 and engine.step == 1


def tu_swept(n, seed):
    from a3vt_amd.pterotactyl.policies.dataset_specific import _engine
    return _engine.swept_batches(n, seed)


def test_leba_limited_search_consumes_random_as_the_reference():
    random.seed(11)
    got = LEBA.remaining_candidates([2, 5], 8, 3, 4)
    after = random.random()
    random.seed(11)
    left = [0, 1, 3, 4, 6, 7]                                                     # reference :103-113: one sample per element, in order
    drawn = [random.sample(left, 4), random.sample(left, 4), random.sample(left, 4)]
    assert got == [[drawn[e][k] for e in range(3)] for k in range(4)] and after == random.random()
    random.seed(11)
    assert LEBA.remaining_candidates([2, 5], 8, 3, 8) == [[a] * 3 for a in (0, 1, 3, 4, 6, 7)]        # full search: no draw
    assert random.random() == random.Random(11).random()


def test_mfba_votes_for_the_greedy_actions(tmp_path):
    for fused in (True, False):
        engine = stub_engine(MFBA, tmp_path / str(fused), fused_tally=fused)
        engine.chosen_actions = [np.int64(1)]
        engine.reset_state()
        assert list(engine.counts) == [0.0, -1e20, 0.0, 0.0, 0.0, 0.0]
        votes = np.zeros(6)
        env = StubEnv(engine.args)
        for v in sorted(tu_swept(10, 0)):
            env.reset({"id": v})
            env.step(np.array([1, 1]))
            table = torch.stack([env._score([k, k]) for k in range(6)]).numpy()
            table[1] = np.inf
            for e in range(2):
                votes[np.argmin(table[:, e])] += 1
        engine.train(BATCHES)
        assert engine.chosen_actions == [1, int(np.argmax(votes))] and engine.greedy_actions.shape == (2,)
        assert list(engine.counts) == [0.0 if i not in engine.chosen_actions else -1e20 for i in range(6)]


def test_mfba_refuses_an_element_without_an_open_action(tmp_path):
    """Full search and limited search (where ``candidate_actions`` has no candidate to offer), both forms alike."""
    for fused in (True, False):
        for greedy_checks in (6, 1):
            engine = stub_engine(MFBA, tmp_path / f"{fused}{greedy_checks}", fused_tally=fused, num_actions=2, greedy_checks=greedy_checks)
            engine.chosen_actions = [np.int64(0), np.int64(1)]
            with pytest.raises(RuntimeError, match="MFBA: element 0 has no action left"):
                engine.train(BATCHES)
            assert not [e for e in engine.env.log if e[0] == "score"]                 # refused before anything is scored


@pytest.mark.parametrize("name", ["LEBA", "MFBA"])
def test_checkpoints_round_trip_both_ways_and_under_both_names(tmp_path, name):
    module = ENGINES[name]
    engine, _ = run_sweeps(module, tmp_path, False, sweeps=1)
    engine.spot = 7
    engine.save()
    keys = {"LEBA": {"action_scores", "checks", "chosen_actions", "step", "spot"}, "MFBA": {"counts", "chosen_actions", "step", "spot"}}[name]
    data = np.load(engine.checkpoint, allow_pickle=True).item()                   # as the reference reads it (LEBA.py:238-243)
    assert set(data) == keys and data["spot"] == 7 and data["step"] == 1 and len(data["chosen_actions"]) == 1
    for key in module.Engine.state_names:
        assert isinstance(data[key], np.ndarray) and data[key].dtype == np.float64 and data[key].shape == (6,)
    # a dict in the reference's layout (LEBA.py:247-255, MFBA.py:213-220) ...
    theirs = {"chosen_actions": [np.int64(3), np.int64(0)], "step": 2, "spot": 4}
    if name == "LEBA":
        theirs.update(action_scores=np.array([1e20, 0.75, 1e10, 1e20, 2.5, 1e10]), checks=np.array([1.0, 2.0, 1.0, 1.0, 4.0, 1.0]))
    else:
        theirs.update(counts=np.array([-1e20, 2, 0, -1e20, 5, 0]))                # (the reference's array is an integer one after a sweep)
    for fused in (False, True):
        # ... under this package's name, and under the reference's (no separator) when the former is missing
        for path in (engine.checkpoint, engine.checkpoint_dir + "actions.npy"):
            if os.path.exists(engine.checkpoint):
                os.remove(engine.checkpoint)
            np.save(path, theirs)
            fresh = stub_engine(module, tmp_path, fused_tally=fused)
            assert fresh.location() == path
            fresh.load()
            assert fresh.chosen_actions == [3, 0] and (fresh.step, fresh.spot) == (2, 4)
            for key in module.Engine.state_names:
                got = getattr(fresh, key)
                assert got.dtype == np.float64 and np.array_equal(got, np.asarray(theirs[key], dtype=np.float64))
            os.remove(path)
    fresh = stub_engine(module, tmp_path)
    assert fresh.location() is None
    fresh.load()                                                                  # nothing to load: the fresh state, as the reference
    assert fresh.chosen_actions == [] and fresh.step == 0
    np.save(engine.checkpoint, dict(theirs, chosen_actions=[np.int64(6)]))
    with pytest.raises(ValueError, match="outside"):
        stub_engine(module, tmp_path).load()


@pytest.mark.parametrize("name", ["LEBA", "MFBA"])
def test_resume_at_spot(tmp_path, name):
    module = ENGINES[name]
    swept = sorted(tu_swept(10, 0))
    engine = stub_engine(module, tmp_path)
    engine.spot = swept[2]
    engine.save()
    resumed = stub_engine(module, tmp_path)
    resumed.load()
    assert resumed.spot == swept[2]
    resumed.train(BATCHES)
    assert [e[1] for e in resumed.env.log if e[0] == "reset"] == swept[2:]        # batch `spot` itself is swept again
    assert resumed.spot == 0 and resumed.step == 1


@pytest.mark.parametrize("name", ["LEBA", "MFBA"])
def test_pretrained_file_names(monkeypatch, name):
    monkeypatch.delenv("PTEROTACTYL_PRETRAINED", raising=False)
    module = ENGINES[name]
    for use_img, finger, kind in ((True, True, "v_t_p"), (True, False, "v_t_g"), (False, True, "t_p"), (False, False, "t_g")):
        e = module.Engine(engine_args(pretrained=True, use_img=use_img, finger=finger, pretrained_root="/models"))
        assert e.location() == os.path.join("/models", "policies", "dataset_specific", f"{name}_{kind}.npy")
    with pytest.raises(FileNotFoundError):
        module.Engine(engine_args(pretrained=True)).location()


@pytest.mark.parametrize("name", ["LEBA", "MFBA"])
def test_validate_replays_the_trajectory(tmp_path, name):
    engine = stub_engine(ENGINES[name], tmp_path)
    engine.chosen_actions = [np.int64(2), np.int64(5)]
    total = engine.validate(BATCHES[:3])
    steps = [e for e in engine.env.log if e[0] == "step"]
    assert [s[2] for s in steps] == [[2, 2], [5, 5]] * 3
    assert engine.names == [n for b in BATCHES[:3] for n in b["names"]]
    assert engine.scores.shape == (6, 3) and engine.chosen.tolist() == [[2.0, 5.0]] * 6
    assert abs(float(total["score"]) - float((engine.scores[:, -1] / engine.scores[:, 0]).mean())) < 1e-7


@pytest.mark.parametrize("name", ["LEBA", "MFBA"])
def test_parser_knob_and_visualize(monkeypatch, name):
    module = ENGINES[name]
    monkeypatch.setenv("PTEROTACTYL_PRETRAINED", "/somewhere/pretrained")
    args = module.get_parser().parse_args([])
    defaults = dict(limit_data=False, finger=False, number_points=30000, seed=0, env_batch_size=3, use_img=False, loss_coeff=9000.0,
                    num_grasps=5, num_actions=50, use_latent=False, use_recon=False, eval=False, budget=5, visualize=False,
                    exp_type="test", greedy_checks=50, pretrained_recon=False, pretrained=False)
    for key, value in defaults.items():
        assert getattr(args, key) == value and type(getattr(args, key)) is type(value), key
    assert args.touch_location == "/somewhere/pretrained/reconstruction/touch/best/"
    assert args.vision_location == "/somewhere/pretrained/reconstruction/vision/t_p/"
    assert (args.recorded, args.fused_tally) == (None, None)
    assert module.get_parser().parse_args(["--no_fused_tally"]).fused_tally is False
    assert module.get_parser().parse_args(["--fused_tally"]).fused_tally is True
    assert module.Engine(engine_args(fused_tally=None)).fused is module.FUSED_TALLY_DEFAULT
    monkeypatch.setattr(module, "FUSED_TALLY_DEFAULT", not module.FUSED_TALLY_DEFAULT)
    assert module.Engine(engine_args(fused_tally=None)).fused is module.FUSED_TALLY_DEFAULT
    with pytest.raises(NotImplementedError, match="visualize"):
        module.Engine(engine_args(visualize=True))()
    with pytest.raises(NotImplementedError, match="visualize"):
        module.Engine(engine_args(visualize=True)).validate([])
    assert callable(module.main)


def test_install_as_pterotactyl_registers_the_modules():
    import a3vt_amd
    kept = {k: v for k, v in sys.modules.items() if k == "pterotactyl" or k.startswith("pterotactyl.")}
    try:
        a3vt_amd.install_as_pterotactyl()
        from pterotactyl.policies.dataset_specific import LEBA as theirs_leba, MFBA as theirs_mfba
        import pterotactyl.policies.dataset_specific.LEBA as by_name
        assert theirs_leba is LEBA and theirs_mfba is MFBA and by_name is LEBA
    finally:
        for k in [k for k in sys.modules if k == "pterotactyl" or k.startswith("pterotactyl.")]:
            del sys.modules[k]
        sys.modules.update(kept)
