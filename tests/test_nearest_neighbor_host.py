"""Host-side parts of the nearest-neighbour latent policy (no GPU): ``ops._latent_nearest_torch`` against the literal NumPy
restatement of the contract (``nn_policy_util.contract``), ``Engine.choose`` against a literal restatement of the reference's
walk (``policies/NearestNeighbor/train.py:114-137``) on gapped inputs, the bank's file format in both directions, the refusals,
the parser's defaults, and ``train``'s batch selection and resume rule on a stub environment."""
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import nn_policy_util as nu
from a3vt_amd import ops
from a3vt_amd.pterotactyl.policies.NearestNeighbor import train as nn

# the reference's flags and defaults, restated from its train.py:223-311 (the three *_location defaults are paths inside its
# package and are compared by their tails); use_recon / use_latent are set after parsing (:314-315)
REFERENCE_DEFAULTS = dict(limit_data=False, finger=False, number_points=30000, seed=0, env_batch_size=3, use_img=False, loss_coeff=9000.0,
                          num_grasps=5, num_actions=50, eval=False, budget=5, visualize=False, exp_type="test", greedy_checks=50,
                          pretrained_recon=False, pretrained=False)
REFERENCE_LOCATIONS = dict(touch_location="reconstruction/touch/best/", vision_location="reconstruction/vision/t_p/",
                           auto_location="reconstruction/auto/t_p/")


def torch_form(bank, acts, queries, taken, k):
    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dt)   # noqa: E731
    out = ops._latent_nearest_torch(t(bank, torch.float32), t(acts, torch.int32), t(queries, torch.float32), t(taken, torch.float32), k)
    return [None if o is None else o.numpy() for o in out]


def gapped(bank_rows, dim, n_queries, k, seed, num_actions=30):
    bank, queries = nu.gapped_bank(bank_rows, dim, n_queries, k + 2, seed)
    g = np.random.default_rng(seed + 1)
    return bank, g.integers(0, num_actions, bank_rows).astype(np.int32), queries, (g.random((n_queries, num_actions)) < 0.5).astype(np.float32)


@pytest.mark.parametrize("bank_rows,dim,n_queries,k", [(1, 5, 1, 25), (7, 200, 1, 25), (101, 200, 3, 25), (101, 3, 3, 1), (300, 1, 3, 64),
                                                       (120, 257, 2, 25)])
def test_torch_form_against_the_contract(bank_rows, dim, n_queries, k):
    bank, acts, queries, taken = gapped(bank_rows, dim, n_queries, k, 10 + bank_rows)
    want = nu.contract(bank, acts, queries, taken, k)
    k_eff = min(k, bank_rows)
    assert min(nu.smallest_gap(r, k_eff) for r in want[1]) > 1e-3
    got = torch_form(bank, acts, queries, taken, k)
    assert got[0].dtype == np.int32 and got[2].dtype == np.int32 and got[3].dtype == np.int32 and got[1].dtype == np.float32
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert np.allclose(got[1][:, :k_eff], want[1][:, :k_eff], rtol=(dim + 4) * 2.0 ** -24, atol=0)
    assert (got[0][:, k_eff:] == -1).all() and np.isposinf(got[1][:, k_eff:]).all()


def test_torch_form_ties_nan_and_the_action_rule():
    bank, acts, queries, _ = gapped(60, 8, 1, 25, 40, num_actions=6)
    bank[[50, 3, 17]] = queries[0] + np.float32(0.001)                       # three bit-identical rows, the nearest
    bank[9, 1], bank[30, 0] = np.nan, np.inf
    got, want = torch_form(bank, acts, queries, None, 64), nu.contract(bank, acts, queries, None, 64)
    assert list(got[0][0, :3]) == [3, 17, 50] and list(got[0][0, 58:60]) == [30, 9] and (got[0][0, 60:] == -1).all()
    assert np.array_equal(got[0], want[0]) and np.isnan(got[1][0, 59]) and np.isposinf(got[1][0, 58])
    # the first listed row whose action is open; an action outside [0, A) never qualifies; nothing open: -1
    acts[[3, 17, 50]] = (6, -1, 2)
    taken = np.zeros((1, 6), dtype=np.float32)
    for mask, rank in ((taken, 2), (np.where(np.arange(6) == 2, 0.5, 0.0)[None].astype(np.float32), None), (taken + 1, -1)):
        got, want = torch_form(bank, acts, queries, mask, 25), nu.contract(bank, acts, queries, mask, 25)
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
        if rank is not None:
            assert got[3][0] == rank and (rank < 0) == (got[2][0] < 0)
    pure = torch_form(bank, None, queries, None, 25)
    assert pure[2] is None and pure[3] is None and np.array_equal(pure[0], want[0])


def test_disagreeing_operands_are_refused():
    bank, acts, queries, taken = (torch.from_numpy(a) for a in gapped(40, 8, 2, 5, 70))
    for bad in ((bank, acts, queries[:, :7], taken, 5), (bank, acts[:-1], queries, taken, 5), (bank, acts, queries, taken[:1], 5),
                (bank, acts.long(), queries, taken, 5), (bank.double(), acts, queries, taken, 5), (bank, acts, queries, taken, 65),
                (bank, acts, queries, taken, 0), (bank, None, queries, taken, 5), (bank[0], acts, queries, taken, 5)):
        with pytest.raises(RuntimeError, match="a3vt: "):
            ops.latent_nearest(*bad)


def cpu_engine(args):
    engine = nn.Engine(args)
    engine.device = "cpu"            # (None: the environment's GPU)
    return engine


def engine_args(**kw):
    d = dict(num_actions=6, num_grasps=5, env_batch_size=2, budget=3, greedy_checks=3, seed=0, eval=True, pretrained=False,
             use_img=False, finger=False, exp_type="t", visualize=False)
    d.update(kw)
    return SimpleNamespace(**d)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "loop"])
@pytest.mark.parametrize("bank_rows,E", [(7, 1), (120, 3)])
def test_choose_against_the_reference_walk(fused, bank_rows, E):
    """Gapped distances (asserted), so fp32 and fp64 order the bank alike; a bank smaller than k = 25 is searched whole (all
    its rows lie around the one query: another query's rows would be equally far from it)."""
    A, k = 6, 25
    bank, acts, queries, _ = gapped(bank_rows, 200, E, k, 90 + bank_rows, num_actions=A)
    if bank_rows < k:
        acts[:A] = np.arange(A)                                                   # every action is in the small bank
    engine = cpu_engine(engine_args(num_actions=A, env_batch_size=E, fused_lookup=fused))
    engine.bank.append(bank, acts)
    assert engine.actions == [int(a) for a in acts] and len(engine.latents) == bank_rows and engine.spot == 0
    g = np.random.default_rng(5)
    for step in range(4):
        mask = np.zeros((E, A), dtype=np.float32)
        for e in range(E):
            mask[e, g.choice(A, step, replace=False)] = 1
        full = nu.contract(bank, None, queries, None, min(k + 1, bank_rows))[1]
        assert min(nu.smallest_gap(r, k + 1) for r in full) > 1e-3
        want = [nu.reference_walk(bank, acts, queries[e], list(np.where(mask[e] != 0)[0]), k) for e in range(E)]
        assert None not in want
        got = engine.choose({"latent": torch.from_numpy(queries), "mask": torch.from_numpy(mask)})
        assert isinstance(got, np.ndarray) and got.shape == (E,) and list(got) == want, (step, got, want)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "loop"])
def test_no_open_action_among_the_nearest_names_element_and_step(fused):
    bank, _, queries, _ = gapped(80, 16, 2, 25, 120, num_actions=6)
    engine = cpu_engine(engine_args(fused_lookup=fused))
    engine.bank.append(bank, np.zeros(80, dtype=np.int64))                          # every entry says action 0
    mask = torch.zeros(2, 6)
    assert list(engine.choose({"latent": torch.from_numpy(queries), "mask": mask})) == [0, 0]
    mask[1, 0] = 1
    engine.steps_chosen = 2
    with pytest.raises(RuntimeError, match=r"element 1 at step 2"):
        engine.choose({"latent": torch.from_numpy(queries), "mask": mask})


def test_knob_default_follows_the_module():
    bank, acts, queries, _ = gapped(60, 16, 2, 25, 130, num_actions=6)
    engine = cpu_engine(engine_args())
    engine.bank.append(bank, acts)
    calls = []
    engine.bank.lookup = lambda *a, **k: calls.append(1) or np.zeros(2, dtype=np.int64)
    engine.choose({"latent": torch.from_numpy(queries), "mask": torch.zeros(2, 6)})
    assert bool(calls) == nn.FUSED_LOOKUP_DEFAULT


def test_bank_file_round_trip_both_ways(tmp_path):
    g = np.random.default_rng(3)
    latents, actions = g.standard_normal((5, 7)).astype(np.float32), [4, 0, 5, 5, 1]
    bank = nn.LatentBank(6)
    bank.append(latents[:2], actions[:2])
    bank.append(torch.from_numpy(latents[2:]), np.array(actions[2:]))
    bank.spot = 9
    path = str(tmp_path / "actions.npy")
    bank.save(path)
    # ... as the reference reads it (:209-212)
    data = np.load(path, allow_pickle=True).item()
    assert set(data) == {"actions", "latents", "spot"} and data["spot"] == 9
    assert list(data["actions"]) == actions and np.issubdtype(data["actions"].dtype, np.integer) and data["actions"].shape == (5,)
    assert data["latents"].dtype == np.float32 and np.array_equal(data["latents"], latents)
    assert [torch.FloatTensor(d) for d in data["latents"]][3].shape == (7,)
    # ... and a file the reference wrote (:216-220: np.array of the list of chosen actions, the stacked latents, spot)
    theirs = str(tmp_path / "theirs.npy")
    np.save(theirs, {"actions": np.array([np.int64(a) for a in actions]), "latents": latents, "spot": 3})
    back = nn.LatentBank(6).load(theirs)
    assert back.actions == actions and back.spot == 3 and all(isinstance(a, int) for a in back.actions)
    assert torch.equal(torch.stack(back.latents), torch.from_numpy(latents)) and len(back) == 5
    lat, act = back.to("cpu")
    assert lat.shape == (5, 7) and lat.dtype == torch.float32 and act.dtype == torch.int32 and act.tolist() == actions
    assert back.to("cpu")[0] is lat                                              # one upload, kept
    back.append(latents[:1], [2])
    assert back.to("cpu")[0].shape == (6, 7)
    assert list(back.lookup(latents[:2], np.zeros((2, 6), dtype=np.float32), 25, device="cpu")) == [4, 0]


def test_bank_refusals(tmp_path):
    bank = nn.LatentBank(6)
    with pytest.raises(RuntimeError, match="empty"):
        bank.lookup(np.zeros((1, 4), dtype=np.float32), np.zeros((1, 6), dtype=np.float32), 25, device="cpu")
    with pytest.raises(RuntimeError, match="empty"):
        bank.to("cpu")
    for bad in ([6], [-1], [0, 7], [1.5]):
        with pytest.raises(ValueError):
            bank.append(np.zeros((len(bad), 4), dtype=np.float32), bad)
    assert len(bank) == 0
    with pytest.raises(ValueError):
        bank.append(np.zeros((2, 4), dtype=np.float32), [1])
    bank.append(np.zeros((1, 4), dtype=np.float32), [1])
    with pytest.raises(ValueError):
        bank.append(np.zeros((1, 5), dtype=np.float32), [1])
    with pytest.raises(RuntimeError, match="mask"):
        bank.lookup(np.zeros((1, 4), dtype=np.float32), np.zeros((1, 5), dtype=np.float32), 25, device="cpu")
    path = str(tmp_path / "bad.npy")
    np.save(path, {"actions": np.array([0, 6]), "latents": np.zeros((2, 4), dtype=np.float32), "spot": 0})
    with pytest.raises(ValueError, match="outside"):
        nn.LatentBank(6).load(path)
    assert len(nn.LatentBank(7).load(path)) == 2


def test_where_the_bank_is_read_from(tmp_path, monkeypatch):
    engine = nn.Engine(engine_args())
    engine.checkpoint_dir = str(tmp_path / "experiments" / "checkpoint" / "t")
    os.makedirs(engine.checkpoint_dir)
    engine.checkpoint = os.path.join(engine.checkpoint_dir, "actions.npy")
    assert engine.bank_location() is None
    engine.load()                                                                  # nothing to load: an empty bank, as the reference
    assert len(engine.bank) == 0
    theirs = engine.checkpoint_dir + "actions.npy"                                 # the reference's name: no separator (:41)
    np.save(theirs, {"actions": np.array([2]), "latents": np.ones((1, 4), dtype=np.float32), "spot": 5})
    assert engine.bank_location() == theirs
    engine.load()
    assert engine.actions == [2] and engine.spot == 5
    engine.bank.append(np.zeros((1, 4), dtype=np.float32), [3])
    engine.save()
    assert engine.bank_location() == engine.checkpoint and os.path.exists(engine.checkpoint)
    fresh = nn.Engine(engine_args())
    fresh.checkpoint_dir, fresh.checkpoint = engine.checkpoint_dir, engine.checkpoint
    fresh.load()
    assert fresh.actions == [2, 3]
    # pretrained banks: the reference's (use_img, finger) rule (:180-202) under the pretrained root
    monkeypatch.delenv("PTEROTACTYL_PRETRAINED", raising=False)
    for use_img, finger, name in ((True, True, "v_t_p.npy"), (True, False, "v_t_g.npy"), (False, True, "t_p.npy"), (False, False, "t_g.npy")):
        e = nn.Engine(engine_args(pretrained=True, use_img=use_img, finger=finger, pretrained_root="/models"))
        assert e.bank_location() == os.path.join("/models", "policies", "NearestNeighbor", name)
    with pytest.raises(FileNotFoundError):
        nn.Engine(engine_args(pretrained=True)).bank_location()


def test_parser_defaults_are_the_reference_s(monkeypatch):
    monkeypatch.setenv("PTEROTACTYL_PRETRAINED", "/somewhere/pretrained")
    args = nn.get_parser().parse_args([])
    for name, value in REFERENCE_DEFAULTS.items():
        assert getattr(args, name) == value and type(getattr(args, name)) is type(value), name
    for name, tail in REFERENCE_LOCATIONS.items():
        assert getattr(args, name) == os.path.join("/somewhere/pretrained", tail), name
    assert (args.data_root, args.pretrained_root, args.recorded, args.fused_lookup) == (None, None, None, None)
    assert not hasattr(args, "use_latent") and not hasattr(args, "use_recon")                 # set after parsing, as the reference
    on = nn.get_parser().parse_args(["--eval", "--finger", "--pretrained", "--budget", "2", "--no_fused_lookup"])
    assert on.eval and on.finger and on.pretrained and on.budget == 2 and on.fused_lookup is False
    with pytest.raises(NotImplementedError):
        nn.Engine(engine_args(visualize=True))()
    with pytest.raises(NotImplementedError):
        nn.Engine(engine_args(visualize=True)).validate([])


class StubEnv:
    """Latents and greedy choices that name the batch and the step they come from."""

    def __init__(self, args):
        self.args, self.log = args, []

    def obs(self):
        return {"latent": torch.full((self.args.env_batch_size + 1, 4), 100.0 * self.batch + self.step) +
                torch.arange(self.args.env_batch_size + 1).view(-1, 1) * 0.25}

    def reset(self, batch):
        self.batch, self.step = batch["id"], 0
        self.log.append(("reset", self.batch))
        return self.obs()

    def best_step(self, greedy_checks=None):
        self.log.append(("best", self.batch, self.step, greedy_checks))
        action = np.array([(self.batch + self.step + e) % self.args.num_actions for e in range(self.args.env_batch_size)])
        self.step += 1
        return action, self.obs(), None, self.step == self.args.budget


@pytest.mark.parametrize("seed", [0, 3])
def test_train_sweeps_the_reference_s_batches(tmp_path, seed):
    args = engine_args(eval=False, seed=seed, budget=2, greedy_checks=4)
    n = 10
    random.seed(seed)
    chosen = sorted(random.sample(range(n), int(n * 0.4)))                      # reference :76-79
    engine = nn.Engine(args)
    engine.env, engine.checkpoint = StubEnv(args), str(tmp_path / "actions.npy")
    saves = []
    engine.save = lambda: saves.append((engine.spot, len(engine.actions)))
    engine.train([{"id": v} for v in range(n)])
    assert [entry[1] for entry in engine.env.log if entry[0] == "reset"] == chosen
    assert all(entry[3] == 4 for entry in engine.env.log if entry[0] == "best")
    assert engine.spot == chosen[-1] and len(engine.actions) == len(chosen) * 2 * 2
    # per step and element: the latent observed BEFORE the step beside the action chosen for that element
    want_a = [(v + s + e) % 6 for v in chosen for s in range(2) for e in range(2)]
    want_l = [100.0 * v + s + 0.25 * e for v in chosen for s in range(2) for e in range(2)]
    assert engine.actions == want_a and [float(l[0]) for l in engine.latents] == want_l
    assert all(l.shape == (4,) for l in engine.latents)
    assert saves == [(v, 4 * (chosen.index(v) + 1)) for v in chosen if v % 3 == 0]       # a save when v % 3 == 0 (:97-98)


def test_train_resumes_from_spot_and_sweeps_that_batch_again(tmp_path):
    args = engine_args(eval=False, seed=0, budget=2)
    n = 10
    random.seed(0)
    chosen = sorted(random.sample(range(n), 4))
    engine = nn.Engine(args)
    engine.env, engine.checkpoint = StubEnv(args), str(tmp_path / "actions.npy")
    engine.train([{"id": v} for v in range(n)])
    engine.save()
    resumed = nn.Engine(args)
    resumed.env, resumed.checkpoint, resumed.checkpoint_dir = StubEnv(args), engine.checkpoint, str(tmp_path)
    resumed.load()
    assert resumed.spot == chosen[-1] and resumed.actions == engine.actions
    resumed.spot = chosen[1]                                                     # as if the run had stopped after its second batch
    before = len(resumed.actions)
    resumed.train([{"id": v} for v in range(n)])
    assert [entry[1] for entry in resumed.env.log if entry[0] == "reset"] == chosen[1:]      # batch `spot` itself is swept again
    assert len(resumed.actions) == before + 4 * len(chosen[1:])
