"""``ops.latent_nearest`` (``a3vt_latent_nearest``, csrc/latent_nn.hip) on the GPU against ``nn_policy_util.contract``, a literal
fp64 restatement of the contract in ``include/a3vt.h``.

Inputs (``nn_policy_util.gapped_bank``): per query, rows ``q + r_j u_j`` with unit directions and radii ``0.05 * 1.02^j``, so
consecutive distances among a query's nearest differ by 4 %; far rows are added and the bank is shuffled.  Every test asserts on
its fp64 reference that the smallest relative gap among the ``k_eff + 1`` nearest exceeds 1e-3 BEFORE it compares anything: fp32
distances are within ``(dim + 4) * 2^-24`` relative of fp64 (one rounding for each subtraction, square and division, ``dim - 1``
for a sum of non-negative terms in any order), at most 2.5e-4 at dim 4096, so equal ``idx`` / ``action`` / ``rank`` follow.

Shapes: the smallest at which the kernel takes each of its paths — ``dim`` 1, 3, 5 (one scalar column group), 4, 200 (one
16-byte group), 257 and 260 (several groups, scalar and 16-byte), 1030 (the widest scalar form), 4096 (the limit); query counts
1, 3, 65 (65 x 200 floats need a second LDS chunk of queries); k 1, 25, 64; banks of 1, 7 (< k), T - 1, T, T + 1 and 3 T + 5 rows
(T = ``ops.LATENT_NN_TILE``) and on both sides of ``ops.LATENT_NN_CACHED_ROWS`` (registers / scratch selection)."""
import os

import numpy as np
import pytest
import torch

import env_util as eu
import nn_policy_util as nu

pytestmark = pytest.mark.gpu

from a3vt_amd import ops  # noqa: E402

T = ops.LATENT_NN_TILE


def run(cuda, bank, acts, queries, taken, k):
    dev = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(cuda)   # noqa: E731
    out = ops.latent_nearest(dev(bank, torch.float32), dev(acts, torch.int32), dev(queries, torch.float32), dev(taken, torch.float32), k)
    return [None if t is None else t.cpu().numpy() for t in out]


def check(cuda, bank, acts, queries, taken, k, what):
    """One call against the contract: the gap condition on the fp64 reference first, then equal idx / action / rank, dist within
    (dim + 4) * 2^-24 relative, -1 / +inf from k_eff on."""
    want = nu.contract(bank, acts, queries, taken, k)
    k_eff = min(k, len(bank))
    upto = min(k_eff + 1, len(bank))
    full = nu.contract(bank, None, queries, None, upto)[1] if upto > k_eff else want[1]
    gap = min(nu.smallest_gap(row, upto) for row in full)
    assert gap > 1e-3, f"{what}: the reference's own distances are only {gap:.2e} apart"
    got = run(cuda, bank, acts, queries, taken, k)
    assert got[0].dtype == np.int32 and got[0].shape == (len(queries), k) and got[1].shape == (len(queries), k)
    assert np.array_equal(got[0], want[0]), f"{what}: idx differs"
    tol = (bank.shape[1] + 4) * 2.0 ** -24
    w, g = want[1][:, :k_eff], got[1][:, :k_eff].astype(np.float64)
    fin = np.isfinite(w)
    assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isposinf(g), np.isposinf(w)), f"{what}: NaN / inf distances"
    err = float((np.abs(g[fin] - w[fin]) / w[fin]).max()) if fin.any() else 0.0
    print(f"{what}: gap {gap:.2e}, dist error {err:.2e} (bound {tol:.2e})")
    assert err <= tol, f"{what}: dist differs by {err:.2e} > {tol:.2e}"
    assert (got[0][:, k_eff:] == -1).all() and np.isposinf(got[1][:, k_eff:]).all()
    if acts is not None:
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), f"{what}: action / rank differ"
    return got, want


def inputs(bank_rows, dim, n_queries, k, seed, num_actions=30):
    bank, queries = nu.gapped_bank(bank_rows, dim, n_queries, k + 2, seed)
    g = np.random.default_rng(seed + 1)
    acts = g.integers(0, num_actions, bank_rows).astype(np.int32)
    taken = (g.random((n_queries, num_actions)) < 0.5).astype(np.float32)
    return bank, acts, queries, taken


def test_constants_are_the_library_s():
    from a3vt_amd import lib
    L = lib.load()
    assert (L.a3vt_latent_nn_tile(), L.a3vt_latent_nn_query_floats(), L.a3vt_latent_nn_cached_rows()) == \
        (ops.LATENT_NN_TILE, ops.LATENT_NN_QUERY_FLOATS, ops.LATENT_NN_CACHED_ROWS)


@pytest.mark.parametrize("dim", [1, 3, 4, 5, 200, 257, 260, 1030, 4096])
def test_dims(cuda, dim):
    check(cuda, *inputs(3 * T + 5, dim, 3, 25, 100 + dim), 25, f"dim {dim}")


@pytest.mark.parametrize("n_queries", [1, 3, 65])
def test_query_counts(cuda, n_queries):
    assert 65 * 200 > ops.LATENT_NN_QUERY_FLOATS >= 3 * 200              # 65 queries of 200 floats take a second chunk
    check(cuda, *inputs(n_queries * 27 + 2 * T + 3, 200, n_queries, 25, 200 + n_queries), 25, f"{n_queries} queries")


def test_query_chunks_at_the_widest_rows(cuda):
    """dim 4096: two queries per LDS chunk, so three queries take two chunks on the 16-column-group form."""
    assert ops.LATENT_NN_QUERY_FLOATS // 4096 == 2
    check(cuda, *inputs(T + 1, 4096, 3, 5, 77), 5, "dim 4096 in chunks")


@pytest.mark.parametrize("k", [1, 25, 64])
def test_k(cuda, k):
    check(cuda, *inputs(7 * T + 3, 5, 3, k, 300 + k), k, f"k {k}")


@pytest.mark.parametrize("dim", [5, 200])
@pytest.mark.parametrize("bank_rows", [1, 7, T - 1, T, T + 1, 3 * T + 5])
def test_bank_rows(cuda, bank_rows, dim):
    for k in (25, 64):
        check(cuda, *inputs(bank_rows, dim, 1, k, 400 + bank_rows), k, f"{bank_rows} rows, dim {dim}, k {k}")


@pytest.mark.parametrize("bank_rows", [1, 7])
def test_small_banks_with_two_queries(cuda, bank_rows):
    """Every row is listed for both queries; the seed is the first whose fp64 distances are gapped (``check`` asserts it)."""
    for seed in range(500, 540):
        args = inputs(bank_rows, 3, 2, 25, seed)
        if min(nu.smallest_gap(r, bank_rows) for r in nu.contract(args[0], None, args[2], None, bank_rows)[1]) > 1e-3:
            break
    check(cuda, *args, 25, f"{bank_rows} rows, two queries")


@pytest.mark.parametrize("bank_rows", [ops.LATENT_NN_CACHED_ROWS, ops.LATENT_NN_CACHED_ROWS + 1])
def test_register_and_scratch_selection(cuda, bank_rows):
    check(cuda, *inputs(bank_rows, 3, 2, 25, 600), 25, f"{bank_rows} rows")


def test_exact_ties_come_back_in_index_order(cuda):
    """30 bit-identical rows at scattered positions, nearer than everything else: ascending indices, one distance."""
    bank, acts, queries, taken = inputs(5 * T + 9, 200, 1, 64, 700)
    g = np.random.default_rng(701)
    where = np.sort(g.choice(len(bank), 30, replace=False))
    row = queries[0] + np.float32(0.001) * g.standard_normal(200).astype(np.float32)
    bank[where] = row
    got = run(cuda, bank, acts, queries, taken, 64)
    want = nu.contract(bank, acts, queries, taken, 64)
    assert np.array_equal(got[0][0, :30], where) and len(np.unique(got[1][0, :30].view(np.uint32))) == 1
    assert nu.smallest_gap(want[1][0, 29:], 35) > 1e-3
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])


def test_nan_and_inf_rows_rank_last(cuda):
    bank, acts, queries, taken = inputs(10, 5, 1, 25, 800)
    bank[3, 2], bank[6, 0] = np.nan, np.inf
    got, want = check(cuda, bank, acts, queries, None, 25, "nan / inf rows")
    assert list(got[0][0, 8:10]) == [6, 3] and np.isposinf(got[1][0, 8]) and np.isnan(got[1][0, 9])
    assert (got[0][0, 10:] == -1).all()
    # two NaN rows: the lower index first
    bank[1, 4] = np.nan
    got = run(cuda, bank, acts, queries, None, 25)
    assert list(got[0][0, 7:10]) == [6, 1, 3] and np.isnan(got[1][0, 8:10]).all()


def test_action_rule(cuda):
    """Masks that put ``rank`` at 0, in the middle, at k_eff - 1 and nowhere; no mask; an action outside the range."""
    k, A = 25, 30
    bank, _, queries, _ = inputs(4 * T + 1, 200, 5, k, 900)
    idx = nu.contract(bank, None, queries, None, k)[0]
    acts = np.full(len(bank), A - 1, dtype=np.int32)
    for e in range(5):
        acts[idx[e]] = np.arange(k)                               # the p-th nearest row of every query carries action p
    taken = np.zeros((5, A), dtype=np.float32)
    taken[1, :12], taken[2, :k - 1], taken[3, :] = 1, 1, 1
    taken[4, :3] = (0.5, -2.0, np.nan)                             # any non-zero value means taken
    got, _ = check(cuda, bank, acts, queries, taken, k, "action rule")
    assert list(got[3]) == [0, 12, k - 1, -1, 3] and list(got[2]) == [0, 12, k - 1, -1, 3]
    got, _ = check(cuda, bank, acts, queries, None, k, "no mask")
    assert list(got[3]) == [0] * 5
    acts[idx[0, 0]], acts[idx[1, 0]], acts[idx[1, 1]] = A, -1, 2 ** 31 - 1    # outside [0, A): skipped, never an index into taken
    got, _ = check(cuda, bank, acts, queries, np.zeros((5, A), dtype=np.float32), k, "actions out of range")
    assert list(got[3][:3]) == [1, 2, 0]
    pure = run(cuda, bank, None, queries, None, k)
    assert pure[2] is None and pure[3] is None and np.array_equal(pure[0], got[0])


def test_same_bits_every_call_alone_and_with_far_rows(cuda):
    bank, acts, queries, taken = inputs(6 * T + 7, 200, 3, 25, 1000)
    first = run(cuda, bank, acts, queries, taken, 25)
    again = run(cuda, bank, acts, queries, taken, 25)
    bits = lambda out: [a.view(np.uint32) if a.dtype == np.float32 else a for a in out]   # noqa: E731
    assert all(np.array_equal(a, b) for a, b in zip(bits(first), bits(again)))
    for e in range(3):
        alone = run(cuda, bank, acts, queries[e:e + 1], taken[e:e + 1], 25)
        assert all(np.array_equal(a[0], b[e]) for a, b in zip(bits(alone), bits(first))), f"query {e} alone"
    far = np.random.default_rng(1001).standard_normal((2 * T + 3, 200)).astype(np.float32) + 9.0
    more = run(cuda, np.concatenate([bank, far]), np.concatenate([acts, acts[:len(far)]]), queries, taken, 25)
    assert all(np.array_equal(a, b) for a, b in zip(bits(more), bits(first)))
    # the same rows in another order and another tile: the same distances, bit for bit
    perm = np.random.default_rng(1002).permutation(len(bank))
    moved = run(cuda, bank[perm], acts[perm], queries, taken, 25)
    assert np.array_equal(perm[moved[0]], first[0]) and np.array_equal(moved[1].view(np.uint32), first[1].view(np.uint32))


def test_disagreeing_operands_are_refused_before_any_launch(cuda):
    bank, acts, queries, taken = (torch.from_numpy(a).to(cuda) for a in inputs(40, 8, 2, 5, 1100))
    for bad in ((bank, acts, queries[:, :7], taken, 5), (bank, acts[:-1], queries, taken, 5), (bank, acts, queries, taken[:1], 5),
                (bank, acts.long(), queries, taken, 5), (bank.double(), acts, queries, taken, 5), (bank, acts, queries, taken, 65),
                (bank, acts, queries, taken, 0), (bank, acts, queries.cpu(), taken, 5), (bank, None, queries, taken, 5)):
        with pytest.raises(RuntimeError, match="a3vt: "):
            ops.latent_nearest(*bad)


# ---- the g19 replay: this package's Engine against the reference's, knob on and off ------------------------------------------------
# Bounds: equal actions and spot; latents and scores within 1e-4 relative (``helpers.rel_err``), the bounds of
# ``test_gpu_active_touch.py`` against g18.  The generator asserts that at every lookup of the fixture consecutive fp64 distances
# among the 26 nearest are more than 1e-2 apart, so equal actions follow from the latent bound.

@pytest.fixture(scope="module")
def golden():
    from golden_util import load
    return load(nu.FIXTURE)


@pytest.fixture(autouse=True)
def restore_process_flags():
    yield from eu.kept_process_flags()


@pytest.fixture(scope="module")
def locations(cuda, golden, tmp_path_factory):
    """The checkpoint directories of this package's models built by the fixture's recipe (checksums asserted)."""
    return eu.package_models(nu.CASE, golden, tmp_path_factory.mktemp("g19"))


def make_engine(golden, locations, monkeypatch, tmp_path, evaluate, fused):
    from a3vt_amd.pterotactyl.policies import environment, recorded
    from a3vt_amd.pterotactyl.policies.NearestNeighbor import train as nn
    monkeypatch.setattr(environment.ActiveTouch, "get_loaders", lambda self: None)
    monkeypatch.chdir(tmp_path)                                   # results/ and experiments/checkpoint/ are made in the working directory
    args = nu.engine_args(evaluate, fused_lookup=fused, **locations)
    engine = nn.Engine(args, sampler=recorded.RecordedSampler(nu.records()), loaders=(nu.batches("train"), nu.batches("valid")))
    inner = environment.ActiveTouch.__init__

    def with_samples(self, *a, **k):
        inner(self, *a, **k)
        self.score_samples = eu.score_samples(golden)

    monkeypatch.setattr(environment.ActiveTouch, "__init__", with_samples)
    return engine, nn


def test_train_builds_the_reference_s_bank(cuda, golden, locations, monkeypatch, tmp_path):
    from helpers import rel_err
    engine, nn = make_engine(golden, locations, monkeypatch, tmp_path, False, None)
    engine()
    assert os.path.exists(engine.checkpoint) and engine.checkpoint.endswith(os.path.join("g19", "actions.npy"))
    assert os.path.isdir(engine.results_dir)
    saved = nn.LatentBank(6).load(engine.checkpoint)
    for bank in (engine.bank, saved):
        assert bank.spot == int(golden["train:spot"]) and bank.actions == list(golden["train:actions"])
        e = rel_err(torch.stack(bank.latents), torch.from_numpy(golden["train:latents"]))
        assert e < 1e-4, f"bank latents differ by {e:.2e} (relative)"
    print(f"train: spot {engine.spot}, actions {engine.actions}, latents within {e:.2e}")


def run_validate(golden, locations, monkeypatch, tmp_path, fused):
    engine, nn = make_engine(golden, locations, monkeypatch, tmp_path, True, fused)
    ckpt = tmp_path / "experiments" / "checkpoint" / "g19"
    ckpt.mkdir(parents=True)
    np.save(str(ckpt / "actions.npy"), {"actions": golden["bank:actions"], "latents": golden["bank:latents"], "spot": 0})
    return engine, nn


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "loop"])
def test_validate_replays_the_reference(cuda, golden, locations, monkeypatch, tmp_path, fused):
    from helpers import rel_err
    engine, nn = run_validate(golden, locations, monkeypatch, tmp_path, fused)
    seen = []
    from a3vt_amd.pterotactyl.policies import environment
    reset, step = environment.ActiveTouch.reset, environment.ActiveTouch.step
    monkeypatch.setattr(environment.ActiveTouch, "reset", lambda self, batch: seen.append([reset(self, batch)]) or seen[-1][0])
    monkeypatch.setattr(environment.ActiveTouch, "step", lambda self, a: (lambda r: seen[-1].append(r[0]) or r)(step(self, a)))
    total = engine()
    assert len(engine.actions) == nu.BANK_ROWS and len(seen) == nu.VALID_BATCHES
    worst = {"score": 0.0, "latent": 0.0}
    for b, episode in enumerate(seen):
        assert len(episode) == 4                                                    # reset + budget steps
        for i, obs in enumerate(episode):
            key = f"valid:{b}:{i}:"
            if i:
                got = engine.chosen[2 * b:2 * b + 2, i - 1].numpy().astype(np.int64)
                assert np.array_equal(got, golden[key + "actions"]), (b, i, got, golden[key + "actions"])
            assert torch.equal(obs["mask"], torch.from_numpy(golden[key + "mask"]))
            for what in worst:
                e = rel_err(obs[what], torch.from_numpy(golden[key + what]))
                worst[what] = max(worst[what], e)
                assert e < 1e-4, f"batch {b} call {i}: {what} differs by {e:.2e} (relative)"
    want = np.stack([[golden[f"valid:{b}:{i}:score"] for i in range(4)] for b in range(nu.VALID_BATCHES)])      # (batch, call, E)
    want = torch.from_numpy(want).permute(0, 2, 1).reshape(-1, 4)
    assert rel_err(engine.scores, want) < 1e-4
    assert abs(float(total["score"]) - float((want[:, -1] / want[:, 0]).mean())) < 1e-4
    print(f"validate {'fused' if fused else 'loop'}: worst relative errors {worst}, total {total}")


def test_one_host_tensor_of_E_integers_leaves_a_lookup(cuda, golden, locations, monkeypatch, tmp_path):
    """With the knob on, every step's ``LatentBank.lookup`` copies exactly one tensor to the host — E integers — and nothing else
    synchronises inside it: ``Tensor.cpu`` / ``numpy`` / ``item`` / ``tolist`` on device tensors are counted while it runs."""
    engine, nn = run_validate(golden, locations, monkeypatch, tmp_path, True)
    copies, lookups = [], []
    inner = nn.LatentBank.lookup
    originals = {name: getattr(torch.Tensor, name) for name in ("cpu", "item", "tolist", "numpy", "__bool__", "__int__", "__float__")}

    def counted(name):
        def method(self, *a, **k):
            if self.is_cuda:
                copies[-1].append((name, tuple(self.shape), self.dtype))
            return originals[name](self, *a, **k)
        return method

    def watched(self, latents, mask, k, device=None):
        self.to(utils_device())                                                    # (the bank's one upload is not a step's traffic)
        copies.append([])
        for name in originals:
            setattr(torch.Tensor, name, counted(name))
        try:
            out = inner(self, latents, mask, k, device=device)
        finally:
            for name, fn in originals.items():
                setattr(torch.Tensor, name, fn)
        lookups.append(out)
        return out

    from a3vt_amd.pterotactyl.utility.utils import _device as utils_device
    monkeypatch.setattr(nn.LatentBank, "lookup", watched)
    engine()
    assert len(lookups) == nu.VALID_BATCHES * 3 and all(isinstance(o, np.ndarray) and o.shape == (2,) for o in lookups)
    for c in copies:
        assert c == [("cpu", (2,), torch.int32)], c
