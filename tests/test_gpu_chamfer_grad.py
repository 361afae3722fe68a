"""-m gpu: what follows the Chamfer search — chamfer_bwd_kernel and chamfer_reduce_kernel (csrc/chamfer.hip) — element by
element against tests/chamfer_grad_ref.py (float64 and integers; tested on the CPU by test_chamfer_grad_ref_host.py), and the
searches on ties between DISTINCT points.  The gradient kernel is called directly (a3vt_chamfer_bwd), so the index tables are the
test's own: hubs, permutations, targets on both sides of every tile boundary; every index is in range (the header promises
nothing otherwise).  The gradients are the middle of larger buffers: every element must be written, nothing outside may change,
and grad_y == NULL must leave grad_x's bits alone.

Exact cases (==): coordinates on the 2^-8 grid in [-1, 1), P, Q, draws and gcd powers of two (one gcd 0): every difference, every
fixed-point term (shift >= 44), every integer sum, ct, cs, both products and their sum are exact, fused or not, so the kernel
has to return the reference's value bit for bit (a zero of either sign where gcd is 0).  Quantised case (==): general floats with
one coordinate at 2^40, P = Q = 8192, draws 1, gcd a power of two: the shift is 7, every term is visibly rounded to 1/128, and
the result is still unique (ct, cs powers of two: one rounding, in the final sum) — it pins the shift itself (46 or 47 in the clean cloud).
Bounded cases: |v - v64| <= u [(nsrc + 8)|ct| A + 9 |cs| Bm] + |cs| n 2^-shift + 2^-149 per element (chamfer_grad_ref's docstring
counts the constants); an element nothing lands on, with a zero direct term, must be exactly 0.
Reduction: cd against the float64 mean of the RETURNED distances, relative error <= K_R u with K_R = ceil(p/1024) + ceil(q/1024) +
draws + 26 (all terms are non-negative); bit for bit where every partial sum is exact.

What these checks see of chamfer.hip, mutation by mutation (reasoned, not run):
  `i < i0` -> `i <= i0`     the first target of every tile loses its scattered terms: the hubs on 0 and on the first index of the
                            second tile lose everything, the tile-edge tables half their terms, every random table what lands
                            on 0; in the bounded cases a lost term is at least 1/8 of Bm against a bound of 9 u Bm.
  `cs` built from nt        the scattered part is off by nt / ns wherever P != Q: three exact cases, every bounded case.
  `idx_stride` 0 for grad_y every draw reads draw 0's tables: every case with more than one draw (exact: draws 2 and 4; bounded: 3).
  `c` one smaller           the exact grid cases do NOT see it (62 leaves a spare bit: the sums stay below 2^63, and a finer
                            quantum is still exact); test_exact_at_a_coarse_quantum does: at shift 8 instead of 7 the terms round
                            differently, and the result is compared with the emulation bit for bit.
  `i >= i1` -> `i > i1`     NOT visible in any output: the extra term (a source whose neighbour is the next tile's first target)
                            is added one accumulator past the tile, which no thread reads back — the next tile's own workgroup
                            still counts the term once.  It is an LDS write past the dynamic allocation, or into its padding;
                            only a check of the code itself could see it, and none is made here.

Measured on an MI355X (profiles/chamfer_grad.txt has every case): the whole file, 63 tests, runs in 4.4 s.  Worst err / bound of
the bounded cases over the sizes 1023 ... 12289, either cloud cut: unit scale 0.40, scale 1e-15 0.36, scale 1e4 0.29, offset 0.34,
one coordinate at 1e6 0.45 (the numpy emulation: 0.50).  Reduction: 0.08 of K_R u over 108 calls.  Every exact case: 0 differing
elements, hubs of up to 32 768 terms.  The searches give a point with a NaN coordinate the distance 3e38, not NaN, so through the
public entry points the reduction never sees a NaN: the poisoned cloud's cd is large and finite (1.5e35 here), and that is what
test_reduce_keeps_a_poisoned_cloud_to_itself pins, with the bits of the other clouds.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import chamfer_grad_ref as cg
from oracle import chamfer as och

pytestmark = pytest.mark.gpu

U = cg.U
SENTINEL = 0x5A5A5A5A              # around the gradients
UNWRITTEN = 0x7FC0BEEF             # in them: a NaN no kernel produces
PAD = 256                          # elements on either side
ALGOS = ("two_pass", "sweep", "pruned")


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------

def _framed(cuda, n):
    buf = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.int32, device=cuda)
    buf[PAD:PAD + n] = UNWRITTEN
    return buf


def _unframe(buf, shape, what):
    h = buf.cpu().numpy()
    assert (h[:PAD] == SENTINEL).all() and (h[-PAD:] == SENTINEL).all(), f"{what}: written outside the gradient"
    mid = h[PAD:-PAD]
    assert not (mid == UNWRITTEN).any(), f"{what}: {int((mid == UNWRITTEN).sum())} of {mid.size} elements never written"
    return mid.view(np.float32).reshape(shape).copy()


def bwd(cuda, x, y, ixy, iyx, gcd, with_gy=True):
    """a3vt_chamfer_bwd on numpy inputs -> (gx, gy or None) as numpy float32, with the frame checks."""
    from a3vt_amd import lib
    L = lib.load()
    R, B, P, _ = x.shape
    Q = y.shape[1]
    assert ixy.shape == (R, B, P) and iyx.shape == (R, B, Q) and ixy.min() >= 0 and ixy.max() < Q and iyx.min() >= 0 and iyx.max() < P
    dev = [torch.from_numpy(np.ascontiguousarray(a, dtype=t)).to(cuda)
           for a, t in ((x, np.float32), (y, np.float32), (ixy, np.int32), (iyx, np.int32), (gcd, np.float32))]
    bx, by = _framed(cuda, x.size), _framed(cuda, y.size) if with_gy else None
    inner = lambda b: ctypes.c_void_p(b.data_ptr() + 4 * PAD)   # noqa: E731
    lib.check(L.a3vt_chamfer_bwd(*[lib.ptr(d) for d in dev[:2]], R, B, P, Q, *[lib.ptr(d) for d in dev[2:]], inner(bx),
                                 inner(by) if with_gy else None, None), "chamfer_bwd")
    torch.cuda.synchronize()
    return _unframe(bx, x.shape, "grad_x"), _unframe(by, y.shape, "grad_y") if with_gy else None


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.int32), np.asarray(b, dtype=np.float32).view(np.int32))


def assert_exact(dev, ref, what):
    """dev == ref for every element (a zero of either sign for a zero; ref holds no NaN, so a NaN fails)."""
    assert cg.is_fp32(ref), f"{what}: a broken case, its expected values are not fp32 numbers"
    bad = dev.astype(np.float64) != ref
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ; first at {i}: device {dev[i]!r} reference {ref[i]!r}")


def ratio(dev, ref, bound, what):
    """Asserts |dev - ref| <= bound for EVERY element and returns the largest err / bound."""
    err = np.abs(dev.astype(np.float64) - ref)
    ok = err <= bound                                           # a NaN is not ok
    worst = float(np.nanmax(err[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0
    if not ok.all():
        i = tuple(np.argwhere(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} elements out of bound; worst err/bound {worst:.3g}; first at "
                             f"{i}: device {dev[i]!r} reference {ref[i]!r} bound {bound[i]!r}")
    return worst


# ---- 3a: exact --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("number", range(len(cg.EXACT_CASES)), ids=[f"{c[0]}x{c[1]}-draws{c[2]}-B{c[3]}" for c in cg.EXACT_CASES])
def test_exact_on_the_grid(cuda, number):
    x, y, gcd, tables = cg.exact_case(number)
    hub = 0
    for name, (ixy, iyx) in tables.items():
        ref = cg.grad(x, y, ixy, iyx, gcd)
        hub = max(hub, int(ref.nx.max()), int(ref.ny.max()))
        gx, gy = bwd(cuda, x, y, ixy, iyx, gcd)
        assert_exact(gx, ref.gx, f"{name} grad_x")
        assert_exact(gy, ref.gy, f"{name} grad_y")
        assert same_bits(bwd(cuda, x, y, ixy, iyx, gcd, with_gy=False)[0], gx), f"{name}: grad_x depends on grad_y == NULL"
    print(f"CHAMFER_GRAD exact (P, Q, draws, B) = {cg.EXACT_CASES[number]}: {len(tables)} table pairs, 0 elements differ, hubs of up to {hub} terms")


@functools.lru_cache(maxsize=None)
def quantised_case():
    """General floats in (-1, 1), x[0, 0, 5000, 2] = 2^40 (so 2^e = 2^41 > max|T| + max|S| and 2^14 > 8192: shift 7); cloud 1 is
    left at unit scale.  P = Q = 8192: two tiles.  gcd (2, -1/4)."""
    rng = np.random.default_rng(77)
    x = rng.uniform(-1, 1, (1, 2, 8192, 3)).astype(np.float32)
    y = rng.uniform(-1, 1, (2, 8192, 3)).astype(np.float32)
    x[0, 0, 5000, 2] = 2.0 ** 40
    gcd = np.array([2.0, -0.25], dtype=np.float32)
    tables = cg.scatter_tables(rng, (1, 2, 8192), 8192)
    return x, y, gcd, {k: tables[k] for k in ("random", "permutation", "tile-edges")}


def test_exact_at_a_coarse_quantum(cuda):
    x, y, gcd, tables = quantised_case()
    sx, sy = cg.scales(x, y, gcd)
    assert sx.shift[0, 0] == 7 and sy.shift[0] == 7 and sx.shift[0, 1] >= 44 and sy.shift[1] >= 44
    for s in (sx, sy):                                          # products by powers of two are exact: fused or not, one rounding
        assert (np.frexp(np.abs(s.ct))[0] == 0.5).all() and (np.frexp(np.abs(s.cs))[0] == 0.5).all()
    for name, t in tables.items():
        other = cg.random_table(np.random.default_rng(len(name)), t.shape, 8192)
        for ixy, iyx in ((other, t), (t, other)):
            ex, ey = cg.emulate(x, y, ixy, iyx, gcd)
            ref = cg.grad(x, y, ixy, iyx, gcd)
            moved = np.abs(ex[0, 0].astype(np.float64) - ref.gx[0, 0]) > abs(sx.cs[0, 0]) * 2.0 ** -10     # an eighth of a quantum
            assert name == "tile-edges" or moved.mean() > 0.2, "the quantum is meant to show"
            gx, gy = bwd(cuda, x, y, ixy, iyx, gcd)
            assert same_bits(gx, ex) and same_bits(gy, ey), \
                f"{name}: {int((gx != ex).sum())} grad_x, {int((gy != ey).sum())} grad_y elements differ from the emulation at shift 7"


# ---- 3b: bounded ---------------------------------------------------------------------------------------------------------------------

def search64(cuda, x, y):
    """The float64 brute force on fp32 clouds (oracle.chamfer.nn_sqdist on the device: plumbing) -> ixy (R,B,P), iyx (R,B,Q)."""
    xd, yd = torch.from_numpy(x).to(cuda).double(), torch.from_numpy(y).to(cuda).double()
    R, B = x.shape[:2]
    ixy = torch.stack([torch.stack([och.nn_sqdist(xd[r, b], yd[b])[1] for b in range(B)]) for r in range(R)])
    iyx = torch.stack([torch.stack([och.nn_sqdist(yd[b], xd[r, b])[1] for b in range(B)]) for r in range(R)])
    return ixy.cpu().numpy(), iyx.cpu().numpy()


@functools.lru_cache(maxsize=None)
def bounded_case(cuda, nt, as_p):
    P, Q = (nt, cg.BOUNDED_OTHER) if as_p else (cg.BOUNDED_OTHER, nt)
    x, y = cg.bounded_clouds(nt * 2 + as_p, P, Q)
    gcd = np.array(cg.BOUNDED_GCD)
    ixy, iyx = search64(cuda, x, y)
    ref = cg.grad(x, y, ixy, iyx, gcd)
    return x, y, gcd, ixy, iyx, ref, cg.bounds(ref, x, y, gcd)


@pytest.mark.parametrize("as_p", [True, False], ids=["P", "Q"])
@pytest.mark.parametrize("nt", cg.BOUNDED_NT)
def test_bounded_per_element(cuda, nt, as_p):
    x, y, gcd, ixy, iyx, ref, (bx, by) = bounded_case(cuda, nt, as_p)
    n_cut = ref.nx if as_p else ref.ny                          # the terms per target of the cloud that is cut into tiles
    assert nt <= cg.BWD_TILE or n_cut.max() <= 8, "at a tile edge a lost or doubled term has to be at least 1/8 of Bm"
    gx, gy = bwd(cuda, x, y, ixy, iyx, gcd)
    worst = []
    for b, name in enumerate(cg.BOUNDED_CLOUDS):
        worst.append(max(ratio(gx[:, b], ref.gx[:, b], bx[:, b], f"{name}: grad_x"), ratio(gy[b], ref.gy[b], by[b], f"{name}: grad_y")))
    print(f"CHAMFER_GRAD err/bound {'P' if as_p else 'Q'} = {nt}: " + "  ".join(f"{n} {w:.3f}" for n, w in zip(cg.BOUNDED_CLOUDS, worst)))
    assert same_bits(bwd(cuda, x, y, ixy, iyx, gcd, with_gy=False)[0], gx)


def test_nothing_lands_means_zero(cuda):
    """y[b, j] = x[r, b, i] with i = ixy's choice and nobody choosing i: direct term 0, n = 0, bound 0 — the element is 0."""
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (3, 2, 1025, 3)).astype(np.float32)
    y = rng.uniform(-1, 1, (2, 777, 3)).astype(np.float32)
    ixy, iyx = cg.random_table(rng, (3, 2, 1025), 777), cg.random_table(rng, (3, 2, 777), 1025)
    free = np.setdiff1d(np.arange(1025), iyx[1, 0])[:5]         # points of x[1, 0] no term lands on
    x[1, 0, free] = y[0, ixy[1, 0, free]]
    gcd = np.array([3.0, -1.0])
    ref = cg.grad(x, y, ixy, iyx, gcd)
    bx, by = cg.bounds(ref, x, y, gcd)
    assert (bx[1, 0, free] == 0).all() and (bx == 0).sum() == 15
    gx, gy = bwd(cuda, x, y, ixy, iyx, gcd)
    assert (gx[1, 0, free] == 0).all()
    ratio(gx, ref.gx, bx, "grad_x"), ratio(gy, ref.gy, by, "grad_y")


# ---- 3c: determinism ------------------------------------------------------------------------------------------------------------------

def test_four_runs_are_identical(cuda):
    """LDS atomics arrive in any order; the integer sums may not depend on it: hubs of 32 768 and 8192 terms on one accumulator and a
    random float case, four times each."""
    x, y, gcd, tables = cg.exact_case(3)
    runs = [(x, y, *tables["y:hub4096"], gcd), (x, y, *tables["x:hub4095"], gcd)]
    x, y, gcd, ixy, iyx, _, _ = bounded_case(cuda, 6145, True)
    runs.append((x, y, ixy, iyx, gcd))
    for a in runs:
        first = bwd(cuda, *a)
        for _ in range(3):
            again = bwd(cuda, *a)
            assert same_bits(again[0], first[0]) and same_bits(again[1], first[1])


# ---- 3d: non-finite coordinates -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def nonfinite_case(cuda):
    """draws 2, B 3, P = 6145 (two tiles: the poisoned point is in the second, the first has to answer too), Q = 300."""
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, (2, 3, 6145, 3)).astype(np.float32)
    y = rng.uniform(-1, 1, (3, 300, 3)).astype(np.float32)
    ixy, iyx = cg.random_table(rng, (2, 3, 6145), 300), cg.random_table(rng, (2, 3, 300), 6145)
    gcd = np.array([1.0, -2.0, 0.5])
    return x, y, ixy, iyx, gcd, bwd(cuda, x, y, ixy, iyx, gcd)


@pytest.mark.parametrize("where", ["x", "y"])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf")], ids=["nan", "inf", "-inf"])
def test_nonfinite_coordinate_poisons_its_clouds_only(cuda, value, where):
    """The kernel's contract: a NaN or an Inf coordinate, alone, makes the gradient of every cloud it enters NaN throughout,
    and leaves every other cloud's bits alone."""
    x, y, ixy, iyx, gcd, (cx, cy) = nonfinite_case(cuda)
    assert np.isfinite(cx).all() and np.isfinite(cy).all()
    x, y = x.copy(), y.copy()
    if where == "x":
        x[1, 1, 6000, 2] = value                                # enters grad_x[1, 1] (target) and grad_y[1] (source)
        nan_x = np.zeros((2, 3), dtype=bool)
        nan_x[1, 1] = True
    else:
        y[1, 299, 0] = value                                    # enters grad_x[:, 1] (source) and grad_y[1] (target)
        nan_x = np.zeros((2, 3), dtype=bool)
        nan_x[:, 1] = True
    gx, gy = bwd(cuda, x, y, ixy, iyx, gcd)
    for r in range(2):
        for b in range(3):
            if nan_x[r, b]:
                assert np.isnan(gx[r, b]).all(), f"grad_x[{r},{b}]: {int((~np.isnan(gx[r, b])).sum())} of {gx[r, b].size} elements are not NaN"
            else:
                assert same_bits(gx[r, b], cx[r, b]), f"grad_x[{r},{b}] changed"
    assert np.isnan(gy[1]).all(), f"grad_y[1]: {int((~np.isnan(gy[1])).sum())} of {gy[1].size} elements are not NaN"
    assert same_bits(gy[0], cy[0]) and same_bits(gy[2], cy[2])
    assert same_bits(bwd(cuda, x, y, ixy, iyx, gcd, with_gy=False)[0], gx)


# ---- 3e: reduction ---------------------------------------------------------------------------------------------------------------------

REDUCE_SIZES = (1, 63, 1023, 1024, 1025, 2049)


def check_cd(cd, dxy, dyx, what):
    """cd (B,) against the float64 mean of the returned distances: NaN where one is NaN, else within K_R u relative."""
    draws, B, p = dxy.shape
    k = cg.k_reduce(p, dyx.shape[2], draws)
    ref = cg.reduce(dxy, dyx)
    worst = 0.0
    for b in range(B):
        if np.isnan(ref[b]):
            assert np.isnan(cd[b]), f"{what}: cd[{b}] = {cd[b]!r} from distances that hold a NaN"
            continue
        err = abs(float(cd[b]) - ref[b])
        assert err <= k * U * ref[b], f"{what}: cd[{b}] = {cd[b]!r}, float64 {ref[b]!r}: {err / (U * ref[b]):.2f} u > K_R = {k}"
        worst = max(worst, err / (k * U * ref[b]) if ref[b] > 0 else 0.0)
    return worst


def test_reduce_against_its_own_distances(cuda):
    from a3vt_amd import ops
    rng = np.random.default_rng(21)
    worst, count = 0.0, 0
    for ip, p in enumerate(REDUCE_SIZES):
        for iq, q in enumerate(REDUCE_SIZES):
            draws = 1 + (ip + iq) % 3
            x = torch.from_numpy(rng.uniform(-1, 1, (draws, 2, p, 3)).astype(np.float32)).to(cuda)
            y = torch.from_numpy(rng.uniform(-1, 1, (2, q, 3)).astype(np.float32)).to(cuda)
            for algo in ALGOS:
                dxy, _, dyx, _, cd = ops.chamfer_nn(x, y, algo=algo)
                worst = max(worst, check_cd(cd.cpu().numpy(), dxy.cpu().numpy(), dyx.cpu().numpy(), f"{algo} p={p} q={q} draws={draws}"))
                count += 1
    print(f"CHAMFER_GRAD reduce err/(K_R u cd), {count} calls: {worst:.3f}")


@pytest.mark.parametrize("draws", [1, 2, 3])
def test_reduce_every_draws_at_the_thread_count(cuda, draws):
    from a3vt_amd import ops
    rng = np.random.default_rng(22 + draws)
    for p, q in ((1024, 1025), (1025, 1023), (2049, 1)):
        x = torch.from_numpy(rng.uniform(-1, 1, (draws, 3, p, 3)).astype(np.float32)).to(cuda)
        y = torch.from_numpy(rng.uniform(-1, 1, (3, q, 3)).astype(np.float32)).to(cuda)
        for algo in ALGOS:
            dxy, _, dyx, _, cd = ops.chamfer_nn(x, y, algo=algo)
            check_cd(cd.cpu().numpy(), dxy.cpu().numpy(), dyx.cpu().numpy(), f"{algo} p={p} q={q} draws={draws}")


@pytest.mark.parametrize("p,q,draws", [(1, 1, 1), (1024, 2048, 2), (2048, 64, 4), (4096, 4096, 1)])
def test_reduce_exact_on_the_grid(cuda, p, q, draws):
    """Grid clouds at 2^-4: every distance is an integer of 2^-8, and with p, q, draws powers of two every quotient and partial
    sum is an integer of 2^-8 / max(p, q) below 2^24: cd equals the integer reference bit for bit."""
    from a3vt_amd import ops
    rng = np.random.default_rng(p + q)
    x = np.stack([np.stack([cg.grid_cloud(rng, p, 4) for _ in range(2)]) for _ in range(draws)])
    y = np.stack([cg.grid_cloud(rng, q, 4) for _ in range(2)])
    m = max(p, q)
    total = np.zeros(2, dtype=np.int64)
    for b in range(2):
        for r in range(draws):
            total[b] += cg.nn_first(x[r, b], y[b])[0].sum() * (m // p) + cg.nn_first(y[b], x[r, b])[0].sum() * (m // q)
    assert total.max() < 2 ** 24, "a broken case: a partial sum would be rounded"
    ref = total.astype(np.float64) / (256.0 * m * draws)
    xd, yd = torch.from_numpy(x.astype(np.float32)).to(cuda), torch.from_numpy(y.astype(np.float32)).to(cuda)
    for algo in ALGOS:
        cd = ops.chamfer_nn(xd, yd, algo=algo)[4].cpu().numpy()
        assert (cd.astype(np.float64) == ref).all(), f"{algo}: cd {cd!r}, integer reference {ref!r}"


def test_reduce_keeps_a_poisoned_cloud_to_itself(cuda):
    """A NaN coordinate in x[0, 1]: cd[1] follows from the distances the search returned (NaN if one of them is NaN; the searches
    return 3e38 for such a point, and one such term does not overflow the sums), cd[0] and cd[2] keep the clean run's bits."""
    from a3vt_amd import ops
    rng = np.random.default_rng(23)
    x = rng.uniform(-1, 1, (2, 3, 1000, 3)).astype(np.float32)
    y = torch.from_numpy(rng.uniform(-1, 1, (3, 900, 3)).astype(np.float32)).to(cuda)
    for algo in ALGOS:
        clean = ops.chamfer_nn(torch.from_numpy(x).to(cuda), y, algo=algo)[4].cpu().numpy()
        bad = x.copy()
        bad[0, 1, 17, 1] = float("nan")
        dxy, _, dyx, _, cd = [t.cpu().numpy() for t in ops.chamfer_nn(torch.from_numpy(bad).to(cuda), y, algo=algo)]
        print(f"CHAMFER_GRAD {algo}: distance of a NaN point {dxy[0, 1, 17]!r}, cd {cd!r}")
        assert same_bits(cd[[0, 2]], clean[[0, 2]])
        check_cd(cd[1:2], dxy[:, 1:2], dyx[:, 1:2], f"{algo}: poisoned cloud")


# ---- 3f: ties between distinct points ---------------------------------------------------------------------------------------------------

TIE_SIZES = (1, 63, 64, 65, 1000, 2048, 2049, 2176)
TIE_PAIRS = sorted({(TIE_SIZES[i], TIE_SIZES[j]) for i in range(8) for j in (i, 7 - i, (i + 3) % 8)})


@functools.lru_cache(maxsize=None)
def tie_clouds():
    """Two draws of x and one y per size on the 2^-4 grid (32^3 sites: from 1000 points on, equal distances are the rule)."""
    rng = np.random.default_rng(31)
    return ({n: np.stack([cg.grid_cloud(rng, n, 4) for _ in range(2)]) for n in TIE_SIZES},
            {n: cg.grid_cloud(rng, n, 4) for n in TIE_SIZES})


@pytest.mark.parametrize("P,Q", TIE_PAIRS)
def test_ties_between_distinct_points_go_to_the_first(cuda, P, Q):
    from a3vt_amd import ops
    xs, ys = tie_clouds()
    x, y = xs[P], ys[Q]
    want = [cg.nn_first(x[r], y) for r in range(2)], [cg.nn_first(y, x[r]) for r in range(2)]
    xd = torch.from_numpy(x[:, None].astype(np.float32)).to(cuda)
    yd = torch.from_numpy(y[None].astype(np.float32)).to(cuda)
    for algo in ALGOS:
        dxy, ixy, dyx, iyx, _ = [t.cpu().numpy() for t in ops.chamfer_nn(xd, yd, algo=algo)]
        for r in range(2):
            for got_d, got_i, (d, i), name in ((dxy[r, 0], ixy[r, 0], want[0][r], "xy"), (dyx[r, 0], iyx[r, 0], want[1][r], "yx")):
                assert np.array_equal(got_d.astype(np.float64) * 256, d), f"{algo} dist_{name}[{r}]"
                assert np.array_equal(got_i, i), f"{algo} idx_{name}[{r}]: {int((got_i != i).sum())} of {i.size} are not the first minimum"


def test_forward_and_backward_on_ties_end_to_end(cuda):
    """ops.ChamferFn on grid clouds, gradients on both clouds, weights powers of two: the search, the saved tables and the
    gradient kernel together return grad on nn_first's indices bit for bit."""
    from a3vt_amd import ops
    xs, ys = tie_clouds()
    rng = np.random.default_rng(32)
    x = np.stack([xs[2048], np.stack([cg.grid_cloud(rng, 2048, 4) for _ in range(2)])], axis=1)      # (2, 2, 2048, 3)
    y = np.stack([ys[64], cg.grid_cloud(rng, 64, 4)])                                                # (2, 64, 3)
    gcd = np.array([4.0, -0.5])
    ixy = np.array([[cg.nn_first(x[r, b], y[b])[1] for b in range(2)] for r in range(2)])
    iyx = np.array([[cg.nn_first(y[b], x[r, b])[1] for b in range(2)] for r in range(2)])
    ref = cg.grad(x, y, ixy, iyx, gcd)
    before = ops.CHAMFER_ALGO
    try:
        for algo in ALGOS:
            ops.CHAMFER_ALGO = ops.NN_ALGOS[algo]
            xd = torch.from_numpy(x.astype(np.float32)).to(cuda).requires_grad_(True)
            yd = torch.from_numpy(y.astype(np.float32)).to(cuda).requires_grad_(True)
            ops.ChamferFn.apply(xd, yd).backward(torch.from_numpy(gcd.astype(np.float32)).to(cuda))
            assert_exact(xd.grad.cpu().numpy(), ref.gx, f"{algo} grad_x")
            assert_exact(yd.grad.cpu().numpy(), ref.gy, f"{algo} grad_y")
    finally:
        ops.CHAMFER_ALGO = before
