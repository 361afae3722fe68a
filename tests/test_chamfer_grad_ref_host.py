"""The references of tests/chamfer_grad_ref.py, tested on the CPU: the float64 gradient against torch autograd and against the
oracle's closed form, the per-element bound against a numpy float32 emulation of the kernel's arithmetic (it has to hold for
the reference arithmetic with room to spare: it is a derived condition, not a figure fitted to the kernel), the precondition of
the cases the GPU test compares bit for bit, and the small builders."""
import numpy as np
import pytest
import torch

import chamfer_grad_ref as cg
from oracle import chamfer as och


def _random_case(seed, R, B, P, Q):
    rng = np.random.default_rng(seed)
    x, y = rng.normal(size=(R, B, P, 3)), rng.normal(size=(B, Q, 3))
    return x, y, rng.normal(size=B)


def _tables(x, y):
    R, B = x.shape[:2]
    nn = [[cg.nn_float64(x[r, b], y[b]) for b in range(B)] for r in range(R)]
    return (np.array([[nn[r][b][0] for b in range(B)] for r in range(R)]),
            np.array([[nn[r][b][1] for b in range(B)] for r in range(R)]))


@pytest.mark.parametrize("R,B,P,Q", [(1, 1, 1, 1), (1, 2, 7, 5), (2, 3, 40, 13), (3, 2, 13, 40), (3, 1, 64, 64)])
def test_grad_equals_autograd_and_the_closed_form(R, B, P, Q):
    """grad on the float64 search's tables == autograd through oracle.chamfer.chamfer_pair, for both clouds, and ==
    oracle.chamfer.chamfer_grad_from_indices draw by draw; the tables themselves equal the oracle's search."""
    x, y, gcd = _random_case(R * 100 + P, R, B, P, Q)
    ixy, iyx = _tables(x, y)
    for r in range(R):
        for b in range(B):
            assert np.array_equal(ixy[r, b], och.nn_sqdist(torch.from_numpy(x[r, b]), torch.from_numpy(y[b]))[1].numpy())
            assert np.array_equal(iyx[r, b], och.nn_sqdist(torch.from_numpy(y[b]), torch.from_numpy(x[r, b]))[1].numpy())
    gr = cg.grad(x, y, ixy, iyx, gcd)
    xt, yt = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(y).requires_grad_(True)
    cd = torch.stack([och.chamfer_pair(xt[r], yt) for r in range(R)]).mean(dim=0)
    (cd * torch.from_numpy(gcd)).sum().backward()
    scale = max(np.abs(gr.gx).max(), np.abs(gr.gy).max())
    assert np.abs(gr.gx - xt.grad.numpy()).max() <= 1e-13 * scale and np.abs(gr.gy - yt.grad.numpy()).max() <= 1e-13 * scale
    gy = np.zeros_like(y)
    for r in range(R):
        for b in range(B):
            ax, ay = och.chamfer_grad_from_indices(torch.from_numpy(x[r, b]), torch.from_numpy(y[b]), torch.from_numpy(ixy[r, b]),
                                                   torch.from_numpy(iyx[r, b]), gcd[b] / R)
            assert np.abs(gr.gx[r, b] - ax.numpy()).max() <= 1e-13 * scale
            gy[b] += ay.numpy()
    assert np.abs(gr.gy - gy).max() <= 1e-13 * scale
    assert np.allclose(cg.reduce(*[np.array([[((x[r, b] - y[b][ixy[r, b]]) ** 2).sum(-1) for b in range(B)] for r in range(R)]),
                                    np.array([[((y[b] - x[r, b][iyx[r, b]]) ** 2).sum(-1) for b in range(B)] for r in range(R)])]),
                       cd.detach().numpy(), rtol=1e-13, atol=0)


def test_grad_counts_what_lands_on_an_element():
    """A, Bm, n on a case small enough to write down: x = (0, 1), y = (3,), every table 0 except iyx."""
    x = np.array([[[[0.0, 0, 0], [1.0, 0, 0]]]])
    y = np.array([[[3.0, 0, 0]]])
    gr = cg.grad(x, y, np.zeros((1, 1, 2), dtype=int), np.array([[[1]]]), np.array([2.0]))
    assert np.array_equal(gr.nx[0, 0], [0, 1]) and np.array_equal(gr.ny[0], [2])
    assert np.array_equal(gr.Ax[0, 0, :, 0], [3, 2]) and np.array_equal(gr.Bx[0, 0, :, 0], [0, 2])
    assert np.array_equal(gr.Ay[0, :, 0], [2]) and np.array_equal(gr.By[0, :, 0], [5])
    # gx_0 = 2 (2/2)(0 - 3) = -6, gx_1 = 2 [(2/2)(1 - 3) + (2/1)(1 - 3)] = -12, gy_0 = 2 [(2/1)(3 - 1) + (2/2)(3 + 2)] = 18
    assert np.array_equal(gr.gx[0, 0, :, 0], [-6, -12]) and np.array_equal(gr.gy[0, :, 0], [18])
    bx, by = cg.bounds(gr, x, y, np.array([2.0]))
    # bound 0 only where no term lands and the direct term is 0: point 0 outside its one coordinate; a zero term still costs a quantum
    assert (bx[0, 0, 0, 1:] == 0).all() and (bx[0, 0, :, 0] > 0).all() and (bx[0, 0, 1, 1:] > 0).all() and (by > 0).all()
    assert bx[0, 0, 1, 1] == 2.0 * 2.0 * 2.0 ** -cg.fix_shift(4.0, 1) + cg.DENORM


def test_fix_shift_follows_frexp():
    assert cg.fix_shift(0.0, 1) == 62 - 0 - 1
    assert cg.fix_shift(1.0, 1) == 62 - 1 - 1                     # 1 = 0.5 * 2^1
    assert cg.fix_shift(np.float32(1.0) - np.float32(2.0 ** -24), 1) == 62 - 0 - 1
    assert cg.fix_shift(2.0, 3) == 62 - 2 - 2 and cg.fix_shift(2.0, 4) == 62 - 2 - 3 and cg.fix_shift(2.0, 7) == 62 - 2 - 3
    assert cg.fix_shift(2.0, 8192) == 62 - 2 - 14 and cg.fix_shift(2.0, 8191) == 62 - 2 - 13
    assert cg.fix_shift(2.0 ** -149, 1) == 62 + 148 - 1
    # the bound is formed in fp32: 2^24 + 1 rounds to 2^24 there
    x, y = np.full((1, 1, 1, 3), 2.0 ** 24), np.full((1, 1, 3), 1.0)
    assert cg.scales(x, y, np.ones(1))[0].shift[0, 0] == 62 - 25 - 1


def test_tiles_and_tables():
    assert cg.tile_edges(6144) == (6144, []) and cg.tile_edges(6145) == (3073, [3073]) and cg.tile_edges(8192) == (4096, [4096])
    assert cg.tile_edges(12289) == (4097, [4097, 8194]) and cg.tile_edges(16384) == (5462, [5462, 10924])
    rng = np.random.default_rng(0)
    t = cg.scatter_tables(rng, (2, 3, 8192), 8192)
    assert sorted(t) == ["hub0", "hub4095", "hub4096", "hub8191", "permutation", "random", "tile-edges"]
    assert (np.sort(t["permutation"], axis=-1) == np.arange(8192)).all() and not np.array_equal(t["permutation"][0, 0], t["permutation"][1, 2])
    assert set(np.unique(t["tile-edges"])) == {4095, 4096}
    t = cg.scatter_tables(rng, (1, 1, 2048), 16384)
    assert set(np.unique(t["tile-edges"])) == {5461, 5462, 10923, 10924} and "permutation" not in t
    assert sorted(cg.scatter_tables(rng, (1, 1, 5), 1)) == ["hub0", "random"]
    for name, tab in t.items():
        assert tab.min() >= 0 and tab.max() < 16384, name
    r = cg.random_table(rng, (3, 2, 9), 77)
    assert (r == 0).any(axis=-1).all() and (r == 76).any(axis=-1).all()


def test_grid_search_takes_the_first_minimum():
    rng = np.random.default_rng(1)
    x, y = cg.grid_cloud(rng, 300, 4), cg.grid_cloud(rng, 700, 4)
    assert np.abs(x).max() <= 1 and cg.is_fp32(x) and np.array_equal(x * 16, np.rint(x * 16))
    dist, idx = cg.nn_first(x, y)
    d = ((x[:, None] - y[None]) ** 2).sum(-1) * 256                                       # exact in float64
    assert np.array_equal(dist, d.min(axis=1)) and np.array_equal(idx, d.argmin(axis=1))
    ties = (d == d.min(axis=1, keepdims=True)).sum(axis=1)
    assert (ties > 1).sum() > 30, "the 2^-4 grid is meant to be full of ties between distinct points"
    for i in np.flatnonzero(ties > 1)[:20]:
        assert idx[i] == np.flatnonzero(d[i] == d[i].min())[0]
    with pytest.raises(AssertionError):
        cg.nn_first(x + 1e-3, y)


@pytest.mark.parametrize("number", range(len(cg.EXACT_CASES)))
def test_exact_cases_are_exact_in_fp32(number):
    """The precondition of the bit-for-bit cases: every expected value, computed exactly in float64, is an fp32 number; and the
    fp32 emulation, fused or not, returns exactly it."""
    x, y, gcd, tables = cg.exact_case(number)
    P, Q, R, B = cg.EXACT_CASES[number]
    assert cg.is_fp32(x) and cg.is_fp32(y) and np.abs(x).max() <= 1 and np.abs(y).max() <= 1
    assert all(g == 0 or np.frexp(abs(g))[0] == 0.5 for g in gcd) and (B == 1 or (gcd == 0).any())
    sx, sy = cg.scales(x, y, gcd)
    assert sx.shift.min() >= 44 and sy.shift.min() >= 44
    assert any(k.startswith("x:hub") for k in tables) and any(k.startswith("y:hub") for k in tables)
    for name, (ixy, iyx) in tables.items():
        gr = cg.grad(x, y, ixy, iyx, gcd)
        assert cg.is_fp32(gr.gx) and cg.is_fp32(gr.gy), name
        if P * R <= 8192:                                                                  # the emulation of the large cases: once
            for fused in (None, "ct", "cs"):
                ex, ey = cg.emulate(x, y, ixy, iyx, gcd, fused)
                assert np.array_equal(ex, gr.gx) and np.array_equal(ey, gr.gy), (name, fused)
    if P * R > 8192:
        name = "y:hub0"
        ex, ey = cg.emulate(x, y, *tables[name], gcd)
        gr = cg.grad(x, y, *tables[name], gcd)
        assert np.array_equal(ex, gr.gx) and np.array_equal(ey, gr.gy), name


def _nn_tables32(x, y):
    """The float64 search of fp32 clouds, by the oracle's torch search (threaded: these clouds are the large ones)."""
    xt, yt = torch.from_numpy(x.astype(np.float64)), torch.from_numpy(y.astype(np.float64))
    R, B = x.shape[:2]
    return (np.array([[och.nn_sqdist(xt[r, b], yt[b])[1].numpy() for b in range(B)] for r in range(R)]),
            np.array([[och.nn_sqdist(yt[b], xt[r, b])[1].numpy() for b in range(B)] for r in range(R)]))


@pytest.mark.parametrize("P,Q,outlier", [(6145, 3000, 1e6), (3000, 6145, 1e6), (3000, 6145, 1e12)])
def test_the_bound_holds_for_the_fp32_emulation(P, Q, outlier):
    """Nearest-neighbour tables on the five clouds of the bounded GPU cases (and the far coordinate at 1e12 as well): the
    emulation, with and without the last multiply-add fused, stays within the bound."""
    x, y = cg.bounded_clouds(5, P, Q, outlier)
    x, y = x[:, 3:], y[3:]                                   # the offset cloud and the far coordinate; the scaled ones below
    gcd = np.array(cg.BOUNDED_GCD[3:])
    _check_emulation(x, y, gcd)


def test_the_bound_holds_for_scaled_clouds():
    x, y = cg.bounded_clouds(6, 3000, 6145)
    _check_emulation(x[:1, :3], y[:3], np.array(cg.BOUNDED_GCD[:3]))
    _check_emulation(x[:, :3, :1500], y[:3, :777], np.array(cg.BOUNDED_GCD[:3]))


def _check_emulation(x, y, gcd):
    ixy, iyx = _nn_tables32(x, y)
    gr = cg.grad(x, y, ixy, iyx, gcd)
    bx, by = cg.bounds(gr, x, y, gcd)
    worst = 0.0
    for fused in (None, "ct", "cs"):
        ex, ey = cg.emulate(x, y, ixy, iyx, gcd, fused)
        for e, ref, b in ((ex, gr.gx, bx), (ey, gr.gy, by)):
            err = np.abs(e.astype(np.float64) - ref)
            assert (err <= b).all(), (fused, float((err / np.maximum(b, 1e-300)).max()))
            worst = max(worst, float((err[b > 0] / b[b > 0]).max()))
    print(f"emulation err/bound {x.shape} {y.shape}: {worst:.3f}")
    assert worst <= 1.0


def test_the_bound_is_zero_only_where_nothing_lands():
    x, y = cg.bounded_clouds(7, 50, 20)
    ixy, iyx = _nn_tables32(x, y)
    gr = cg.grad(x, y, ixy, iyx, np.array(cg.BOUNDED_GCD))
    bx, by = cg.bounds(gr, x, y, np.array(cg.BOUNDED_GCD))
    assert (bx > 0).all() and (by > 0).all()                                               # a nearest neighbour is never at distance 0 here
    y[0, 3] = x[0, 0, 5]                                                                   # ... until a point coincides with its neighbour
    ixy, iyx = _nn_tables32(x, y)
    gr = cg.grad(x, y, ixy, iyx, np.array(cg.BOUNDED_GCD))
    bx, _ = cg.bounds(gr, x, y, np.array(cg.BOUNDED_GCD))
    assert ixy[0, 0, 5] == 3 and gr.nx[0, 0, 5] == 1 and (bx[0, 0, 5] > 0).all() and (gr.gx[0, 0, 5] == 0).all()


def test_k_reduce():
    assert cg.k_reduce(1, 1, 1) == 1 + 1 + 1 + 26 and cg.k_reduce(1024, 1025, 3) == 1 + 2 + 3 + 26 and cg.k_reduce(2049, 63, 2) == 3 + 1 + 2 + 26
