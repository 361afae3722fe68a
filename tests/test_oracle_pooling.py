"""oracle.pooling.pool_reference (explicit numpy formulas) against oracle.gcn.image_pooling (the reference's own statement:
a grid_sample call) in float64, on the lattice inputs of the GPU tests: pixel hits, borders, 1-wide and non-square maps,
the depth patch.  Both are float64 evaluations of the same function, so they agree to 1e-12 of the largest value (measured:
4e-16 features, 6e-14 vertex gradient, 1e-13 map gradients)."""
import numpy as np
import pytest
import torch

import pool_lattice as pl
from oracle import gcn as og
from oracle.pooling import pool_reference, project

CASES = {"pyramid": (3, 200, [(8, 23, 23), (4, 7, 7), (4, 3, 3)]),
         "nonsquare": (2, 300, [(8, 5, 9), (12, 17, 3), (4, 1, 5), (4, 9, 1)]),
         "wide": (2, 200, [(4, 32, 32), (4, 46, 46), (4, 5, 5)])}


@pytest.mark.parametrize("name", list(CASES))
def test_pool_reference_matches_grid_sample(name):
    B, N, shapes = CASES[name]
    case = pl.lattice_case(B, N, shapes, seed=sum(map(ord, name)))
    slots = case["slots"]
    pl.assert_geometry_exact(case["verts"], case["sizes"], inexact_quotient_rows=(slots["depth"],))
    flat = case["verts"].reshape(-1, 3).astype(np.float64)
    pr = project(case["verts"], pl.IDENTITY)
    assert pr["z_patched"].reshape(-1).nonzero()[0].tolist() == [slots["depth"]]
    assert pr["ys_patched"].reshape(-1).nonzero()[0].tolist() == [slots["ys"], slots["both"]]
    assert pr["xs_patched"].reshape(-1).nonzero()[0].tolist() == [slots["xs"], slots["both"]]
    # float64 does not overflow where float32 does: those rows get no output gradient (so they add nothing to the map
    # gradients on either side), a harmless position on the grid_sample side, and are left out of the row comparisons
    over = [slots["ys"], slots["xs"], slots["both"]]
    gout = case["grad_out"].astype(np.float64).reshape(B * N, -1).copy()
    gout[over] = 0.0
    gout = gout.reshape(B, N, -1)
    ref = pool_reference(case["maps"], case["verts"], pl.IDENTITY, grad_out=gout)
    v_gs = flat.copy()
    v_gs[over] = (128.0, 128.0, 1.0)
    v_gs[slots["depth"], 2] = float(np.float32(0.1))       # the same patched depth, as a plain value: no patch fires
    v64 = torch.from_numpy(v_gs.reshape(B, N, 3)).requires_grad_(True)
    m64 = [torch.from_numpy(m).double().requires_grad_(True) for m in case["maps"]]
    f = og.image_pooling(m64, v64, matrix=torch.tensor(pl.IDENTITY, dtype=torch.float64))
    (f * torch.from_numpy(gout)).sum().backward()
    keep = np.ones(B * N, dtype=bool)
    keep[over] = False

    def close(a, b, what):
        tol = 1e-12 * np.abs(b).max()
        assert np.abs(a - b).max() <= tol, (what, np.abs(a - b).max(), tol)

    close(f.detach().numpy().reshape(B * N, -1)[keep], ref["feats"].reshape(B * N, -1)[keep], "feats")
    for k, m in enumerate(m64):
        close(m.grad.numpy(), ref["grad_maps"][k], f"grad_maps[{k}]")
    gv, gv_ref = v64.grad.numpy().reshape(B * N, 3).copy(), ref["grad_verts"].reshape(B * N, 3).copy()
    assert gv_ref[slots["depth"], 2] == 0.0 and gv[slots["depth"], 2] != 0.0    # the patch cuts the gradient to the depth
    gv[slots["depth"], 2] = 0.0
    close(gv[keep], gv_ref[keep], "grad_verts")
    assert np.abs(gv_ref).max() > 0 and all(np.abs(g).max() > 0 for g in ref["grad_maps"])
    # the huge vertex: no corner in range on any map with more than one row and column
    assert not ref["grad_verts"].reshape(-1, 3)[slots["huge"]].any()


def test_patch_rows_of_the_reference():
    """The rows float64 cannot reproduce, by their definition: an overflowed coordinate samples at 0.5 (the centre pixel of an
    odd map) and passes no gradient to the vertex through that coordinate; the depth patch divides by float32(0.1)."""
    rng = np.random.default_rng(5)
    maps = [rng.standard_normal((1, 4, 5, 9))]
    verts = np.array([pl.PATCH_VERTS], dtype=np.float32)
    gout = rng.standard_normal((1, 4, 4))
    ref = pool_reference(maps, verts, pl.IDENTITY, grad_out=gout)
    m = maps[0][0]
    # (3e38, 40, .5): ix = 0.5 * 8 = 4, iy = 40 / .5 / 256 * 4 = 1.25
    np.testing.assert_allclose(ref["feats"][0, 1], 0.75 * m[:, 1, 4] + 0.25 * m[:, 2, 4], rtol=1e-14)
    np.testing.assert_allclose(ref["feats"][0, 3], m[:, 2, 4], rtol=1e-14)           # both: the centre pixel
    gv = ref["grad_verts"][0]
    assert gv[1, 0] == 0 and gv[1, 1] != 0 and gv[2, 1] == 0 and gv[2, 0] != 0 and not gv[3].any()
    assert gv[0, 2] == 0 and gv[0, 0] != 0 and gv[0, 1] != 0
    # depth row: d feats / d x = sum_c g_c d f_c / d ix * (W - 1) / (256 * 0.1f), by a central difference in x
    h = 2.0 ** -6
    fd = [pool_reference(maps, verts + np.array([s * h, 0, 0], dtype=np.float32), pl.IDENTITY)["feats"][0, 0] for s in (1, -1)]
    np.testing.assert_allclose(gv[0, 0], (gout[0, 0] * (fd[0] - fd[1])).sum() / (2 * h), rtol=1e-6)
