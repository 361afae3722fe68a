"""CPU: the oracle against the REAL reference's outputs stored in tests/golden/g15_oracle_vs_reference.npz (written by
tests/golden/make_golden.py g15, which imports the reference under oracle/ref_shim.py): the reference's weights, inputs,
adjacency, vertex positions, loss and gradients, so the comparison needs nothing outside the repository."""
import numpy as np
import pytest
import torch

from golden_util import load

CASES = {(False, False, 1): "vision_g1", (True, False, 2): "touch_g2", (True, True, 3): "finger_g3"}


def _dense(z, tag):
    rp, col, val = z[f"{tag}_adj_rowptr"], z[f"{tag}_adj_col"], z[f"{tag}_adj_val"]
    n = rp.shape[0] - 1
    a = np.zeros((n, n), dtype=np.float32)
    a[np.repeat(np.arange(n), np.diff(rp)), col] = val
    return a


@pytest.mark.parametrize("use_touch,finger,grasps", [(False, False, 1), (True, False, 2), (True, True, 3)])
def test_deformation_chamfer_fwd_bwd_live(use_touch, finger, grasps):
    from oracle import chamfer as och, gcn as og
    z = load("g15_oracle_vs_reference.npz")
    tag = CASES[(use_touch, finger, grasps)]
    B = 2
    st = {k[len(tag) + 3:]: torch.from_numpy(z[k]).requires_grad_(True) for k in z.files if k.startswith(f"{tag}_w:")}
    grads = {k[len(tag) + 3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"{tag}_g:")}
    adj, faces = torch.from_numpy(_dense(z, tag)), torch.from_numpy(z[f"{tag}_faces"].astype(np.int64))
    tc, verts, gt = (torch.from_numpy(z[f"{tag}_{k}"]) for k in ("touch_charts", "verts", "gt"))
    out_o, mask_o = og.deformation_forward(st, {"adj": adj}, og.prepare_mesh(tc, verts, B, use_touch), use_touch, 4, 0.33)
    out_r = torch.from_numpy(z[f"{tag}_verts_out"])
    assert torch.equal(torch.from_numpy(z[f"{tag}_mask"]), mask_o)
    # Bit for bit on the BLAS code path that wrote the fixture; another CPU may block its matmuls differently (measured:
    # up to 4.2e-7 with MKL's AVX2 / SSE4.2 kernels), so the forward gets last-bit slack ...
    torch.testing.assert_close(out_o.detach(), out_r, rtol=0, atol=1e-6)
    # ... and the Chamfer term runs on the reference's own vertex values (gradient through the oracle's forward), which
    # keeps the area-weighted surface draws, and so the loss, bit-exact on any CPU
    torch.manual_seed(5)
    loss_o = 9000 * och.chamfer_distance(out_o + (out_r - out_o).detach(), faces, gt, num=400).mean()
    loss_o.backward()
    assert float(z[f"{tag}_loss"]) == loss_o.item()
    assert grads and set(grads) <= set(st)
    for k, g in grads.items():
        err = (g - st[k].grad).abs().max() / g.abs().max().clamp_min(1e-30)
        assert err < 5e-6, k


def test_product_csr_equals_reference_dense():
    from a3vt_amd import mesh as amesh
    z = load("g15_oracle_vs_reference.npz")
    v, f = amesh.load_asset("vision_charts")
    sv, sf = amesh.load_asset("touch_chart")
    for tag, grasps, finger in (("touch_g5", 5, False), ("finger_g5", 5, True), ("touch_g1", 1, False)):
        r, c, n, faces = amesh.fused_pairs(v, f, sf, grasps, finger)
        A = amesh.CSRAdjacency.from_pairs(r, c, n)
        assert np.array_equal(A.to_dense(), _dense(z, tag))
        assert np.array_equal(faces, z[f"{tag}_faces"])
