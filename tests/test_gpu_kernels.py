"""-m gpu: every HIP entry point against the CPU oracle on seeded inputs (fp32, tolerances stated per test)."""
import numpy as np
import pytest
import torch

from helpers import _fuzz_shapes, assert_grad_close, make_args, oracle_adj, random_cloud, rel_err, template

pytestmark = pytest.mark.gpu


def test_library_loads(cuda):
    from a3vt_amd import lib
    assert lib.load().a3vt_version() == 163


@pytest.mark.parametrize("m,k,n", [(128, 16, 16), (1000, 52, 300), (4099, 300, 300), (300, 300, 50), (77, 300, 3),
                                   (32868, 300, 300), (33000, 52, 100)])  # the last two take the main + N-split remainder path
def test_rowgemm_matches_fp64(cuda, m, k, n):
    from a3vt_amd import ops
    g = torch.Generator().manual_seed(m + k + n)
    a = torch.randn(m, k, generator=g)
    w = torch.randn(k, n, generator=g)
    c = ops.rowgemm(a.to(cuda), w.to(cuda)).cpu()
    ref = (a.double() @ w.double())
    # fp32 fma chain over K <= 300: ~1e-6 relative to the row scale
    assert rel_err(c, ref) < 2e-6


@pytest.mark.parametrize("bf16", [False, True])
def test_rowgemm_shape_fuzz(cuda, bf16):
    """Every launch path of a3vt_rowgemm (column blocks for few rows, 1/4/8/13/19-tile kernels, main + rowtile remainder
    split, ragged last tile, K tail chunk) on 48 seeded random shapes against fp64 (operands rounded to bf16 first in
    the bf16 operand mode)."""
    from a3vt_amd import ops
    from oracle.gcn import bf16_round
    for m, k, n in _fuzz_shapes(48, 20261002):
        g = torch.Generator().manual_seed(m * 7 + k * 3 + n)
        a = torch.randn(m, k, generator=g)
        w = torch.randn(k, n, generator=g)
        c = ops.rowgemm(a.to(cuda), w.to(cuda), bf16=bf16).cpu()
        if bf16:
            ref = bf16_round(a).double() @ bf16_round(w).double()
        else:
            ref = a.double() @ w.double()
        assert c.shape == (m, n)
        assert torch.isfinite(c).all(), (m, k, n)
        assert rel_err(c, ref) < 3e-6, (m, k, n, rel_err(c, ref))


def _state_to(dev, st):
    return {k: v.to(dev) for k, v in st.items()}


@pytest.mark.parametrize("tname,use_touch,L,H,B", [("ico2", False, 3, 32, 3), ("atlas", True, 4, 300, 2),
                                                     ("ico3", False, 20, 300, 2), ("ico2", False, 1, 300, 2),
                                                     ("ico4", False, 3, 300, 13),   # 33306 rows: split launches
                                                     ("ico2", False, 36, 32, 2)])   # 35 hidden layers: two launches of weight images
def test_gcn_stack_fwd_bwd(cuda, tname, use_touch, L, H, B):
    from a3vt_amd import mesh as amesh, ops
    from oracle import gcn as og
    args = make_args(use_touch=use_touch, num_GCN_layers=L, hidden_GCN_size=H, num_grasps=1)
    verts, faces = template(tname)
    adj_o, _ = oracle_adj(verts, faces, args)
    n = adj_o[0].numel() - 1
    st = og.init_state(50, H, L, seed=3)
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(B, n, 50, generator=g) * 0.5
    gup = torch.randn(B, n, 3, generator=g)
    # oracle (float64 reference of the same weights)
    st64 = {k: v.double().requires_grad_(True) for k, v in st.items() if k.startswith("mesh_deform_1")}
    f64 = feats.double().requires_grad_(True)
    out_o = og.gcn(f64, st64, "mesh_deform_1", (adj_o[0], adj_o[1], adj_o[2].double()), L, 0.33)
    (out_o * gup.double()).sum().backward()
    # HIP
    if use_touch:
        sv, sf = amesh.load_asset("touch_chart")
        r, c, nn_, _ = amesh.fused_pairs(verts, faces, sf, 1, False)
    else:
        r, c = amesh.vision_pairs(faces, verts.shape[0])
        nn_ = verts.shape[0]
    adj = ops.DeviceCSR(amesh.CSRAdjacency.from_pairs(r, c, nn_), cuda)
    ws = [st[f"mesh_deform_1.layers.{i}.weight"].to(cuda).requires_grad_(True) for i in range(L)]
    bs = [st[f"mesh_deform_1.layers.{i}.bias"].to(cuda).requires_grad_(True) for i in range(L)]
    fd = torch.nn.functional.pad(feats, (0, 2)).to(cuda).requires_grad_(True)
    out = ops.gcn_stack(fd, adj, 50, H, round(H * 0.33), ws, bs)
    (out * gup.to(cuda)).sum().backward()
    assert rel_err(out, out_o) < 1e-4
    # gradients: tolerant of the rare ReLU-kink flips (helpers.assert_grad_close)
    assert_grad_close(fd.grad[..., :50], f64.grad, "grad_feats")
    assert fd.grad[..., 50:].abs().max().item() == 0.0
    for i in range(L):
        assert_grad_close(ws[i].grad, st64[f"mesh_deform_1.layers.{i}.weight"].grad, f"dW layer {i}")
        assert_grad_close(bs[i].grad, st64[f"mesh_deform_1.layers.{i}.bias"].grad, f"db layer {i}")


def test_gcn_stack_config_fuzz(cuda):
    """Twelve seeded random (template, layers, hidden, cut, batch) stacks against the fp64 oracle: hidden any multiple
    of 4 up to 304, cut ratios that put 0 .. hidden channels through the aggregation, 1-5 layers."""
    from a3vt_amd import mesh as amesh, ops
    from oracle import gcn as og
    rng = np.random.default_rng(77)
    for it in range(12):
        tname = ["ico1", "ico2", "ico3", "atlas"][int(rng.integers(0, 4))]
        L, H, B = int(rng.integers(1, 6)), 4 * int(rng.integers(2, 77)), int(rng.integers(1, 5))
        cut = float(rng.choice([0.0, 0.1, 0.33, 0.5, 0.77, 1.0]))
        args = make_args(num_GCN_layers=L, hidden_GCN_size=H, cut=cut)
        verts, faces = template(tname)
        adj_o, _ = oracle_adj(verts, faces, args)
        n = adj_o[0].numel() - 1
        st = og.init_state(50, H, L, seed=100 + it)
        g = torch.Generator().manual_seed(500 + it)
        feats = torch.randn(B, n, 50, generator=g) * 0.5
        gup = torch.randn(B, n, 3, generator=g)
        st64 = {k: v.double().requires_grad_(True) for k, v in st.items() if k.startswith("mesh_deform_1")}
        f64 = feats.double().requires_grad_(True)
        out_o = og.gcn(f64, st64, "mesh_deform_1", (adj_o[0], adj_o[1], adj_o[2].double()), L, cut)
        (out_o * gup.double()).sum().backward()
        r, c = amesh.vision_pairs(faces, verts.shape[0])
        adj = ops.DeviceCSR(amesh.CSRAdjacency.from_pairs(r, c, verts.shape[0]), cuda)
        ws = [st[f"mesh_deform_1.layers.{i}.weight"].to(cuda).requires_grad_(True) for i in range(L)]
        bs = [st[f"mesh_deform_1.layers.{i}.bias"].to(cuda).requires_grad_(True) for i in range(L)]
        fd = torch.nn.functional.pad(feats, (0, 2)).to(cuda).requires_grad_(True)
        out = ops.gcn_stack(fd, adj, 50, H, round(H * cut), ws, bs)
        (out * gup.to(cuda)).sum().backward()
        tag = f"[{it}: {tname} L={L} H={H} cut={cut} B={B}]"
        assert rel_err(out, out_o) < 1e-4, tag
        assert_grad_close(fd.grad[..., :50], f64.grad, "grad_feats " + tag)
        for i in range(L):
            assert_grad_close(ws[i].grad, st64[f"mesh_deform_1.layers.{i}.weight"].grad, f"dW layer {i} " + tag)
            assert_grad_close(bs[i].grad, st64[f"mesh_deform_1.layers.{i}.bias"].grad, f"db layer {i} " + tag)


@pytest.mark.parametrize("tname,use_touch,B,kin,nout,cut,do_cut,relu", [
    ("ico2", False, 3, 300, 300, 0.33, True, True),      # a hidden layer of any consumer
    ("ico2", False, 3, 300, 300, 0.33, False, False),    # auto-encoder encoder's last layer (autoencoder/model.py:59-64)
    ("atlas", True, 2, 300, 200, 0.33, True, True),      # DDQN graph model: 3*100 inputs -> hidden_dim
    ("atlas", True, 2, 200, 50, 0.33, False, False),     # DDQN: hidden_dim -> num_actions, all channels aggregated
    ("ico2", False, 2, 50, 300, 0.33, True, True),       # unpadded 50-wide input (padded to 52 by the module)
    ("ico2", False, 2, 37, 30, 0.5, True, False),        # odd sizes, identity activation with the cut
    ("ico2", False, 2, 300, 3, 0.33, False, False),      # 3-channel output through the generic path
    ("ico2", False, 2, 64, 128, 0.0, True, True),        # cut 0: nothing aggregated
    ("ico3", False, 2, 448, 300, 0.33, True, True),      # 448-wide (image-model) input
    ("ico4", False, 13, 300, 300, 0.33, True, True)])    # 33306 rows: split launches
def test_gcn_layer_standalone(cuda, tname, use_touch, B, kin, nout, cut, do_cut, relu):
    """Product ``GCN_layer.forward(features, adj, activation)`` (reference model.py:351-363) with a dense adjacency
    tensor and with a CSR handle, against the fp64 oracle: output 1e-4 (north_star), gradients 1e-3 (helpers)."""
    from a3vt_amd import ops
    from a3vt_amd.pterotactyl.reconstruction.vision import model
    from oracle import gcn as og, mesh as omesh
    from a3vt_amd import mesh as amesh
    args = make_args(use_touch=use_touch, num_grasps=1)
    verts, faces = template(tname)
    sv, sf = amesh.load_asset("touch_chart")
    dense = torch.from_numpy(omesh.adj_init(verts, faces, use_touch, 1, False, sv, sf)["adj"]).float()
    adj_o, _ = oracle_adj(verts, faces, args)
    n = dense.shape[0]
    torch.manual_seed(5)
    layer = model.GCN_layer(kin, nout, cut, do_cut).to(cuda)
    g = torch.Generator().manual_seed(kin + nout)
    x = torch.randn(B, n, kin, generator=g) * 0.5
    gy = torch.randn(B, n, nout, generator=g)
    w64 = layer.weight.detach().cpu().double().requires_grad_(True)
    b64 = layer.bias.detach().cpu().double().requires_grad_(True)
    x64 = x.double().requires_grad_(True)
    y_o = og.gcn_layer(x64, w64, b64, (adj_o[0], adj_o[1], adj_o[2].double()), cut, do_cut, relu)
    (y_o * gy.double()).sum().backward()
    act = torch.nn.functional.relu if relu else (lambda t: t)
    for adj in (dense.to(cuda), model._csr_from_arg(dense.to(cuda))):
        layer.zero_grad()
        xd = x.to(cuda).requires_grad_(True)
        y = layer(xd, adj, act)
        assert y.shape == (B, n, nout)
        (y * gy.to(cuda)).sum().backward()
        assert rel_err(y, y_o) < 1e-4
        assert_grad_close(xd.grad, x64.grad, "grad_x")
        assert_grad_close(layer.weight.grad, w64.grad, "grad_weight")
        assert_grad_close(layer.bias.grad, b64.grad, "grad_bias")
        if do_cut:  # dead bias channels get exact zeros (model.py:358)
            assert layer.bias.grad[round(nout * cut):].abs().max().item() == 0.0


def test_image_pool_fwd_bwd(cuda):
    """Fused projection + bilinear pooling (a3vt_image_pool_fwd/bwd) vs the oracle's restatement of
    Image_Encoder.pooling (model.py:70-103) in float64: default pyramid sizes (64x23x23, 128x7x7, 256x3x3), vertices
    inside the image, on its border and projected outside it (zero padding)."""
    from a3vt_amd import ops
    from oracle import gcn as og
    B, N = 3, 700
    g = torch.Generator().manual_seed(12)
    verts = (torch.rand(B, N, 3, generator=g) - 0.5) * 0.5
    verts[:, :40] *= 6.0                                     # far off-screen: all four corners out of range
    maps = [torch.randn(B, c, h, h, generator=g) for c, h in ((64, 23), (128, 7), (256, 3))]
    gout = torch.randn(B, N, 448, generator=g)
    matrix = og.projection_matrix().float()
    v64 = verts.double().requires_grad_(True)
    m64 = [m.double().requires_grad_(True) for m in maps]
    f_o = og.image_pooling(m64, v64)
    (f_o * gout.double()).sum().backward()
    vd = verts.to(cuda).requires_grad_(True)
    md = [m.to(cuda).requires_grad_(True) for m in maps]
    f = ops.image_pool(vd, matrix, md)
    assert f.shape == (B, N, 448)
    (f * gout.to(cuda)).sum().backward()
    assert rel_err(f, f_o) < 1e-5
    assert (f[:, :40].abs().sum(-1) == 0).float().mean() > 0.5          # most far vertices sample nothing
    for k in range(3):
        assert md[k].grad.shape == maps[k].shape and rel_err(md[k].grad, m64[k].grad) < 1e-5
    # position gradient: piecewise-smooth in the position (kinks at pixel boundaries) -> L2 + outlier tolerant check
    assert_grad_close(vd.grad, v64.grad, "grad_verts")
    # channels_last input is consumed as is, and the result does not depend on the input memory format
    f2 = ops.image_pool(vd.detach(), matrix, [m.detach().contiguous(memory_format=torch.channels_last) for m in md])
    assert torch.equal(f2, f.detach())
    # the backward scatter into the maps accumulates in fixed point: a second evaluation reproduces every bit
    vd2 = verts.to(cuda).requires_grad_(True)
    md2 = [m.to(cuda).requires_grad_(True) for m in maps]
    (ops.image_pool(vd2, matrix, md2) * gout.to(cuda)).sum().backward()
    assert torch.equal(vd2.grad, vd.grad) and all(torch.equal(a.grad, b.grad) for a, b in zip(md, md2))
    # round 6: the vertex-feature sum of the image models (model.py:243,265,277) in the pooling's own pass — the same fp32 add,
    # so the same bits as `base + image_pool(...)`; the gradient of `base` is the output gradient itself
    base = torch.randn(B, N, 448, generator=g).to(cuda).requires_grad_(True)
    vd3 = verts.to(cuda).requires_grad_(True)
    md3 = [m.to(cuda).requires_grad_(True) for m in maps]
    f3 = ops.image_pool(vd3, matrix, md3, base=base)
    assert torch.equal(f3.detach(), base.detach() + f.detach())
    (f3 * gout.to(cuda)).sum().backward()
    assert torch.equal(base.grad, gout.to(cuda)) and torch.equal(vd3.grad, vd.grad)
    assert all(torch.equal(a.grad, b.grad) for a, b in zip(md, md3))
    with pytest.raises(RuntimeError):
        ops.image_pool(vd3.detach(), matrix, [m.detach() for m in md3], base=base.detach()[..., :440])


@pytest.mark.parametrize("m,k,n", [(1000, 52, 300), (4099, 300, 300), (33000, 300, 300), (777, 300, 52)])
def test_rowgemm_bf16_operand_mode(cuda, m, k, n):
    """gemm_bf16 = 1: operands rounded to bf16 (RNE), exact products, fp32 accumulation — checked against exactly that
    arithmetic in float64 (tolerance = fp32 accumulation only), and against the unrounded product at the bf16 level."""
    from a3vt_amd import ops
    from oracle import gcn as og
    g = torch.Generator().manual_seed(m + k + n)
    a = torch.randn(m, k, generator=g)
    w = torch.randn(k, n, generator=g)
    c = ops.rowgemm(a.to(cuda), w.to(cuda), bf16=True).cpu()
    ref_bf = og.bf16_round(a).double() @ og.bf16_round(w).double()
    assert rel_err(c, ref_bf) < 2e-6
    assert 1e-4 < rel_err(c, a.double() @ w.double()) < 2e-2      # it really is the rounded product


@pytest.mark.parametrize("tname,use_touch,L,B", [("ico2", False, 3, 3), ("atlas", True, 6, 2), ("ico4", False, 3, 13)])
def test_gcn_stack_bf16_mode(cuda, tname, use_touch, L, B):
    """BASELINE configs[3]/[4] ("bf16 + MFMA feature MLP"): the stack with bf16 GEMM operands.  Forward against the
    oracle's emulation of the same rounding (float64 otherwise) and against the fp32 path; gradients against autograd of
    that emulation at the bf16 level.  Autograd through ``bf16_round`` rounds the GRADIENT at every rounding point: it rounds
    dW, grad_feats and the outputs of the backward products to bf16, where the device rounds their operands and keeps dW and
    grad_feats in fp32 — most of the measured gap.  tests/test_gpu_bf16_exact.py holds this mode to an emulation that
    rounds where the kernels do."""
    from a3vt_amd import mesh as amesh, ops
    from oracle import gcn as og
    from helpers import rel_l2
    H = 300
    args = make_args(use_touch=use_touch, num_GCN_layers=L, hidden_GCN_size=H, num_grasps=1)
    verts, faces = template(tname)
    adj_o, _ = oracle_adj(verts, faces, args)
    n = adj_o[0].numel() - 1
    st = og.init_state(50, H, L, seed=3)
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(B, n, 50, generator=g) * 0.5
    gup = torch.randn(B, n, 3, generator=g)
    st64 = {k: v.double().requires_grad_(True) for k, v in st.items() if k.startswith("mesh_deform_1")}
    f64 = feats.double().requires_grad_(True)
    adj64 = (adj_o[0], adj_o[1], adj_o[2].double())
    with torch.no_grad():
        out_fp32 = og.gcn(feats.double(), {k: v.detach() for k, v in st64.items()}, "mesh_deform_1", adj64, L, 0.33)
    # emulated forward with autograd straight through the roundings: same ReLU masks as the device forward (up to
    # rounding ties); its backward rounds the gradients at each bf16_round (see the docstring)
    out_emul = og.gcn(f64, st64, "mesh_deform_1", adj64, L, 0.33, bf16=True)
    (out_emul * gup.double()).sum().backward()
    if use_touch:
        sv, sf = amesh.load_asset("touch_chart")
        r, c, nn_, _ = amesh.fused_pairs(verts, faces, sf, 1, False)
    else:
        r, c = amesh.vision_pairs(faces, verts.shape[0])
        nn_ = verts.shape[0]
    adj = ops.DeviceCSR(amesh.CSRAdjacency.from_pairs(r, c, nn_), cuda)
    ws = [st[f"mesh_deform_1.layers.{i}.weight"].to(cuda).requires_grad_(True) for i in range(L)]
    bs = [st[f"mesh_deform_1.layers.{i}.bias"].to(cuda).requires_grad_(True) for i in range(L)]
    fd = torch.nn.functional.pad(feats, (0, 2)).to(cuda).requires_grad_(True)
    out = ops.gcn_stack(fd, adj, 50, H, 99, ws, bs, bf16=True)
    (out * gup.to(cuda)).sum().backward()
    # same rounding -> close (a value within fp32 rounding of a bf16 tie may round the other way and move one element by
    # 2^-8; hence 2e-3 rather than 1e-5); bf16 level against the exact path
    assert rel_err(out, out_emul) < 2e-3 and rel_l2(out, out_emul) < 2e-4
    assert rel_l2(out, out_fp32) < 1e-2
    errs = [rel_l2(fd.grad[..., :50], f64.grad)]
    for i in range(L):
        errs.append(rel_l2(ws[i].grad, st64[f"mesh_deform_1.layers.{i}.weight"].grad))
        errs.append(rel_l2(bs[i].grad, st64[f"mesh_deform_1.layers.{i}.bias"].grad))
    assert max(errs) < 3e-2, errs
    # the default path is untouched by the flag
    out32 = ops.gcn_stack(fd.detach(), adj, 50, H, 99, [w.detach() for w in ws], [b.detach() for b in bs])
    assert rel_err(out32, out_fp32) < 1e-4


@pytest.mark.parametrize("B,N", [(3, 517), (16, 2563)])   # one tile per wave; several tiles per wave and a ragged last tile
def test_posenc_mask_fwd_bwd(cuda, B, N):
    from a3vt_amd import ops
    from oracle import gcn as og
    st = og.init_state(50, 8, 1, seed=5)
    g = torch.Generator().manual_seed(2)
    verts = (torch.rand(B, N, 3, generator=g) - 0.5) * 0.6
    mask = torch.randint(0, 4, (B, N, 1), generator=g).float()
    gout = torch.randn(B, N, 52, generator=g)
    gout[..., 50:] = 0
    names = ["positional_encoder.model.0.weight", "positional_encoder.model.0.bias",
             "positional_encoder.model.2.weight", "positional_encoder.model.2.bias",
             "positional_encoder.model.4.weight", "positional_encoder.model.4.bias", "mask_encoder.model.0.weight"]
    st64 = {k: st[k].double().requires_grad_(True) for k in names}
    v64 = verts.double().requires_grad_(True)
    f_o = og.positional_encoder(v64, st64) + og.mask_encoder(mask, st64)
    (f_o * gout[..., :50].double()).sum().backward()
    packed = torch.cat([st[k].reshape(-1) for k in names]).to(cuda).requires_grad_(True)
    vd = verts.to(cuda).requires_grad_(True)
    f = ops.PosEncMaskFn.apply(vd, mask.to(cuda), packed, 50, 52)
    (f * gout.to(cuda)).sum().backward()
    assert rel_err(f[..., :50], f_o) < 1e-5
    assert f[..., 50:].abs().max().item() == 0.0
    g_o = torch.cat([st64[k].grad.reshape(-1) for k in names])
    if B * N < 4096:
        assert rel_err(vd.grad, v64.grad) < 1e-4
        assert rel_err(packed.grad, g_o) < 1e-4
    else:
        # 41 008 vertices x 37 ReLU arguments: one of them lies within float32 rounding of zero and takes the other branch
        # than in float64, which moves that vertex's gradient by 1.5e-2 of the largest one (the round-3 kernel gives the same
        # figure) — every other element agrees to 1e-4, the whole tensor to 1e-4 in relative L2
        assert_grad_close(vd.grad, v64.grad, "grad_verts", tol=1e-4, outlier_frac=1e-4, l2_tol=1e-3)
        assert_grad_close(packed.grad, g_o, "grad_params", tol=1e-3, outlier_frac=1e-3, l2_tol=1e-3)


@pytest.mark.parametrize("I,B,N", [(448, 3, 1949), (448, 1, 37), (64, 2, 700), (200, 2, 333)])
def test_posenc_mask_wide_fwd_bwd(cuda, I, B, N):
    """The vertex-feature encoder at the image models' input size (448) and two other wide sizes:
    a3vt_posenc_wide_fwd / _bwd (three augmented products on the fp32 matrix pipe, csrc/posenc_wide.hip) against the fp64
    oracle of Positional_Encoder + Mask_Encoder (model.py:381-414): features, position gradient, every parameter gradient
    (biases and the mask embedding come out of the augmented weight gradients), 1e-4; bit-reproducible."""
    from a3vt_amd import ops
    from oracle import gcn as og
    st = og.init_state(I, 8, 1, seed=7)
    g = torch.Generator().manual_seed(I + N)
    verts = (torch.rand(B, N, 3, generator=g) - 0.5) * 0.6
    mask = torch.randint(0, 4, (B, N, 1), generator=g).float()
    gout = torch.randn(B, N, I, generator=g)
    names = ["positional_encoder.model.0.weight", "positional_encoder.model.0.bias",
             "positional_encoder.model.2.weight", "positional_encoder.model.2.bias",
             "positional_encoder.model.4.weight", "positional_encoder.model.4.bias", "mask_encoder.model.0.weight"]
    st64 = {k: st[k].double().requires_grad_(True) for k in names}
    v64 = verts.double().requires_grad_(True)
    f_o = og.positional_encoder(v64, st64) + og.mask_encoder(mask, st64)
    (f_o * gout.double()).sum().backward()
    g_o = torch.cat([st64[k].grad.reshape(-1) for k in names])
    outs = []
    for _ in range(2):
        packed = torch.cat([st[k].reshape(-1) for k in names]).to(cuda).requires_grad_(True)
        vd = verts.to(cuda).requires_grad_(True)
        f = ops.PosEncMaskFn.apply(vd, mask.to(cuda), packed, I, I)
        (f * gout.to(cuda)).sum().backward()
        outs.append((f.detach(), vd.grad, packed.grad))
    f, gv, gp = outs[0]
    assert f.shape == (B, N, I)
    assert rel_err(f, f_o) < 1e-5
    assert rel_err(gv, v64.grad) < 1e-4
    assert rel_err(gp, g_o) < 1e-4
    off = 0
    for k in names:                       # every tensor on its own scale (the embedding rows are small next to W3's)
        n = st[k].numel()
        assert rel_err(gp[off:off + n], st64[k].grad.reshape(-1)) < 2e-4, k
        off += n
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    with torch.no_grad():                 # forward-only call: no activations are kept
        f2 = ops.PosEncMaskFn.apply(verts.to(cuda), mask.to(cuda), packed.detach(), I, I)
    assert torch.equal(f2, f)


@pytest.mark.parametrize("P,Q,B,draws", [(1, 1, 1, 1), (100, 37, 2, 3), (1000, 2176, 2, 1), (4099, 5000, 1, 2)])
def test_chamfer_fwd_bwd(cuda, P, Q, B, draws):
    from a3vt_amd import ops
    from oracle import chamfer as och
    x = random_cloud(draws * B, P, 1).reshape(draws, B, P, 3) * 1.1
    y = random_cloud(B, Q, 2)
    gcd = torch.rand(B) + 0.5
    xd = x.to(cuda).requires_grad_(True)
    yd = y.to(cuda).requires_grad_(True)
    cd = ops.ChamferFn.apply(xd, yd)
    (cd * gcd.to(cuda)).sum().backward()
    x64 = x.double().requires_grad_(True)
    y64 = y.double().requires_grad_(True)
    cd_o = torch.stack([och.chamfer_pair(x64[r], y64) for r in range(draws)]).mean(0)
    (cd_o * gcd.double()).sum().backward()
    assert rel_err(cd, cd_o) < 1e-5
    assert rel_err(xd.grad, x64.grad) < 1e-4
    assert rel_err(yd.grad, y64.grad) < 1e-4
    # nearest-neighbour distances bit-for-bit against the plain-C oracle (same fp32 arithmetic, fma aside)
    dxy, ixy, dyx, iyx, _ = ops.chamfer_nn(xd.detach(), yd.detach())
    dc, _ = och.nn_sqdist_c(x[0, 0].numpy(), y[0].numpy())
    assert np.allclose(dxy[0, 0].cpu().numpy(), dc, rtol=1e-5, atol=1e-12)
    # indices must point at a candidate realising the reported distance
    yy = y[0][ixy[0, 0].cpu().long()]
    assert np.allclose(((x[0, 0] - yy) ** 2).sum(-1).numpy(), dxy[0, 0].cpu().numpy(), rtol=1e-5, atol=1e-12)


@pytest.mark.parametrize("single_pass", [True, False])
@pytest.mark.parametrize("P,R", [(1280, 5), (1024, 4), (1536, 6), (200, 3), (2048, 8), (2560, 10)])
def test_chamfer_nn_every_queries_per_lane_variant(cuda, P, R, single_pass):
    """launch_nn / launch_nn2 pick the queries-per-lane template from the workgroup count per CU (chamfer.hip); 256 clouds
    of these sizes select R = 5 / 4 / 6 / 3 (and 8 / 10 in the single-pass search; the two-pass one falls back to 4 and
    5 there).  Distances and first-arg-min indices against a brute-force fp64 search (the clouds hold duplicated points,
    so ties exist and the lowest index must win)."""
    from a3vt_amd import ops
    B, Q = 256, 200
    g = torch.Generator().manual_seed(P)
    x = (torch.rand(1, B, P, 3, generator=g) * 0.3).float()
    y = (torch.rand(B, Q, 3, generator=g) * 0.3).float()
    y[:, Q // 2:] = y[:, :Q - Q // 2]          # every candidate twice: exact distance ties
    x[0, :, :7] = y[:, :7]                     # and a few zero distances
    dxy, ixy, dyx, iyx, _ = ops.chamfer_nn(x.to(cuda), y.to(cuda), single_pass=single_pass)
    for b in (0, 1, B // 2, B - 1):
        d = ((x[0, b].double()[:, None, :] - y[b].double()[None, :, :]) ** 2).sum(-1)
        ref_d, ref_i = d.min(1)
        # first arg-min of the fp32 distances the kernel computes: compare through the reported distance
        got_i = ixy[0, b].cpu().long()
        got_d = dxy[0, b].cpu().double()
        assert torch.allclose(got_d, ref_d, rtol=1e-5, atol=1e-12)
        assert (got_i < Q // 2 + (Q - 2 * (Q // 2))).all()      # of two identical candidates the first one
        assert torch.allclose(d[torch.arange(P), got_i], ref_d, rtol=1e-5, atol=1e-12)
        d2 = d.t()
        ref_d2, _ = d2.min(1)
        assert torch.allclose(dyx[0, b].cpu().double(), ref_d2, rtol=1e-5, atol=1e-12)
        assert torch.allclose(d2[torch.arange(Q), iyx[0, b].cpu().long()], ref_d2, rtol=1e-5, atol=1e-12)


@pytest.mark.parametrize("draws,B,P,Q,dup", [(1, 1, 1, 1, False), (1, 2, 100, 37, False), (3, 2, 1000, 2176, True),
                                             (2, 1, 4099, 5000, False), (2, 3, 777, 1025, True), (1, 1, 5, 3000, False),
                                             (1, 64, 2600, 700, True)])
def test_chamfer_single_pass_equals_two_pass(cuda, draws, B, P, Q, dup):
    """The single-pass search (both directions from one sweep over the distance matrix, column minima folded through DPP
    butterflies and 64-bit atomic minima of (distance, wave, lane)) against the two-pass search: every output bit for bit,
    including the tie rule (duplicated queries AND candidates: lowest index wins in both directions)."""
    from a3vt_amd import ops
    g = torch.Generator().manual_seed(P * 7 + Q)
    x = (torch.rand(draws, B, P, 3, generator=g) * 0.3).float()
    y = (torch.rand(B, Q, 3, generator=g) * 0.3).float()
    if dup:
        y[:, Q // 2:] = y[:, :Q - Q // 2]
        x[:, :, P // 2:] = x[:, :, :P - P // 2]
        x[0, :, :3] = y[:, :3]
    a = ops.chamfer_nn(x.to(cuda), y.to(cuda), single_pass=False)
    b = ops.chamfer_nn(x.to(cuda), y.to(cuda), single_pass=True)
    for name, u, v in zip(("dist_xy", "idx_xy", "dist_yx", "idx_yx", "cd"), a, b):
        assert torch.equal(u, v), f"{name}: {(u != v).sum().item()} of {u.numel()} differ"


def test_chamfer_known_answers(cuda):
    from a3vt_amd import ops
    x = random_cloud(2, 300, 4).to(cuda)
    cd = ops.ChamferFn.apply(x[None], x)
    assert cd.abs().max().item() == 0.0                      # a cloud against itself
    t = torch.tensor([1e-4, -2e-4, 5e-5], device=cuda)       # shift far below the point spacing -> 2|t|^2
    cd2 = ops.ChamferFn.apply((x + t)[None], x)
    assert abs(cd2[0].item() - 2 * (t ** 2).sum().item()) < 1e-3 * 2 * (t ** 2).sum().item()


def test_sample_points_injected_and_grad(cuda):
    from a3vt_amd import ops
    from oracle import chamfer as och
    verts, faces = template("ico2")
    B, num, draws = 3, 500, 2
    g = torch.Generator().manual_seed(9)
    v = torch.from_numpy(verts)[None].repeat(B, 1, 1) + 0.02 * torch.randn(B, verts.shape[0], 3, generator=g)
    f = torch.from_numpy(faces)
    fi = torch.randint(0, f.shape[0], (draws, B, num), generator=g)
    u = torch.rand(draws, B, num, generator=g)
    w = torch.rand(draws, B, num, generator=g)
    gp = torch.randn(draws, B, num, 3, generator=g)
    vd = v.to(cuda).requires_grad_(True)
    pts = ops.SamplePointsFn.apply(vd, f.to(torch.int32).to(cuda), num, draws, 0, 0, fi.to(torch.int32).to(cuda),
                                   u.to(cuda), w.to(cuda))
    (pts * gp.to(cuda)).sum().backward()
    v64 = v.double().requires_grad_(True)
    pts_o = torch.stack([och.sample_points(v64, f, fi[r], u[r].double(), w[r].double()) for r in range(draws)])
    (pts_o * gp.double()).sum().backward()
    assert rel_err(pts, pts_o) < 1e-6
    assert rel_err(vd.grad, v64.grad) < 1e-5


def test_sample_points_rng_statistics(cuda):
    """Philox + inverse-CDF path: face histogram proportional to area, zero-area faces never drawn,
    barycentric weights inside the triangle, points on the faces' planes."""
    from a3vt_amd import ops
    from oracle import chamfer as och
    verts, faces = template("ico1")
    v = torch.from_numpy(verts)[None].clone()
    v[0, faces[3]] = v[0, faces[3][0]].clone()  # collapse face 3 (and shrink its neighbours)
    f = torch.from_numpy(faces)
    num = 200000
    pts = ops.SamplePointsFn.apply(v.to(cuda), f.to(torch.int32).to(cuda), num, 1, 1234, 0, None, None, None)
    assert torch.isfinite(pts).all()
    prob = och.face_probabilities(v, f)[0].numpy()
    # recover the face of each sample through the saved indices of a second identical call
    from a3vt_amd import lib
    L = lib.load()
    vdev, fdev = v.to(cuda), f.to(torch.int32).to(cuda)   # keep the device copies alive across the raw C calls
    cdf = torch.empty(1, f.shape[0], device=cuda)
    lib.check(L.a3vt_face_cdf(lib.ptr(vdev), lib.ptr(fdev), 1, v.shape[1], f.shape[0], lib.ptr(cdf), None), "cdf")
    torch.cuda.synchronize()
    assert np.allclose(cdf[0].cpu().numpy(), np.cumsum(prob), rtol=1e-5, atol=1e-6)
    fi = torch.empty(1, 1, num, dtype=torch.int32, device=cuda)
    uu = torch.empty(1, 1, num, device=cuda)
    vv = torch.empty(1, 1, num, device=cuda)
    p2 = torch.empty(1, 1, num, 3, device=cuda)
    lib.check(L.a3vt_sample_points_fwd(lib.ptr(vdev), lib.ptr(fdev), lib.ptr(cdf), 1, v.shape[1], f.shape[0], 1, num,
                                       None, None, None, 1234, 0, lib.ptr(p2), lib.ptr(fi), lib.ptr(uu), lib.ptr(vv),
                                       None), "sample")
    torch.cuda.synchronize()
    assert torch.equal(p2, pts)                               # same seed/offset -> same cloud
    hist = np.bincount(fi.cpu().numpy().ravel(), minlength=f.shape[0]) / num
    assert hist[prob == 0].sum() == 0
    assert np.abs(hist - prob).max() < 4 * np.sqrt(prob.max() / num) + 1e-3
    assert 0.0 <= uu.min().item() and uu.max().item() < 1.0 and abs(uu.mean().item() - 0.5) < 5e-3
    assert abs(vv.mean().item() - 0.5) < 5e-3


@pytest.mark.parametrize("B,C,H,W,dt", [(4, 3, 61, 59, "bf16"), (64, 3, 254, 254, "bf16"), (5, 16, 126, 126, "bf16"),
                                        (3, 48, 17, 9, "fp32"), (2, 512, 3, 3, "bf16"), (1, 24, 7, 5, "fp32"),
                                        (2, 7, 11, 13, "bf16")])
def test_bias_grad_nhwc_is_the_column_sum(cuda, B, C, H, W, dt):
    """a3vt_bias_grad_nhwc against a float64 sum of the same (bf16 or fp32) values; repeatable bit for bit.
    Tolerance: fp32 accumulation of B*H*W terms in a fixed tree, 1e-5 of the sum of magnitudes."""
    from a3vt_amd import ops
    g = torch.Generator().manual_seed(B * C + H)
    x = torch.randn(B, C, H, W, generator=g).to(torch.bfloat16 if dt == "bf16" else torch.float32)
    xd = x.to(cuda).contiguous(memory_format=torch.channels_last)
    out = ops.bias_grad_nhwc(xd)
    ref = x.double().sum((0, 2, 3))
    scale = x.double().abs().sum((0, 2, 3))
    assert out.dtype == torch.float32 and out.shape == (C,)
    assert ((out.cpu().double() - ref).abs() / scale).max().item() < 1e-5
    assert torch.equal(out, ops.bias_grad_nhwc(xd))
    assert torch.equal(out, ops.bias_grad_nhwc(x.to(cuda)))          # NCHW input: made channels-last by the wrapper


def test_conv_nhwc_function_matches_autocast_conv(cuda):
    """ops.ConvNHWCFn (image pyramid, bf16 channels-last branch) against nn.Conv2d under bf16 autocast: same MIOpen kernels,
    so outputs and data / weight gradients agree to bf16 rounding; the bias gradient agrees with the float64 sum."""
    from a3vt_amd import ops
    torch.manual_seed(3)
    conv = torch.nn.Conv2d(16, 32, 5, stride=2, padding=1).to(cuda).to(memory_format=torch.channels_last)
    x = torch.randn(6, 16, 40, 40, device=cuda).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    gy = torch.randn(6, 32, 19, 19, device=cuda).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    xa = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ya = conv(xa)
    ya.backward(gy)
    ref = (xa.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone())
    conv.zero_grad()
    xb = x.clone().requires_grad_(True)
    yb = ops.ConvNHWCFn.apply(xb, conv.weight, conv.bias, [2, 2], [1, 1])
    yb.backward(gy)
    assert yb.dtype == torch.bfloat16 and rel_err(yb.float(), ya.float()) < 1e-2
    assert rel_err(xb.grad.float(), ref[0].float()) < 1e-2
    assert conv.weight.grad.dtype == torch.float32 and rel_err(conv.weight.grad, ref[1]) < 1e-2
    exact = gy.double().sum((0, 2, 3))
    assert rel_err(conv.bias.grad.double(), exact) < 1e-5            # fp32 sum; torch's own is rounded to bf16
    assert rel_err(ref[2].double(), exact) < 1e-2


def test_posenc_wide_bf16_operand_mode(cuda):
    """gemm_bf16 = 1 of a3vt_posenc_wide_fwd/bwd (the bf16 configurations): products after the embedding layer on bf16-rounded
    operands, fp32 storage and accumulation; the embedding layer and its backward stay exact.  Against the exact path of the
    same call: features 1.6e-3 (tolerance 5e-3, the bf16 configurations' level on positions); gradients 2.1e-2 (parameters) and
    3.6e-2 (positions: random upstream gradient, i.e. full cancellation inside every 232- and 448-term sum, then the
    frequencies up to 18 pi of the embedding's derivative) — tolerance 6e-2; repeatable bit for bit."""
    from a3vt_amd import ops
    from a3vt_amd.pterotactyl.reconstruction.vision import model as vmodel
    I, B, N = 448, 2, 1949
    torch.manual_seed(5)
    pe, me = vmodel.Positional_Encoder(I).to(cuda), vmodel.Mask_Encoder(I).to(cuda)
    packed = torch.cat([p.reshape(-1) for p in pe.packed()] + [me.model[0].weight.reshape(-1)]).detach()
    g = torch.Generator().manual_seed(9)
    verts = ((torch.rand(B, N, 3, generator=g) - 0.5) * 0.6).to(cuda)
    mask = torch.randint(0, 4, (B, N, 1), generator=g).float().to(cuda)
    gout = torch.randn(B, N, I, generator=g).to(cuda)
    res = []
    for mode in (False, True, True):
        v, pk = verts.clone().requires_grad_(True), packed.clone().requires_grad_(True)
        f = ops.PosEncMaskFn.apply(v, mask, pk, I, I, mode)
        (f * gout).sum().backward()
        res.append((f.detach(), v.grad, pk.grad))
    exact, a, b = res
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], exact[0])                      # the flag does reach the products
    from helpers import rel_l2
    errs = [rel_l2(x, y) for x, y in zip(a, exact)]
    assert errs[0] < 5e-3 and max(errs[1:]) < 6e-2, errs


def test_image_encoder_bf16_branch_batches_1_to_4(cuda):   # (batches 1, 3 and 4: both sides of the threshold)
    """the bf16 channels-last image encoder at the batch sizes around MIOpen's BatchNorm defect (its bf16 NHWC
    training BatchNorm takes the host down below 4 samples).  With the library's own BatchNorm + ReLU (round 6, the default)
    every batch size runs the same kernels and nothing is reported; with ``fused_bn_relu = False`` the small batches take the
    NCHW kernel (``Image_Encoder.bn_nhwc_min_batch``) and say so once.  Every batch size trains, and the maps agree with the
    fp32 branch to bf16 rounding."""
    import warnings
    from a3vt_amd.pterotactyl.reconstruction.vision import model
    # (a three-block pyramid: every new convolution shape costs a MIOpen search)
    args16 = make_args(use_img=True, CNN_ker_size=5, num_CNN_blocks=3, layers_per_block=2, gemm_precision="bf16s")
    args32 = make_args(use_img=True, CNN_ker_size=5, num_CNN_blocks=3, layers_per_block=2)
    torch.manual_seed(0)
    enc16 = model.Image_Encoder(args16).to(cuda)
    enc32 = model.Image_Encoder(args32).to(cuda)
    enc32.load_state_dict(enc16.state_dict())
    g = torch.Generator().manual_seed(1)
    for fused, reports in ((True, 0), (False, 1)):
        model.Image_Encoder._bn_fallback_reported = False
        model.Image_Encoder.fused_bn_relu = fused
        try:
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                for B in (1, 3, 4):
                    img = torch.rand(B, 3, 256, 256, generator=g).to(cuda)
                    enc16.train(), enc32.train()
                    maps16 = enc16(img)
                    maps32 = enc32(img)
                    assert len(maps16) == len(maps32)
                    for a, b in zip(maps16, maps32):
                        assert a.shape == b.shape and torch.isfinite(a.float()).all()
                        assert ((a.float() - b).norm() / b.norm()).item() < 0.1, (fused, B)   # 16 bf16 convolutions + tiny-batch BatchNorm deep
                    sum(m.float().square().mean() for m in maps16).backward()
                    assert all(torch.isfinite(p.grad).all() for p in enc16.parameters() if p.grad is not None)
                    enc16.zero_grad()
        finally:
            model.Image_Encoder.fused_bn_relu = True
        assert sum("bn_nhwc_min_batch" in str(x.message) for x in w) == reports, fused      # reported once, by the MIOpen branch only


@pytest.mark.parametrize("library", [True, False])
def test_bf16_weight_copies_follow_the_fused_optimizer(cuda, library):
    """ops._bf16_copy caches the bf16 channels-last copy of a convolution weight per weight VERSION; the trainer's optimizer —
    the library's one-launch Adam (a3vt_amd/optim.py) or torch's fused Adam (``library_adam = False``) — writes the weights in
    place without moving ``_version``: the cache (and the direct convolution's weight images, ops._conv5_image) must see its updates."""
    from a3vt_amd import ops, optim as aopt
    w = torch.nn.Parameter(torch.randn(16, 16, 5, 5, device=cuda))
    opt = aopt.make_adam([w], 0.1, library=library)
    a = ops._bf16_copy(w, True)
    img = ops._conv5_image(w, 0)
    assert ops._bf16_copy(w, True) is a and ops._conv5_image(w, 0) is img
    w.grad = torch.ones_like(w)
    opt.step()
    assert getattr(opt, "library_steps", 0) == (1 if library else 0)
    b = ops._bf16_copy(w, True)
    img2 = ops._conv5_image(w, 0)
    assert b is not a and img2 is not img and not torch.equal(img, img2)
    assert torch.equal(b.float(), w.detach().to(torch.bfloat16).float()) and not torch.equal(a.float(), b.float())
