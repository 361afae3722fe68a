"""-m gpu: the bf16 STORAGE mode of the GCN stack (``gemm_precision = "bf16s"``, BASELINE configs[3]/[4]: activations,
gradients and weight images bf16 in HBM, fp32 accumulation, fp32 master weights).  It is a separately-toleranced mode,
never the headline: forward against the oracle's float64 emulation of exactly these roundings (``oracle.gcn.gcn(...,
bf16="storage")``) and against the exact fp32 network at the bf16 level; vertex positions of the full 20 x 300 network
within 5e-3 of the REFERENCE's fp32 positions (fixture g4; SURVEY App. B measured 1.4e-3 for bf16 rounding after every
layer); gradients against autograd of the emulation at the bf16 level.  That autograd rounds the GRADIENT wherever the
emulation rounds a value (dW through the bf16 weight, grad_feats through the bf16 input, each stored gradient), while the
device reduces dW and writes grad_feats in fp32: the gradient bound below is sized to that mismatch.
tests/test_gpu_bf16_exact.py holds the mode to an emulation that rounds where the kernels do."""
import numpy as np
import pytest
import torch

from golden_util import load
from helpers import make_args, oracle_adj, random_cloud, rel_err, rel_l2, template

pytestmark = pytest.mark.gpu


def _stack_case(cuda, tname, use_touch, L, H, B, I=50, cut=0.33, seed=3):
    from a3vt_amd import mesh as amesh, ops
    from oracle import gcn as og
    args = make_args(use_touch=use_touch, num_GCN_layers=L, hidden_GCN_size=H, num_grasps=1, cut=cut)
    verts, faces = template(tname)
    adj_o, _ = oracle_adj(verts, faces, args)
    n = adj_o[0].numel() - 1
    st = og.init_state(I, H, L, seed=seed)
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(B, n, I, generator=g) * 0.5
    gup = torch.randn(B, n, 3, generator=g)
    st64 = {k: v.double().requires_grad_(True) for k, v in st.items() if k.startswith("mesh_deform_1")}
    f64 = feats.double().requires_grad_(True)
    adj64 = (adj_o[0], adj_o[1], adj_o[2].double())
    with torch.no_grad():
        out_fp32 = og.gcn(feats.double(), {k: v.detach() for k, v in st64.items()}, "mesh_deform_1", adj64, L, cut)
    out_emul = og.gcn(f64, st64, "mesh_deform_1", adj64, L, cut, bf16="storage")
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
    ld = (I + 3) // 4 * 4
    fd = torch.nn.functional.pad(feats, (0, ld - I)).to(cuda).requires_grad_(True)
    out = ops.gcn_stack(fd, adj, I, H, round(H * cut), ws, bs, bf16="bf16s")
    (out * gup.to(cuda)).sum().backward()
    errs = {"out_vs_emul_max": rel_err(out, out_emul), "out_vs_emul_l2": rel_l2(out, out_emul),
            "out_vs_fp32_l2": rel_l2(out, out_fp32), "gfeats": rel_l2(fd.grad[..., :I], f64.grad)}
    for i in range(L):
        errs[f"dW{i}"] = rel_l2(ws[i].grad, st64[f"mesh_deform_1.layers.{i}.weight"].grad)
        errs[f"db{i}"] = rel_l2(bs[i].grad, st64[f"mesh_deform_1.layers.{i}.bias"].grad)
    assert fd.grad[..., I:].abs().max().item() == 0.0 if ld > I else True
    # a second evaluation reproduces every bit (deterministic kernels)
    ws2 = [w.detach().clone().requires_grad_(True) for w in ws]
    fd2 = fd.detach().clone().requires_grad_(True)
    out2 = ops.gcn_stack(fd2, adj, I, H, round(H * cut), ws2, [b.detach() for b in bs], bf16="bf16s")
    (out2 * gup.to(cuda)).sum().backward()
    assert torch.equal(out, out2) and torch.equal(fd.grad, fd2.grad) and all(torch.equal(a.grad, b.grad) for a, b in zip(ws, ws2))
    return errs


@pytest.mark.parametrize("tname,use_touch,L,H,B,I,cut", [
    ("ico2", False, 3, 300, 3, 50, 0.33),       # small mesh: few-row launch paths (column blocks)
    ("atlas", True, 6, 300, 2, 50, 0.33),       # fused touch graph: hub rows through csr16_heavy_kernel
    ("ico4", False, 3, 300, 13, 50, 0.33),      # 33306 rows: main + remainder split of the MFMA launch, ragged dW units
    ("ico3", False, 4, 64, 5, 50, 0.5),         # narrow hidden, another cut
    ("ico3", False, 3, 300, 2, 448, 0.33),      # the image model's 448-wide input: dW in two column windows
    ("ico2", False, 3, 128, 4, 50, 0.0),        # cut 0: nothing aggregated
    ("ico4", False, 3, 300, 3, 50, 0.33),       # 7686 rows: the register-resident product (gcn_gemm16.hip), one block per workgroup
    ("atlas", True, 3, 300, 8, 50, 0.33),       # the same on the fused touch graph (15592 rows, ragged last block)
    ("ico4", False, 3, 296, 4, 50, 0.25),       # 296 columns: 37 store groups, K short of the last k-step, another cut
    ("ico4", False, 4, 304, 5, 50, 0.0),        # widest hidden size, nothing aggregated (no raw-output stores)
])
def test_gcn_stack_bf16_storage(cuda, tname, use_touch, L, H, B, I, cut):
    e = _stack_case(cuda, tname, use_touch, L, H, B, I, cut)
    # forward: same roundings as the emulation (a value within fp32 rounding of a bf16 tie may round the other way: 2^-8
    # of one activation) -> close in L2; bf16 level against the exact network
    # Tolerances = 2.5x the worst case measured over these ten configurations (round 3: 2.4e-4 / 6.5e-4 against the emulation,
    # 3.0e-3 against the exact network, 8.1e-3 on a gradient — the deep touch-graph case); the kernels are deterministic, so the
    # figures do not move from box to box.  (Round 2 asserted 3e-3 / 2e-2 / 3e-2 / 5e-2.)
    assert e["out_vs_emul_l2"] < 6e-4 and e["out_vs_emul_max"] < 2e-3, e
    assert e["out_vs_fp32_l2"] < 7.5e-3, e
    grads = {k: v for k, v in e.items() if k[0] in "gd"}
    assert max(grads.values()) < 2e-2, e


def test_g4_full_size_forward_bf16_storage(cuda):
    """Full 20 x 300 network, three stages, seed-0 reference init: positions within 5e-3 of the reference's fp32 output."""
    from a3vt_amd.pterotactyl.reconstruction.vision import model
    from a3vt_amd.pterotactyl.utility import utils
    z = load("g4_full_forward.npz")
    args = make_args(gemm_precision="bf16s")
    info, verts = utils.load_mesh_vision(args, "vision_charts")
    torch.manual_seed(0)
    net = model.Deformation(info, verts, args).to(cuda)
    charts = {"vision_charts": torch.from_numpy(z["verts_in"]).to(cuda), "vision_masks": 3 * torch.ones(2, 1824, 1, device=cuda)}
    with torch.no_grad():
        out, _ = net(torch.zeros(2, 1), charts)
    err = rel_err(out, torch.from_numpy(z["verts_out"]))
    assert 1e-5 < err < 5e-3, err
    out_t, _ = net(torch.zeros(2, 1), charts)                 # the stash-writing forward gives the same positions
    assert torch.equal(out, out_t.detach())


def test_training_step_bf16_storage_fullsize(cuda):
    """configs[1] sizes in the bf16 storage mode: finite, the whole step reproduces bit for bit, and the loss / weight
    gradients agree with the fp32 step on the same inputs at the bf16 level."""
    from a3vt_amd.pterotactyl.reconstruction.vision import model
    from a3vt_amd.pterotactyl.utility import utils
    v, f = template("ico4")
    vt, ft = torch.from_numpy(v).to(cuda), torch.from_numpy(f).to(cuda)
    B, P = 64, 10000
    gt = random_cloud(B, P, 3).to(cuda)
    g = torch.Generator().manual_seed(1)
    samples = (torch.randint(0, f.shape[0], (3, B, P), generator=g).to(torch.int32).to(cuda),
               torch.rand(3, B, P, generator=g).to(cuda), torch.rand(3, B, P, generator=g).to(cuda))
    res = {}
    for prec in ("fp32", "bf16s", "bf16s"):
        args = make_args(gemm_precision=prec)
        info = utils.adj_init(vt, ft, args)
        torch.manual_seed(0)
        net = model.Deformation(info, vt, args).to(cuda)
        charts = model.prepare_mesh({"img": torch.zeros(B, 1)}, vt, args)
        out = net(torch.zeros(B, 1), charts)[0]
        loss = 9000.0 * utils.chamfer_distance(out, info["faces"], gt, num=P, samples=samples).mean()
        loss.backward()
        grads = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
        assert torch.isfinite(grads).all() and torch.isfinite(out).all()
        res.setdefault(prec, []).append((out.detach(), loss.item(), grads))
    a, b = res["bf16s"]
    assert torch.equal(a[0], b[0]) and a[1] == b[1] and torch.equal(a[2], b[2])
    ref = res["fp32"][0]
    assert rel_err(a[0], ref[0]) < 5e-3 and abs(a[1] - ref[1]) < 2e-2 * abs(ref[1])
    assert rel_l2(a[2], ref[2]) < 0.15                         # whole-network gradient, 60 bf16-rounded layers deep


@pytest.mark.parametrize("tname,B,spatial", [("ico4", 6, True), ("ico5", 2, True), ("atlas", 8, True), ("ico4", 5, False)])
def test_tiled_aggregation_is_the_row_walk_bit_for_bit(cuda, tname, B, spatial):
    """Round 6: on graphs of degree <= 8 the bf16 stacks aggregate from LDS tiles (csr16t_*, gcn_bf16s.hip: tile + halo rows
    staged once, neighbour sums in CSR order) instead of gathering every neighbour row from L2.  Same sums in the same order:
    outputs, feature and weight gradients equal the row walk's bit for bit (``dbg_csr_algo("rows")``); the bias gradients are
    sums over the rows in another grouping (fp32, 1e-5).  ``spatial=False``: icosphere vertices in subdivision order — every
    tile's halo exceeds the plan's bound, and the tiles walk their rows inside the same kernel."""
    from a3vt_amd import mesh as amesh, ops
    from oracle import gcn as og
    L, H, I, cut = 3, 300, 50, 0.33
    if tname.startswith("ico"):
        verts, faces = amesh.icosphere(int(tname[3:]), spatial_order=spatial)
    else:
        verts, faces = template(tname)
    n = verts.shape[0]
    adj = ops.DeviceCSR(amesh.CSRAdjacency.from_pairs(*amesh.vision_pairs(faces, n), n), cuda)
    st = og.init_state(I, H, L, seed=4)
    g = torch.Generator().manual_seed(21)
    feats = torch.nn.functional.pad(torch.randn(B, n, I, generator=g) * 0.5, (0, 2)).to(cuda)
    gup = torch.randn(B, n, 3, generator=g).to(cuda)
    res = {}
    try:
        for algo in ("rows", "auto"):
            ops.dbg_csr_algo(algo)
            ops.path_counts(reset=True)
            ws = [st[f"mesh_deform_1.layers.{i}.weight"].to(cuda).requires_grad_(True) for i in range(L)]
            bs = [st[f"mesh_deform_1.layers.{i}.bias"].to(cuda).requires_grad_(True) for i in range(L)]
            fd = feats.clone().requires_grad_(True)
            out = ops.gcn_stack(fd, adj, I, H, round(H * cut), ws, bs, bf16="bf16s")
            (out * gup).sum().backward()
            res[algo] = (out.detach(), fd.grad, [w.grad for w in ws], [b.grad for b in bs], ops.path_counts()["csr16_tiles"])
    finally:
        ops.dbg_csr_algo("auto")
    r, t = res["rows"], res["auto"]
    assert r[4] == 0 and t[4] == L - 1, (r[4], t[4])
    assert torch.equal(r[0], t[0]) and torch.equal(r[1], t[1])
    for a, b in zip(r[2], t[2]):
        assert torch.equal(a, b)
    for a, b in zip(r[3], t[3]):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5 * float(a.abs().max()))
