"""-m gpu: the GCN stack's bf16 gemm modes (1 "bf16": bf16 operands, fp32 storage; 2 "bf16s": bf16 storage) against the
oracle's rounding-exact float64 emulation (``oracle.gcn.bf16_stack_forward`` / ``bf16_stack_backward``: the roundings
written out where the kernels round, on values only — tests/test_oracle_bf16_emulation.py anchors it on the CPU).

The checks are TEACHER-FORCED: every layer is recomputed from the activations the device itself stashed for its backward
(``out.grad_fn.acts``), so a layer's check sees its own fp32-versus-float64 differences only, not the rounding ties that
compound up a bf16 stack from the layers below.  Then the bounds can be tight enough to see one wrong row or column group:
a dropped 8-row block of a 33 306-row dW reduction moves dW by ~1.5 %, far above them.

Stash layout (csrc/capi.hip, StackStash / stack_stash; stated here independently): mode 2 — hidden layer i as [M][pad8(hidden)] bf16
at element i * M * pad8(hidden), the stack's input converted to bf16 behind them as [M][pad8(in_features)]; mode 1 — hidden
layer i as [M][hidden] fp32 at float i * M * hidden (never hybrid rows: the channel-sliced path is fp32-only).
"""
import ctypes

import pytest
import torch

from helpers import template

pytestmark = pytest.mark.gpu


def _pad8(n):
    return (n + 7) // 8 * 8


def _graph(cuda, tname, use_touch):
    from a3vt_amd import mesh as amesh, ops
    verts, faces = template(tname)
    if use_touch:
        _, sf = amesh.load_asset("touch_chart")
        r, c, n, _ = amesh.fused_pairs(verts, faces, sf, 1, False)
    else:
        r, c = amesh.vision_pairs(faces, verts.shape[0])
        n = verts.shape[0]
    host = amesh.CSRAdjacency.from_pairs(r, c, n)
    adj = ops.DeviceCSR(host, cuda)
    # the emulation aggregates with the device's own fp32 coefficients, in float64, on the GPU
    emul = (torch.from_numpy(host.rowptr).long().to(cuda), torch.from_numpy(host.col).long().to(cuda),
            torch.from_numpy(host.val).double().to(cuda))
    return adj, emul, n


def _inputs(cuda, n, B, L, H, I, seed=3):
    from oracle import gcn as og
    st = og.init_state(I, H, L, seed=seed)
    ws = [st[f"mesh_deform_1.layers.{i}.weight"].to(cuda) for i in range(L)]
    bs = [st[f"mesh_deform_1.layers.{i}.bias"].to(cuda) for i in range(L)]
    g = torch.Generator().manual_seed(11 + seed)
    feats = torch.randn(B, n, I, generator=g) * 0.5
    gup = torch.randn(B, n, 3, generator=g).to(cuda)
    ld = (I + 3) // 4 * 4
    return torch.nn.functional.pad(feats, (0, ld - I)).to(cuda), ws, bs, gup


def _run(adj, feats, I, H, cl, ws, bs, gup, mode):
    """One forward + backward through ops.gcn_stack.  Returns the output, a copy of the stash (the backward drops it) and
    the gradients."""
    from a3vt_amd import ops
    fd = feats.clone().requires_grad_(True)
    wl = [w.clone().requires_grad_(True) for w in ws]
    bl = [b.clone().requires_grad_(True) for b in bs]
    out = ops.gcn_stack(fd, adj, I, H, cl, wl, bl, bf16=mode)
    stash = out.grad_fn.acts.clone()
    (out * gup).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), stash, fd.grad, [w.grad for w in wl], [b.grad for b in bl]


def _stash_acts(stash, mode, L, B, n, H, I):
    """Inputs of layers 0 .. L-1 as the device stored them, as float64 (with the padding columns, for the checks)."""
    m = B * n
    if mode == "bf16s":
        ldh, ld0 = _pad8(H), _pad8(I)
        h = stash.view(torch.int16).view(torch.bfloat16)
        hid = h[:(L - 1) * m * ldh].view(L - 1, B, n, ldh)
        x0 = h[(L - 1) * m * ldh:(L - 1) * m * ldh + m * ld0].view(B, n, ld0)
        return [x0] + [hid[i] for i in range(L - 1)]
    f = stash.view(torch.float32)
    hid = f[:(L - 1) * m * H].view(L - 1, B, n, H)
    return [None] + [hid[i] for i in range(L - 1)]


def _ulp(v):
    """One bf16 unit in the last place at |v| (8 significant bits), float64."""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), e - 8)


def _rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _elementwise(a, b, tol=1e-3):
    """Fraction of the elements further than tol * max|b| from b (the outlier accounting of helpers.assert_grad_close)."""
    a, b = a.double(), b.double()
    return ((a - b).abs() > tol * b.abs().max().clamp_min(1e-300)).double().mean().item()


def _forward_layer_bound(x, w, b, y_emul, adjE, cl, mode):
    """Per-element bound on |device - emulation| for one teacher-forced hidden layer: one bf16 ulp of the output (mode 2:
    fp32 and float64 sums on either side of a rounding tie), plus the fp32 summation error of the K-term product, carried
    through the aggregation together with a one-ulp tie of each aggregated raw value (mode 2).  None of it is large
    enough to hide a wrong term: ~1e-5 of |X||W| against values of the order of |X||W| / sqrt(K)."""
    from oracle import gcn as og
    K = x.shape[-1]
    wm = og.bf16_round(w[0].double())
    s = torch.matmul(og.bf16_round(x).abs(), wm.abs())
    acc = K * 2.0 ** -24 * s
    tol = acc.clone()
    if cl:
        z = torch.matmul(og.bf16_round(x), wm)[..., :cl]
        absA = (adjE[0], adjE[1], adjE[2].abs())
        za_err = acc[..., :cl] + (_ulp(z) + 1e-300 if mode == "bf16s" else 0.0)
        tol[..., :cl] = og.adj_matmul(absA, za_err) + 2.0 ** -20 * (og.adj_matmul(absA, z.abs()) + b[:cl].double().abs())
    if mode == "bf16s":
        tol = tol + _ulp(y_emul.abs() + tol)
    else:
        tol = tol + 2.0 ** -23 * y_emul.abs()
    return tol


def _check_case(cuda, tname, use_touch, B, L, H, I, cl, mode, algo="auto"):
    from a3vt_amd import ops
    from oracle import gcn as og
    adj, adjE, n = _graph(cuda, tname, use_touch)
    feats, ws, bs, gup = _inputs(cuda, n, B, L, H, I)
    m = B * n
    ops.dbg_csr_algo(algo)
    try:
        ops.path_counts(reset=True)
        out, stash, gf, dws, dbs = _run(adj, feats, I, H, cl, ws, bs, gup, mode)
        paths = ops.path_counts()
        # determinism: a second evaluation reproduces every bit, the stored activations included (not the stash's slack)
        out2, stash2, gf2, dws2, dbs2 = _run(adj, feats, I, H, cl, ws, bs, gup, mode)
    finally:
        ops.dbg_csr_algo("auto")
    acts = _stash_acts(stash, mode, L, B, n, H, I)
    acts2 = _stash_acts(stash2, mode, L, B, n, H, I)
    assert torch.equal(out, out2) and torch.equal(gf, gf2)
    assert all(a is None or torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a, b.view(torch.int16) if b.dtype == torch.bfloat16 else b) for a, b in zip(acts, acts2))
    assert all(torch.equal(a, b) for a, b in zip(dws + dbs, dws2 + dbs2))
    assert torch.isfinite(out).all() and torch.isfinite(gf).all()

    rep = {"m": m}
    if mode == "bf16s":
        # the stored input is r(feats) bit for bit, its padding columns zero
        x0 = acts[0]
        assert torch.equal(x0[..., :I].view(torch.int16), feats[..., :I].to(torch.bfloat16).view(torch.int16))
        assert (x0[..., I:].view(torch.int16) == 0).all()
        xs = [x0[..., :I].double()] + [a[..., :H].double() for a in acts[1:]]
        for a in acts[1:]:
            assert (a[..., H:].view(torch.int16) == 0).all()        # padding columns of every hidden layer: exactly 0
    else:
        xs = [feats[..., :I].double()] + [a.double() for a in acts[1:]]

    # ---- forward, per layer, from the device's own input to that layer
    worst_frac = 0.0
    for i in range(L - 1):
        ye = og.bf16_hidden_layer(xs[i], ws[i].double(), bs[i].double(), adjE, cl, 1 if mode == "bf16" else 2)
        yd = xs[i + 1]
        d = (yd - ye).abs()
        tol = _forward_layer_bound(xs[i], ws[i], bs[i], ye, adjE, cl, mode)
        bad = d > tol
        rep[f"fwd_bad{i}"] = int(bad.sum())
        if bad.any():
            print("layer", i, "outside the bound:", d[bad][:5].tolist(), tol[bad][:5].tolist())
        if mode == "bf16s":
            # and hardly any element differs at all: a rounding tie decided by the fp32 sum (RNE = RNE, not truncation)
            frac = (d > 0).double().mean().item()
            worst_frac = max(worst_frac, frac)
        else:
            rep[f"fwd{i}"] = (d.max() / ye.abs().max()).item()
    rep["tie_frac"] = worst_frac
    # output layer on the device's last stash: fp32 level
    ue = og.bf16_output_layer(xs[L - 1], ws[L - 1].double(), bs[L - 1].double(), adjE)
    rep["out"] = ((out.double() - ue).abs().max() / ue.abs().max()).item()

    # ---- backward from the device's stash and the same grad_update
    mnum = 1 if mode == "bf16" else 2
    ge, dwe, dbe = og.bf16_stack_backward(xs, [w.double() for w in ws], adjE, cl, mnum, gup.double())
    assert (gf[..., I:] == 0).all()                              # grad_feats padding columns
    rep["gfeats"] = _rel_l2(gf[..., :I], ge)
    rep["gfeats_el"] = _elementwise(gf[..., :I], ge)
    for i in range(L):
        rep[f"dW{i}"] = _rel_l2(dws[i], dwe[i])
        rep[f"dW{i}_el"] = _elementwise(dws[i], dwe[i])
        if i < L - 1:
            assert (dbs[i][cl:] == 0).all(), i                   # dead bias channels (model.py:358): exact zeros
        rep[f"db{i}"] = _rel_l2(dbs[i], dbe[i]) if cl or i == L - 1 else 0.0
        rep[f"db{i}_el"] = _elementwise(dbs[i], dbe[i]) if cl or i == L - 1 else 0.0
    print(tname, B, L, H, I, cl, mode, algo, {k: (f"{v:.2e}" if isinstance(v, float) else v) for k, v in rep.items()})
    # every element of every hidden layer within the per-element bound of the emulation
    assert all(v == 0 for k, v in rep.items() if k.startswith("fwd_bad")), rep
    return rep, paths, adj


def _grad_worst(rep, suffix=""):
    return max(v for k, v in rep.items() if k[:2] in ("gf", "dW", "db") and k.endswith("_el") == (suffix == "_el"))


# case: (graph, touch, B, L, hidden, in_features, cut_len, algo) — each row pins what the comment says
CASES16 = [
    ("ico1", False, 1, 3, 16, 20, 5, "auto"),      # few rows (column-block launches); minimum hidden; cut_len 5 (cpad 8)
    ("ico2", False, 3, 3, 20, 51, 1, "auto"),      # hidden 20 (pad8 = 24: padding columns), in_features 51 (pad8 56), cut_len 1
    ("ico4", False, 3, 3, 300, 50, 99, "auto"),    # 7 686 rows: the register-resident product (gcn_gemm16.hip)
    ("ico4", False, 13, 3, 300, 50, 99, "auto"),   # 33 306 rows: main + remainder split, ragged dw16 units
    ("ico5", False, 4, 3, 304, 600, 0, "auto"),    # 40 968 rows; widest hidden, cut 0; dW_0 in windows 304 + 296
    ("atlas", True, 2, 3, 300, 50, 99, "auto"),    # fused touch graph: hub rows (csr16_heavy) and the split output layer
    ("ico3", False, 2, 3, 296, 448, 74, "auto"),   # 37 store groups; dW_0 windows 304 + 144; cut 0.25
    ("ico4", False, 3, 3, 300, 50, 99, "rows"),    # the same on the row-walk aggregation instead of the LDS-tiled one (csr16t)
    ("ico2", False, 2, 4, 64, 50, 64, "auto"),     # cut_len = hidden: every channel aggregated
    ("ico3", False, 2, 4, 128, 50, 7, "auto"),     # cut_len 7 (cpad 8), four layers
]


@pytest.mark.parametrize("tname,use_touch,B,L,H,I,cl,algo", CASES16)
def test_bf16_storage_stack_against_exact_emulation(cuda, tname, use_touch, B, L, H, I, cl, algo):
    rep, paths, adj = _check_case(cuda, tname, use_touch, B, L, H, I, cl, "bf16s", algo)
    # launch paths the case claims
    if (tname, B) == ("ico4", 3):
        assert paths["rowgemm16"] > 0, paths
        assert paths["csr16_tiles"] == (L - 1 if algo == "auto" else 0), paths
    if B >= 4:
        assert rep["m"] > 32768
    if use_touch:       # hub rows (the heavy-row workgroups of csr16), and the output layer through the split
        assert adj.max_degree > 64 and adj.split is not None and paths["csr16_tiles"] == 0, paths
    # forward: hardly any element differs from the emulation at all (measured on MI355X: <= 5.5e-5 of the elements, each by
    # one ulp); every element within the per-element bound (asserted in _check_case)
    assert rep["tie_frac"] < 2e-4, rep
    # output layer, fp32 level on the device's last stash (measured: <= 1.6e-7)
    assert rep["out"] < 5e-7, rep
    # gradients, rel L2 and elementwise outliers (> 1e-3 of max).  Measured: <= 6.1e-4 / 1.1e-4 with M * hidden >= 9 720.
    # The backward is teacher-forced at its input only: G, dZa and the next G are bf16 roundings of fp32 sums that the
    # emulation takes in float64, so ~4e-5 of them land on the other side of a tie (one ulp, 2^-8 relative) at every
    # rounding point and the differences grow ~3x per layer down the chain (dW2 2e-7, dW1 1.8e-4, dW0 6.1e-4 on ico4).
    # On the two small matrices (ico1: 42 x 16, ico2 cut_len = hidden: 324 x 64, four layers) one such tie is a sizeable
    # part of the whole tensor: measured 1.1e-3 / 1.5e-3 rel L2, 2.8e-2 / 1.2e-2 outliers; bounded at 4e-3 / 5e-2.
    small = rep["m"] * H < 25000
    assert _grad_worst(rep) < (4e-3 if small else 1e-3), rep
    assert _grad_worst(rep, "_el") <= (5e-2 if small else 1e-3), rep


CASES1 = [
    ("ico1", False, 1, 3, 16, 20, 5),       # few rows, minimum hidden, cut_len 5
    ("ico2", False, 3, 3, 20, 51, 1),       # hidden and in_features not multiples of 8, cut_len 1
    ("ico4", False, 13, 3, 300, 50, 99),    # 33 306 rows: main + remainder split
    ("atlas", True, 2, 3, 300, 50, 99),     # fused touch graph: hub rows, the split output layer
    ("ico3", False, 2, 3, 304, 600, 0),     # widest hidden (dW_1 over 304 inputs in one pass), cut 0; dW_0 through the
                                            # column panels (300 + 300)
    ("ico3", False, 2, 3, 296, 448, 74),    # panels 300 + 148
    ("ico2", False, 2, 4, 64, 50, 64),      # cut_len = hidden
    ("ico2", False, 2, 8, 300, 50, 99),     # deep stack: eight layers
]


@pytest.mark.parametrize("tname,use_touch,B,L,H,I,cl", CASES1)
def test_bf16_operand_stack_against_exact_emulation(cuda, tname, use_touch, B, L, H, I, cl):
    rep, paths, adj = _check_case(cuda, tname, use_touch, B, L, H, I, cl, "bf16")
    if use_touch:
        assert adj.max_degree > 64 and adj.split is not None
    assert paths["stack_rows"] == 1 and paths["stack_quad"] == 0, paths   # mode 1 keeps the row-walk aggregation
    # forward, teacher-forced: fp32 level (measured: <= 4.0e-7 per layer, 1.4e-7 output)
    assert max(v for k, v in rep.items() if k.startswith("fwd") and not k.startswith("fwd_bad")) < 1.2e-6, rep
    assert rep["out"] < 5e-7, rep
    # gradients, rel L2 and elementwise outliers.  Measured (three layers): <= 8.3e-5, no outliers.  Before the fix of the
    # stack's dW column blocks, hidden = 304 gave 6e-2 (rows 300..303 of dW_1 were X's columns 0..3 times dZ).
    # The eight-layer stack: dZ is rounded to bf16 as an operand at each of seven layers, from an fp32 gradient chain the
    # emulation carries in float64; ~1e-4 of those roundings go the other way per layer and compound down the chain
    # (dW6 3e-7 ... dW0 6.9e-4, grad_feats 7.2e-4, 2.8e-3 outliers): bounded at 2e-3 / 1e-2.
    deep = L > 4
    assert _grad_worst(rep) < (2e-3 if deep else 1e-4), rep
    assert _grad_worst(rep, "_el") <= (1e-2 if deep else 1e-3), rep


@pytest.mark.parametrize("mode,cl", [("bf16", 21), ("bf16s", 21), ("bf16s", 0)])
def test_bf16_stack_backward_accumulates(cuda, mode, cl):
    """a3vt_gcn_stack_bwd_acc with accumulate = 1 (the trainer's gradient bucket: mesh_deform_2 serves two stages) adds to
    pre-filled weight / bias gradients exactly what accumulate = 0 writes; grad_feats is written, not accumulated."""
    from a3vt_amd import lib as _lib, ops
    L, H, I, B = 3, 64, 50, 2
    adj, _, n = _graph(cuda, "ico2", False)
    feats, ws, bs, gup = _inputs(cuda, n, B, L, H, I, seed=4)
    fd = feats.clone().requires_grad_(True)
    wl = [w.clone().requires_grad_(True) for w in ws]
    bl = [b.clone().requires_grad_(True) for b in bs]
    out = ops.gcn_stack(fd, adj, I, H, cl, wl, bl, bf16=mode)
    ctx = out.grad_fn
    g = torch.Generator().manual_seed(9)
    pre_w = [torch.randn(w.shape, generator=g).to(cuda) for w in ws]
    pre_b = [torch.randn(b.shape, generator=g).to(cuda) for b in bs]
    gw, gb = [p.clone() for p in pre_w], [p.clone() for p in pre_b]
    gfeats = torch.full_like(feats, 7.0)
    Lb = _lib.load()
    scratch = ops.workspace("gcn", Lb.a3vt_gcn_stack_scratch_bytes_mode(B, n, I, H, L, cl, 1, ops.gemm_mode(mode)), cuda)
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    _lib.check(Lb.a3vt_gcn_stack_bwd_acc(
        _lib.ptr(feats), feats.shape[-1], I, arr(ws), arr(bs), L, H, cl, _lib.ptr(adj.rowptr), _lib.ptr(adj.col),
        _lib.ptr(adj.val), _lib.ptr(adj.t_rowptr), _lib.ptr(adj.t_col), _lib.ptr(adj.t_val),
        max(adj.max_degree, adj.t_max_degree), n, B, ops.gemm_mode(mode), _lib.ptr(ctx.acts), _lib.ptr(ctx.masks),
        _lib.ptr(gup), arr(gw), arr(gb), _lib.ptr(gfeats), _lib.ptr(scratch), 1, torch.cuda.current_stream().cuda_stream),
        "gcn_stack_bwd_acc")
    (out * gup).sum().backward()                                  # accumulate = 0 through autograd
    torch.cuda.synchronize()
    assert torch.equal(gfeats, fd.grad)
    for i in range(L):
        assert torch.equal(gw[i], pre_w[i] + wl[i].grad), i
        assert torch.equal(gb[i], pre_b[i] + bl[i].grad), i
