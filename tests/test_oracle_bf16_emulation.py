"""CPU: anchors for the oracle's rounding-exact emulation of the stack's bf16 gemm modes (``oracle.gcn.bf16_stack_forward`` /
``bf16_stack_backward``), which the GPU tests of tests/test_gpu_bf16_exact.py hold the kernels to.

1. With the rounding switched off (the identity) the explicit forward and backward are the exact network: they equal
   ``oracle.gcn.gcn`` and its float64 autograd gradients to ~1e-12, on an icosphere and on the fused vision + touch graph.
2. With the rounding on they equal a naive per-element restatement (Python loops over rows, channels and edges, a bf16
   round-to-nearest-even written out on the bit pattern) on a tiny case.
"""
import struct

import numpy as np
import pytest
import torch

from a3vt_amd import mesh as amesh
from helpers import template
from oracle import gcn as og


def _adj(tname, use_touch):
    verts, faces = template(tname)
    if use_touch:
        _, sf = amesh.load_asset("touch_chart")
        r, c, n, _ = amesh.fused_pairs(verts, faces, sf, 1, False)
    else:
        r, c = amesh.vision_pairs(faces, verts.shape[0])
        n = verts.shape[0]
    h = amesh.CSRAdjacency.from_pairs(r, c, n)
    return (torch.from_numpy(h.rowptr.astype(np.int64)), torch.from_numpy(h.col.astype(np.int64)),
            torch.from_numpy(h.val).double()), n


def _params(I, H, L, seed):
    st = og.init_state(I, H, L, seed=seed, dtype=torch.float64)
    ws = [st[f"mesh_deform_1.layers.{i}.weight"] for i in range(L)]
    bs = [st[f"mesh_deform_1.layers.{i}.bias"] for i in range(L)]
    return st, ws, bs


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("cut", [0.33, 0.0])
@pytest.mark.parametrize("tname,use_touch,B,H,I", [("ico2", False, 2, 24, 20), ("atlas", True, 1, 16, 12)])
def test_unrounded_emulation_is_the_exact_network(mode, cut, tname, use_touch, B, H, I):
    L = 3
    adj, n = _adj(tname, use_touch)
    st, ws, bs = _params(I, H, L, seed=7)
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(B, n, I, generator=g, dtype=torch.float64) * 0.5
    gup = torch.randn(B, n, 3, generator=g, dtype=torch.float64)
    leaf = {k: v.clone().requires_grad_(True) for k, v in st.items() if k.startswith("mesh_deform_1")}
    f = feats.clone().requires_grad_(True)
    out = og.gcn(f, leaf, "mesh_deform_1", adj, L, cut)
    (out * gup).sum().backward()
    c = og.cut_length(H, cut)
    acts, upd = og.bf16_stack_forward(feats, ws, bs, adj, c, mode, rnd=lambda t: t)
    assert _rel(upd, out.detach()) < 1e-12
    gf, dws, dbs = og.bf16_stack_backward(acts, ws, adj, c, mode, gup, rnd=lambda t: t)
    assert _rel(gf, f.grad) < 1e-12
    for i in range(L):
        assert _rel(dws[i], leaf[f"mesh_deform_1.layers.{i}.weight"].grad) < 1e-12, i
        assert _rel(dbs[i], leaf[f"mesh_deform_1.layers.{i}.bias"].grad) < 1e-12, i
        assert dws[i].shape == ws[i].shape and dbs[i].shape == bs[i].shape


# ---- naive restatement ------------------------------------------------------------------------------------------------

def _r(v):
    """bf16 round-to-nearest-even of a Python float, as the device does it to an fp32 value: to fp32 first, then the low
    16 bits of the pattern rounded away."""
    u = struct.unpack("<I", struct.pack("<f", v))[0]
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return struct.unpack("<f", struct.pack("<I", u))[0]


def _naive(feats, ws, bs, rowptr, col, val, c, gup):
    """Mode 2 forward and backward of one mesh with loops (lists of Python floats)."""
    n, I = len(feats), len(feats[0])
    L = len(ws)
    H = len(ws[0][0])
    W = [[[_r(ws[i][k][j]) for j in range(len(ws[i][k]))] for k in range(len(ws[i]))] for i in range(L - 1)]
    edges = [[(col[e], val[e]) for e in range(rowptr[v], rowptr[v + 1])] for v in range(n)]
    x = [[_r(feats[v][k]) for k in range(I)] for v in range(n)]
    acts = [x]
    for i in range(L - 1):
        K = len(x[0])
        z = [[sum(x[v][k] * W[i][k][j] for k in range(K)) for j in range(H)] for v in range(n)]
        za = [[_r(z[v][j]) for j in range(c)] for v in range(n)]
        y = [[0.0] * H for _ in range(n)]
        for v in range(n):
            for j in range(H):
                pre = sum(w * za[u][j] for u, w in edges[v]) + bs[i][j] if j < c else z[v][j]
                y[v][j] = _r(max(pre, 0.0))
        x = y
        acts.append(x)
    wl = ws[L - 1]
    z3 = [[sum(x[v][k] * wl[k][j] for k in range(H)) for j in range(3)] for v in range(n)]
    upd = [[sum(w * z3[u][j] for u, w in edges[v]) + bs[L - 1][j] for j in range(3)] for v in range(n)]
    # backward
    dz3 = [[0.0] * 3 for _ in range(n)]
    for v in range(n):
        for u, w in edges[v]:
            for j in range(3):
                dz3[u][j] += w * gup[v][j]
    dws, dbs = [None] * L, [None] * L
    dws[L - 1] = [[sum(x[v][k] * dz3[v][j] for v in range(n)) for j in range(3)] for k in range(H)]
    dbs[L - 1] = [sum(gup[v][j] for v in range(n)) for j in range(3)]
    g = [[_r(sum(dz3[v][t] * wl[k][t] for t in range(3))) if x[v][k] > 0 else 0.0 for k in range(H)] for v in range(n)]
    for i in range(L - 2, -1, -1):
        at = [[0.0] * c for _ in range(n)]
        for v in range(n):
            for u, w in edges[v]:
                for j in range(c):
                    at[u][j] += w * g[v][j]
        dz = [[_r(at[v][j]) if j < c else g[v][j] for j in range(H)] for v in range(n)]
        dbs[i] = [sum(g[v][j] for v in range(n)) if j < c else 0.0 for j in range(H)]
        xi = acts[i]
        K = len(xi[0])
        dws[i] = [[sum(xi[v][k] * dz[v][j] for v in range(n)) for j in range(H)] for k in range(K)]
        dx = [[sum(dz[v][j] * W[i][k][j] for j in range(H)) for k in range(K)] for v in range(n)]
        g = [[_r(dx[v][k]) if xi[v][k] > 0 else 0.0 for k in range(K)] for v in range(n)] if i > 0 else dx
    return acts, upd, g, dws, dbs


def test_rounded_emulation_matches_a_naive_loop():
    """ico1 (42 vertices), B = 1, H = 16, I = 20, L = 3, cut 0.33 (5 aggregated channels): every activation, the output and
    every gradient of the mode-2 emulation against the loop, to float64 summation order."""
    L, H, I = 3, 16, 20
    adj, n = _adj("ico1", False)
    st, ws, bs = _params(I, H, L, seed=2)
    g = torch.Generator().manual_seed(8)
    feats = torch.randn(1, n, I, generator=g, dtype=torch.float64) * 0.5
    gup = torch.randn(1, n, 3, generator=g, dtype=torch.float64)
    c = og.cut_length(H, 0.33)
    assert c == 5
    acts, upd = og.bf16_stack_forward(feats, ws, bs, adj, c, 2)
    gf, dws, dbs = og.bf16_stack_backward(acts, ws, adj, c, 2, gup)
    rp, col, val = (t.tolist() for t in adj)
    n_acts, n_upd, n_gf, n_dws, n_dbs = _naive(feats[0].tolist(), [w[0].tolist() for w in ws], [b.tolist() for b in bs],
                                                rp, col, val, c, gup[0].tolist())
    T = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    # the bf16 activations are bf16 values on both sides: identical unless a sum lands within float64 rounding of a tie
    for a, b in zip(acts, n_acts):
        assert torch.equal(a[0], T(b))
        assert torch.equal(a[0], a[0].to(torch.bfloat16).double())
    assert _rel(upd[0], T(n_upd)) < 1e-13
    assert _rel(gf[0], T(n_gf)) < 1e-13
    for i in range(L):
        assert _rel(dws[i][0], T(n_dws[i])) < 1e-13, i
        assert _rel(dbs[i], T(n_dbs[i])) < 1e-13, i
    assert (dbs[0][c:] == 0).all() and (dbs[1][c:] == 0).all()
    # the emulation differs from autograd through oracle.gcn.gcn(..., bf16="storage") — the point of the explicit form
    leaf = {k: v.clone().requires_grad_(True) for k, v in st.items() if k.startswith("mesh_deform_1")}
    out = og.gcn(feats, leaf, "mesh_deform_1", adj, L, 0.33, bf16="storage")
    (out * gup).sum().backward()
    assert _rel(out.detach(), upd) < 1e-12                      # same forward
    assert _rel(leaf["mesh_deform_1.layers.0.weight"].grad, dws[0]) > 1e-4   # autograd rounds dW to bf16
