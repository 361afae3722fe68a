"""CPU: the exactly summable inputs of tests/test_gpu_gcn_exact.py (tests/gcn_exact_util.py) are what they claim to be.

Every case meets the precondition ``sum |terms| <= 2^24 quanta`` per sum of the chain; the graphs have the row lengths, the
symmetric pattern and the values claimed; on such inputs an fp32 evaluation equals the float64 oracle bit for bit in more than
one association (so the GPU gate may ask for ``torch.equal``); and the gate is sharp: one quantum in one element, or one edge
missing from the graph, is a failed comparison."""
import functools

import numpy as np
import pytest
import torch

import gcn_exact_util as gx
from oracle import gcn as og


@pytest.mark.parametrize("name", list(gx.STACK_CASES))
def test_every_stack_case_is_exactly_summable(name):
    c = gx.STACK_CASES[name]
    s = gx.case_sums(c)
    worst = gx.assert_exactly_summable(gx.problem(c), s)
    print(f"{name}: worst sum {s.worst_name} at {worst:.3f} of 2^24; pre-activations exactly zero: {s.zero_fraction:.3f}")
    assert 0 < worst <= 1.0
    # the ReLU-at-zero convention (relu'(0) = 0) is exercised, not just permitted
    assert s.zero_fraction >= 0.05 or not c.backward


@pytest.mark.parametrize("name", list(gx.LAYER_CASES))
def test_every_layer_case_is_exactly_summable(name):
    shares = gx.layer_sums(gx.layer_problem(gx.LAYER_CASES[name]))
    assert 0 < max(shares.values()) <= 1.0, shares


def test_fp32x3_cases_keep_dz_within_bf16():
    """The six-product split is exact when one operand of each product has 8 significant bits: the ternary weights for the
    forward and dX; for dW the dZ of the layers on the split kernels (hidden -> hidden: 1 .. L-2), at most 255 quanta."""
    for name in ("whole_tiles", "four_layers"):
        c = gx.STACK_CASES[name]
        dzq = gx.case_sums(c).dz_quanta
        assert all(dzq[i] <= 255 for i in range(1, c.layers - 1)), (name, dzq)


def test_accumulating_backward_stays_on_the_lattice():
    """tests/test_gpu_gcn_exact.py adds the gradients of ``whole_tiles`` twice onto integers in [-3, 3]: every partial sum of
    prefill + 2 x gradient, in any order, within 2^24 quanta (the finest quantum of a three-layer stack is 2^-6)."""
    s = gx.case_sums(gx.STACK_CASES["whole_tiles"])
    assert 2 * s.worst + 3 * 2.0 ** 6 / gx.LIMIT <= 1.0


@pytest.mark.parametrize("kind,n", [("a", 1028), ("a", 2564), ("b", 1028), ("b", 260)])
def test_graphs_are_as_claimed(kind, n):
    g = gx.graph(kind, n)
    deg = np.diff(g.rowptr)
    rows = np.repeat(np.arange(n), deg)
    if kind == "a":
        assert sorted(set(deg)) == [2, 4]
        assert np.array_equal(g.val, (1.0 / deg[rows]).astype(np.float32))           # row-normalised
    else:
        hub = 1 + 3 * gx.hub_leaves(n) // 4
        assert sorted(set(deg)) == [2, 4, 8, 16, hub] and hub > 64 and int((deg == hub).sum()) == 4
        assert set(g.val.tolist()) == {0.5, 0.25}
        # both values inside one row, for rows of every length class; and A^T carries other values than A
        for d in (2, 4, 8, 16, hub):
            mixed = [len(set(g.val[g.rowptr[r]:g.rowptr[r + 1]].tolist())) == 2 for r in np.flatnonzero(deg == d)]
            assert any(mixed), d
        dense = np.zeros((n, n), dtype=np.float32)
        dense[rows, g.col] = g.val
        assert not np.array_equal(dense, dense.T)
    key = rows * n + g.col
    assert np.all(np.diff(key) > 0)                                                  # ascending columns, no entry twice
    assert np.array_equal(np.sort(g.col.astype(np.int64) * n + rows), key)           # symmetric pattern
    assert int((rows == g.col).sum()) == n                                           # a self loop in every row


def test_tile_edge_rows_and_columns_are_nonzero():
    p = gx.problem(gx.STACK_CASES["whole_tiles"])
    for w in p.weights:
        k, h = w.shape[-2:]
        for i in gx.EDGE_INDICES:
            assert i >= k or w[0, i].abs().sum() > 0
            assert i >= h or w[0, :, i].abs().sum() > 0
        assert set(w.unique().tolist()) <= {-1.0, 0.0, 1.0}


def test_over_budget_problem_is_refused():
    """Dense +-1 weights with a backward: dW leaves the lattice and the precondition says so (an error, never a skip)."""
    c = gx.STACK_CASES["whole_tiles"]._replace(name="over_budget", w0_density=1.0, w_density=1.0, out_density=1.0)
    with pytest.raises(AssertionError, match="not exactly summable"):
        gx.assert_exactly_summable(gx.problem(c))


# ---- order independence and sharpness, on the small hub-row case -------------------------------------------------------

SMALL = gx.STACK_CASES["small_h300"]


def _forward32(p, adj, regroup):
    """The stack forward in fp32 on the CPU: ``A (X W)`` per layer, or ``(A X) W`` on the aggregated channels."""
    x = p.feats.clone()
    adj = (adj[0], adj[1], adj[2].float())
    for i in range(p.case.layers):
        last = i == p.case.layers - 1
        w, b = p.weights[i][0], p.biases[i]
        cl = w.shape[1] if last else p.cut_len
        if regroup:
            y = torch.cat((og.adj_matmul(adj, x) @ w[:, :cl] + b[:cl], x @ w[:, cl:]), dim=-1)
        else:
            z = x @ w
            y = torch.cat((og.adj_matmul(adj, z[..., :cl]) + b[:cl], z[..., cl:]), dim=-1)
        x = y if last else torch.relu(y)
    return x


def test_fp32_equals_fp64_in_either_association():
    p, ref = gx.problem(SMALL), gx.reference(SMALL)
    adj = gx.oracle_adj(p.graph)
    assert ref.out.dtype == torch.float32 and torch.equal(ref.out.double(), gx.oracle_reference(p).out)   # the cast is exact
    assert torch.equal(_forward32(p, adj, False), ref.out)
    assert torch.equal(_forward32(p, adj, True), ref.out)


def test_dw_in_fp32_as_one_product_and_as_reversed_row_blocks():
    p, ref = gx.problem(SMALL), gx.reference(SMALL)
    s = gx.exact_sums(p)
    for i in range(SMALL.layers):
        x = s.acts[i].float().reshape(-1, s.acts[i].shape[-1])
        dz = s.dzs[i].float().reshape(-1, s.dzs[i].shape[-1])
        assert torch.equal(x.t() @ dz, ref.dws[i][0]), i
        acc = torch.zeros_like(ref.dws[i][0])
        for r0 in reversed(range(0, x.shape[0], 37)):
            acc += x[r0:r0 + 37].t() @ dz[r0:r0 + 37]
        assert torch.equal(acc, ref.dws[i][0]), i


def test_explicit_chain_equals_autograd():
    """The precondition's own restatement of the backward (exact_sums) and the oracle's autograd agree on dZ of layer 0, hence on
    every step above it: grad_feats = dZ_0 W_0^T."""
    p, ref = gx.problem(SMALL), gx.reference(SMALL)
    s = gx.exact_sums(p)
    assert torch.equal((s.dzs[0] @ p.weights[0][0].double().t()).float(), ref.grad_feats)


def test_the_gate_is_sharp():
    p, ref = gx.problem(SMALL), gx.reference(SMALL)
    adj = gx.oracle_adj(p.graph)
    got = _forward32(p, adj, False)
    # one quantum (2^-6 after three aggregations) in one element
    off = ref.out.clone()
    off[1, 7, 2] += 2.0 ** -(gx.AGG_SHIFT * SMALL.layers)
    assert off[1, 7, 2] != ref.out[1, 7, 2] and not torch.equal(got, off)
    # one edge missing from the CSR handed to the oracle (the last entry of a 16-entry row)
    g = p.graph
    row = int(np.flatnonzero(np.diff(g.rowptr) == 16)[0])
    e = int(g.rowptr[row + 1]) - 1
    rowptr = torch.from_numpy(g.rowptr).long().clone()
    rowptr[row + 1:] -= 1
    keep = torch.arange(len(g.col)) != e
    fewer = (rowptr, adj[1][keep], adj[2][keep])
    r2 = gx.oracle_reference(p, fewer)
    assert not torch.equal(got.double(), r2.out)
    assert not torch.equal(ref.grad_feats.double(), r2.grad_feats)
    # a swapped pair of values inside that row
    val = adj[2].clone()
    a, b = int(g.rowptr[row]), int(g.rowptr[row]) + 1
    while val[a] == val[b]:
        b += 1
    val[a], val[b] = val[b].clone(), val[a].clone()
    assert not torch.equal(got.double(), gx.oracle_reference(p, (adj[0], adj[1], val)).out)


# ---- the split graph diag(s) (P + J): csrqs_kernel, csrqs_image_kernel and csr3s_kernel --------------------------------

SPLIT_GRAPHS = sorted({(c.graph, c.n) for c in gx.SPLIT_CASES.values()})
SPLIT_SMALL = gx.SPLIT_CASES["split_below_threshold"]


@pytest.mark.parametrize("kind,n", SPLIT_GRAPHS)
def test_split_graph_is_as_claimed(kind, n):
    """P, S, C and the values of graph "s" / "sc", by physical vertex index (where a vertex sits in the 512-thread workgroup of
    csrqs_kernel is the point); ``a3vt_adj_split_validate`` proves the split against the full CSR; and
    ``CSRAdjacency.split()`` does not find it (the values are not 1 / row length), which is why tests/test_gpu_gcn_exact.py
    installs the split itself."""
    from a3vt_amd import lib, mesh as amesh
    g = gx.graph(kind, n)
    sp = gx.split_arrays(g)
    v = np.arange(n)
    pdeg = np.diff(sp.p_rowptr)
    prow = np.repeat(v, pdeg)
    pkey = prow * n + sp.p_col
    # P: ascending, symmetric, a self loop everywhere, nothing but the self loop in the first wave's vertices
    assert np.all(np.diff(pkey) > 0) and np.array_equal(np.sort(sp.p_col.astype(np.int64) * n + prow), pkey)
    assert int((prow == sp.p_col).sum()) == n and np.all(pdeg[:64] == 1)
    assert pdeg.max() <= 12
    if n >= 512:
        assert sorted(set(pdeg)) == list(range(1, 13))                     # odd lengths: a slot pair half filled
        # the last slot pair (rows of 11 and 12) is needed in some waves only: wave 0 of slot 0 stops at the first
        assert (pdeg >= 11).sum() >= 8
    # S: about a quarter; a member in every 16-lane DPP row of every wave of every per-thread slot that holds a vertex
    s_idx, c_idx = np.flatnonzero(sp.cls == 1), np.flatnonzero(sp.cls == 2)
    assert set(np.flatnonzero(v % 4 == 1)) <= set(s_idx) and len(s_idx) <= n // 4 + 1
    assert set(s_idx // 16) == set(v // 16)
    # C: four centres outside S, in different slots and waves as far as the mesh has them
    assert len(c_idx) == 4 and not set(c_idx) & set(s_idx)
    slots, waves = -(-n // gx.QS_THREADS), min(8, -(-n // 64))
    assert len(set(c_idx // gx.QS_THREADS)) == min(4, slots)
    assert len(set((c_idx % gx.QS_THREADS) >> 6)) == min(4, waves)
    assert sp.cls[n - 1] == (2 if kind == "sc" else 1)                     # the vertex that threads past the end copy
    # no S-C entry in P
    assert not np.any(sp.cls[prow].astype(int) * sp.cls[sp.p_col] == 2)
    # values and the full CSR: the sorted union of P and J, val = scale[row]
    assert np.array_equal(sp.scale, np.where(v % 3 == 1, 0.5, 0.25).astype(np.float32))
    deg = np.diff(g.rowptr)
    rows = np.repeat(v, deg)
    assert np.all(np.diff(rows * n + g.col) > 0) and np.array_equal(g.val, sp.scale[rows])
    assert np.array_equal(deg, pdeg + np.where(sp.cls == 1, 4, 0) + np.where(sp.cls == 2, len(s_idx), 0))
    if n >= 260:
        assert deg[c_idx].min() > 64                                       # the plain-CSR runs go through the heavy-row kernels
    L = lib.load()
    ptr = lambda a: np.ascontiguousarray(a).ctypes.data  # noqa: E731
    assert L.a3vt_adj_split_validate(ptr(g.rowptr), ptr(g.col), ptr(g.val), n, ptr(sp.p_rowptr), ptr(sp.p_col), ptr(sp.scale),
                                     ptr(sp.cls)) == 0, L.a3vt_last_error().decode()
    wrong = sp.scale.copy()
    wrong[n - 1] *= 2                                                       # (the validator does look at the values)
    assert L.a3vt_adj_split_validate(ptr(g.rowptr), ptr(g.col), ptr(g.val), n, ptr(sp.p_rowptr), ptr(sp.p_col), ptr(wrong),
                                     ptr(sp.cls)) != 0
    assert amesh.CSRAdjacency(g.rowptr, g.col, g.val, n).split() is None


@functools.lru_cache(maxsize=None)
def _split_facts(name):
    """One evaluation of the chain per case, shared by the two tests below: the figures of the precondition, and per hidden
    aggregation the (mesh, quad) pairs whose class sums would not discriminate."""
    c = gx.SPLIT_CASES[name]
    p = gx.problem(c)
    s = gx.exact_sums(p)
    blind = {}
    for what, sig_s, sig_c in gx.split_class_sums(p, s):
        blind[what] = (int((sig_s == 0).all(-1).sum()), int((sig_c == 0).all(-1).sum()), int((sig_s == sig_c).all(-1).sum()))
    return s._replace(acts=None, dzs=None), blind


@pytest.mark.parametrize("name", list(gx.SPLIT_CASES))
def test_every_split_case_is_exactly_summable(name):
    """``exact_sums`` bounds the sums over the FULL rows of diag(s) (P + J).  The split kernels associate differently — the
    sum over a row of P, sigma_S, sigma_C, then their sum, then the scale — but each of these partial sums is over a subset of
    the terms of a full row (the product with the power of two ``scale`` is exact, before or after), so the same bound holds
    for every one of them.  Shares of 2^24 as chosen: 0.67, 0.70, 0.48, 0.74, 0.59, 0.48, 0.52, 0.63, 0.30 (forward only),
    0.23 and 0.88 (n = 3844)."""
    c = gx.SPLIT_CASES[name]
    s, _ = _split_facts(name)
    worst = gx.assert_exactly_summable(gx.problem(c), s)
    print(f"{name}: worst sum {s.worst_name} at {worst:.3f} of 2^24; pre-activations exactly zero: {s.zero_fraction:.3f}")
    assert 0 < worst <= 1.0
    assert s.zero_fraction >= 0.05


@pytest.mark.parametrize("name", list(gx.SPLIT_CASES))
def test_class_sums_discriminate_in_every_quad(name):
    """For every mesh and every aggregated quad of every hidden aggregation, forward and backward: sigma_S and sigma_C are
    non-zero in at least one channel and differ from each other — a kernel that drops or swaps the bipartite term in one quad
    of one mesh then shows (``gcn_exact_util._keep_class_sums_alive`` arranges the inputs for it)."""
    _, blind = _split_facts(name)
    c = gx.SPLIT_CASES[name]
    assert set(blind) == {f"{d} {i}" for i in range(c.layers - 1) for d in (("forward", "backward") if c.backward else ("forward",))}
    assert all(v == (0, 0, 0) for v in blind.values()), f"(sigma_S = 0, sigma_C = 0, sigma_S = sigma_C) per aggregation: {blind}"


def test_split_association_in_fp32_equals_fp64_and_is_sharp():
    """The forward in fp32 on the CPU in the split's own association (P sum, plus class sum, then scale) equals the float64
    oracle on the full CSR bit for bit, and each single fault of that association fails ``torch.equal``."""
    p, ref = gx.problem(SPLIT_SMALL), gx.reference(SPLIT_SMALL)
    sp = gx.split_arrays(p.graph)
    n = p.graph.n
    assert p.cut_len % 4 != 0                                               # the last quad has a pass-through channel
    assert torch.equal(gx.split_forward32(p), ref.out)
    s_idx, c_idx = np.flatnonzero(sp.cls == 1), np.flatnonzero(sp.cls == 2)
    row12 = int(np.flatnonzero(np.diff(sp.p_rowptr) == 12)[0])
    faults = {"one member removed from S": dict(drop_member=int(s_idx[len(s_idx) // 2])),
              "one centre counted twice": dict(twice=int(c_idx[1])),
              "sigma_S and sigma_C swapped": dict(swap=True),
              "the last P entry of a 12-entry row dropped": dict(drop_last_of=row12),
              "a pass-through channel of the last quad scaled": dict(scale_tail=True),
              "the last vertex once more in its class sum": dict(last_again=True)}
    assert sp.cls[n - 1] == 1
    for what, kw in faults.items():
        assert not torch.equal(gx.split_forward32(p, **kw), ref.out), what
