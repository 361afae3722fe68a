"""CPU: the exactly summable inputs of tests/test_gpu_gcn_exact.py (tests/gcn_exact_util.py) are what they claim to be.

Every case meets the precondition ``sum |terms| <= 2^24 quanta`` per sum of the chain; the graphs have the row lengths, the
symmetric pattern and the values claimed; on such inputs an fp32 evaluation equals the float64 oracle bit for bit in more than
one association (so the GPU gate may ask for ``torch.equal``); and the gate is sharp: one quantum in one element, or one edge
missing from the graph, is a failed comparison."""
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
