"""-m gpu: the exact-fp32 GCN stack against the float64 oracle BIT FOR BIT, on inputs whose every fp32 sum is exact in any order.

tests/gcn_exact_util.py builds the inputs (ternary features, weights and ``grad_update``, integer biases, adjacency values
1/2 and 1/4) and states the precondition ``sum |terms| <= 2^24 quanta`` for every sum of the forward and backward chain;
tests/test_gcn_exact_host.py proves it for every case used here, shows on the CPU that fp32 then equals fp64 in more than one
association, and that one quantum in one element or one missing edge fails the comparison.  So every assertion below is
``torch.equal`` — outputs, ``grad_feats`` (pad columns exactly zero), every dW and every db (dead bias channels exactly
zero) — whatever the tiling, split or summation order of the kernels: the layer-0 products, rowgemm / rowgemmw, dw / dww, csr
and csrq forward and transposed, the thin output layer and the slab reduces.  There are no ReLU kinks to tolerate: the
pre-activations are exact, some 7 % of them are exactly 0, and ``relu'(0) = 0`` there as in the oracle's autograd.

Each case asserts through ``ops.path_counts`` that it reached the kernels it names, and prints its worst share of 2^24.

The P + bipartite split kernels (csrc/gcn_csrqs.hip: ``csrqs_kernel<MODE, VPT>`` and ``csrqs_image_kernel``; csrc/gcn_csr.hip:
``csr3s_kernel<TRANSPOSED>``) are held to the same gate by the ``test_split_*`` cases.  They never compute 1 / row length: they
take ``a3vt_adj_split.scale`` as data, and ``a3vt_adj_split_validate`` asks only that every value of row i of the full CSR is
``scale[i]``.  So the graph is ``diag(s) (P + J)`` with s in {1/2, 1/4} (graph "s" of tests/gcn_exact_util.py, built by physical
vertex index: where a vertex sits in the 512-thread workgroup is the point) — not row-normalised, on purpose — and each case
installs the validated split on its ``ops.DeviceCSR`` itself.  Shapes: four and six vertices per thread, a last slot of four
vertices with vertex n-1 (the one threads past the mesh's end copy) in S and in C, 16 / 10 (uneven) / 25 (clamped) / 3 / 1
parts, a mesh smaller than the workgroup, batches that are and are not multiples of 8, cut_len 12, 99, 128 and 132 (not
taken), forward only, csr3s_kernel alone below the hybrid threshold and its LDS limit, the plain CSR and the forced row
kernels on the same inputs, and batch invariance.  ``csr3_split`` counts the csr3s_kernel launches.

Not covered here: gemm mode ``fp32x3`` on the split graph.  Its dW condition (|dZ| of the hidden layers at most 255 quanta)
is out of reach with class sums of some 250 terms (~1000 quanta on sparse inputs), and the mode aggregates with the same
csrqs_kernel as fp32.  The real 1 / row length values of the fused vision + touch matrix, which are no powers of two, keep
tests/test_gpu_csr_sliced.py.  The bf16 modes (the bf16-storage split walk included) have their own rounding-exact gate
(tests/test_gpu_bf16_exact.py).
"""
import ctypes

import pytest
import torch

import gcn_exact_util as gx
from helpers import _fuzz_shapes

pytestmark = pytest.mark.gpu


def _same(got, want, what):
    """``torch.equal`` with the element pattern of a mismatch in the message (which rows, which columns)."""
    got = got.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, what
    if torch.equal(got, want):
        return
    bad = (got != want) | torch.isnan(got)
    idx = bad.nonzero()
    cols = sorted(set(idx[:, -1].tolist()))
    rows = sorted(set(idx[:, -2].tolist())) if idx.shape[1] > 1 else []
    first = tuple(idx[0].tolist())
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at {first}: "
                         f"{got[first].item()!r} != {want[first].item()!r}; columns {cols[:12]}.. ({len(cols)}), "
                         f"rows {rows[:12]}.. ({len(rows)})")


def _device_adj(cuda, g):
    from a3vt_amd import mesh as amesh, ops
    return ops.DeviceCSR(amesh.CSRAdjacency(g.rowptr, g.col, g.val, g.n), cuda)


def _precondition(c):
    s = gx.case_sums(c)
    worst = gx.assert_exactly_summable(gx.problem(c), s)      # before any GPU call
    return worst, s.worst_name


def _run(cuda, p, adj, mode=False, feats=None, gup=None):
    """One forward (+ backward) of ``ops.gcn_stack`` on a lattice problem (``feats``, ``gup``: other meshes than the problem's
    own, same weights).  Returns (out, grad_feats, dWs, dbs, path counts)."""
    from a3vt_amd import ops
    c = p.case
    feats, gup = p.feats if feats is None else feats, p.grad_update if gup is None else gup
    fd = torch.nn.functional.pad(feats, (0, 2)).to(cuda).requires_grad_(c.backward)
    ws = [w.to(cuda).requires_grad_(c.backward) for w in p.weights]
    bs = [b.to(cuda).requires_grad_(c.backward) for b in p.biases]
    ops.path_counts(reset=True)
    if not c.backward:
        with torch.no_grad():
            out = ops.gcn_stack(fd, adj, gx.IN_FEATURES, c.hidden, p.cut_len, ws, bs, bf16=mode)
        torch.cuda.synchronize()
        return out, None, None, None, ops.path_counts()
    out = ops.gcn_stack(fd, adj, gx.IN_FEATURES, c.hidden, p.cut_len, ws, bs, bf16=mode)
    (out * gup.to(cuda)).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), fd.grad, [w.grad for w in ws], [b.grad for b in bs], ops.path_counts()


def _compare(p, res, what):
    c, ref = p.case, gx.reference(p.case)
    out, gf, dws, dbs, _ = res
    _same(out, ref.out, f"{what}: output")
    if not c.backward:
        return
    _same(gf[..., :gx.IN_FEATURES], ref.grad_feats, f"{what}: grad_feats")
    assert (gf[..., gx.IN_FEATURES:] == 0).all(), f"{what}: grad_feats pad columns"
    for i in range(c.layers):
        _same(dws[i], ref.dws[i], f"{what}: dW{i}")
        _same(dbs[i], ref.dbs[i], f"{what}: db{i}")
        if i < c.layers - 1:
            assert (dbs[i][p.cut_len:] == 0).all(), f"{what}: dead bias channels of layer {i}"


def _case(cuda, name, want, algo="auto", mode=False):
    """Run one named case and compare everything; ``want``: path counters that must be positive."""
    from a3vt_amd import ops
    c = gx.STACK_CASES[name]
    worst, where = _precondition(c)
    p = gx.problem(c)
    adj = _device_adj(cuda, p.graph)
    ops.dbg_csr_algo(algo)
    try:
        res = _run(cuda, p, adj, mode)
    finally:
        ops.dbg_csr_algo("auto")
    paths = res[-1]
    print(f"\n{name} [{algo}, mode {mode or 'fp32'}]: {c.batch * c.n} rows, cut_len {p.cut_len}, worst sum {where} at "
          f"{worst:.3f} of 2^24; paths { {k: v for k, v in paths.items() if v} }")
    for k in want:
        assert paths[k] > 0, (name, k, paths)
    assert paths["stack_split"] == 0, paths                    # the plain CSR everywhere (module docstring)
    _compare(p, res, f"{name}/{algo}")
    return paths


def test_sliced_whole_tiles(cuda):
    """12 336 rows = 771 whole 16-row tiles: the weights-resident products and dW kernels of the hidden -> hidden layer."""
    paths = _case(cuda, "whole_tiles", ("stack_quad", "rowgemm_w", "dw_w"))
    assert paths["stack_rows"] == 0


def test_sliced_ragged_rows(cuda):
    """13 364 rows: 4 rows past the last whole tile — the generic 19-tile product and dw_kernel on quad-major operands."""
    paths = _case(cuda, "ragged_rows", ("stack_quad", "rowgemm_adirect", "dw_hybrid"))
    assert paths["rowgemm_w"] == 0 and paths["dw_w"] == 0, paths


def test_sliced_six_vertices_per_thread(cuda):
    """n = 2564 > 4 x 512: csrq keeps six vertices per thread; 12 820 rows, ragged."""
    _case(cuda, "six_per_thread", ("stack_quad",))


def test_four_layers_hidden_to_hidden(cuda):
    """Two hidden -> hidden layers: a hybrid layer output feeds the next weights-resident product, forward and backward."""
    _case(cuda, "four_layers", ("stack_quad", "rowgemm_w", "dw_w"))


@pytest.mark.parametrize("algo,path", [("rows", "stack_rows"), ("sliced", "stack_quad")])
def test_long_and_hub_rows(cuda, algo, path):
    """Rows of 2 .. 8 entries (register slots), 16 (CSR continuation) and 103 (the heavy pass), values that differ inside a
    row and between A and A^T: both aggregations, forward and transposed."""
    g = gx.graph("b", 1028)
    deg = g.rowptr[1:] - g.rowptr[:-1]
    assert deg.min() <= 8 and ((deg > 8) & (deg <= 64)).any() and deg.max() > 64
    _case(cuda, "hub_rows", (path,), algo=algo)


@pytest.mark.parametrize("name", ["cut_004", "cut_05"])
def test_other_cuts(cuda, name):
    """cut_len 12 and 150: other column splits between the aggregated and the plain channels; the path is the shape rule's."""
    paths = _case(cuda, name, ())
    assert paths["stack_quad"] + paths["stack_rows"] == 1, paths


@pytest.mark.parametrize("name", ["small_h300", "small_h32"])
def test_below_the_hybrid_threshold(cuda, name):
    """780 rows on the hub-row graph: row-major rows, the generic products, csr_fwd / csr_bwd with their heavy pass."""
    paths = _case(cuda, name, ("stack_rows",))
    assert paths["stack_quad"] == 0


def test_forward_only_dense_weights(cuda):
    """``torch.no_grad()``: no stash, no sign bytes; every weight +-1 (the forward has the room)."""
    _case(cuda, "forward_dense", ("stack_quad",))


@pytest.mark.parametrize("name", ["whole_tiles", "four_layers"])
def test_fp32x3_is_exact_on_the_lattice(cuda, name):
    """Gemm mode 3: six bf16 products of operands split in three.  Exact when one operand of each product fits bf16's 8
    significant bits: the ternary weights (forward, dX); for dW the dZ of the layers on the split kernels, at most 255 quanta
    (asserted here and in tests/test_gcn_exact_host.py) — so dW is compared as well."""
    c = gx.STACK_CASES[name]
    dzq = gx.case_sums(c).dz_quanta
    assert all(dzq[i] <= 255 for i in range(1, c.layers - 1)), dzq
    _case(cuda, name, ("stack_quad", "rowgemm3", "dw3"), mode="fp32x3")


def test_backward_accumulates_exactly(cuda):
    """``a3vt_gcn_stack_bwd_acc`` with accumulate = 1, twice (the trainer's bucket: one stack serves two stages), onto sinks
    pre-filled with integers: prefill + 2 x reference, bit for bit; ``grad_feats`` is written, not accumulated."""
    from a3vt_amd import lib as _lib, ops
    c = gx.STACK_CASES["whole_tiles"]
    worst, _ = _precondition(c)
    assert 2 * worst + 3 * 2.0 ** 6 / gx.LIMIT <= 1.0          # the accumulated sums stay exact too
    p, ref = gx.problem(c), gx.reference(c)
    adj = _device_adj(cuda, p.graph)
    feats = torch.nn.functional.pad(p.feats, (0, 2)).to(cuda)
    ws, bs = [w.to(cuda) for w in p.weights], [b.to(cuda) for b in p.biases]
    gup = p.grad_update.to(cuda)
    g = torch.Generator().manual_seed(9)
    pre_w = [torch.randint(-3, 4, w.shape, generator=g).float() for w in ws]
    pre_b = [torch.randint(-3, 4, b.shape, generator=g).float() for b in bs]
    gw, gb = [t.to(cuda) for t in pre_w], [t.to(cuda) for t in pre_b]
    Lb = _lib.load()
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    ops.path_counts(reset=True)
    for use in range(2):
        fd = feats.clone().requires_grad_(True)
        wl = [w.clone().requires_grad_(True) for w in ws]
        out = ops.gcn_stack(fd, adj, gx.IN_FEATURES, c.hidden, p.cut_len, wl, bs)
        ctx = out.grad_fn
        gfeats = torch.full_like(feats, 7.0)
        scratch = ops.workspace("gcn", Lb.a3vt_gcn_stack_scratch_bytes_mode(c.batch, c.n, gx.IN_FEATURES, c.hidden, c.layers,
                                                                            p.cut_len, 1, 0), cuda)
        _lib.check(Lb.a3vt_gcn_stack_bwd_acc(
            _lib.ptr(feats), feats.shape[-1], gx.IN_FEATURES, arr(ws), arr(bs), c.layers, c.hidden, p.cut_len,
            _lib.ptr(adj.rowptr), _lib.ptr(adj.col), _lib.ptr(adj.val), _lib.ptr(adj.t_rowptr), _lib.ptr(adj.t_col),
            _lib.ptr(adj.t_val), max(adj.max_degree, adj.t_max_degree), c.n, c.batch, 0, _lib.ptr(ctx.acts),
            _lib.ptr(ctx.masks), _lib.ptr(gup), arr(gw), arr(gb), _lib.ptr(gfeats), _lib.ptr(scratch), 1,
            torch.cuda.current_stream().cuda_stream), "gcn_stack_bwd_acc")
        torch.cuda.synchronize()
        _same(gfeats[..., :gx.IN_FEATURES], ref.grad_feats, f"use {use}: grad_feats")
        assert (gfeats[..., gx.IN_FEATURES:] == 0).all()
    paths = ops.path_counts()
    assert paths["stack_quad"] == 2 and paths["dw_w"] > 0, paths
    for i in range(c.layers):
        _same(gw[i], pre_w[i] + 2 * ref.dws[i], f"accumulated dW{i}")
        _same(gb[i], pre_b[i] + 2 * ref.dbs[i], f"accumulated db{i}")


# ---- the P + bipartite split: csrqs_kernel<MODE, VPT>, csrqs_image_kernel (csrc/gcn_csrqs.hip) and csr3s_kernel<TRANSPOSED> --------

def _device_adj_split(cuda, g):
    """``ops.DeviceCSR`` of the full CSR of a split graph, with the split installed the way ``DeviceCSR.__init__`` does it:
    proven against the CSR by the library first.  ``CSRAdjacency.split()`` itself does not find it — the values are powers of
    two, not 1 / row length (tests/test_gcn_exact_host.py)."""
    from a3vt_amd import lib as _lib, mesh as amesh
    adj = _device_adj(cuda, g)
    assert adj.split is None and adj.split_struct is None and adj.max_degree > 8
    sp = gx.split_arrays(g)
    host = adj.host
    _lib.check(_lib.load().a3vt_adj_split_validate(host.rowptr.ctypes.data, host.col.ctypes.data, host.val.ctypes.data, host.n,
                                                   sp.p_rowptr.ctypes.data, sp.p_col.ctypes.data, sp.scale.ctypes.data,
                                                   sp.cls.ctypes.data), "adj_split_validate")
    hs = amesh.SplitAdjacency(sp.p_rowptr, sp.p_col, sp.scale, sp.cls)
    assert hs.max_degree <= 12 and hs.n_centre == 4
    adj.split = tuple(torch.from_numpy(a).to(cuda) for a in (hs.rowptr, hs.col, hs.scale, hs.cls))
    adj.split_struct = _lib.AdjSplit(*[t.data_ptr() for t in adj.split], hs.max_degree, hs.n_seam, hs.n_centre)
    return adj


def _split_case(cuda, name, counts, algo="auto", use_split=True, more_meshes=0):
    """Run one case of ``gx.SPLIT_CASES`` and compare everything bit for bit; ``counts``: the path counters of the call, exactly.
    ``more_meshes``: the batch grows by copies of the first meshes with a zero ``grad_update`` — the reference stays the
    case's own (they add exact zeros to dW and db), the launch gets other ``parts`` and other workgroups."""
    from a3vt_amd import ops
    c = gx.SPLIT_CASES[name]
    worst, where = _precondition(c)
    p = gx.problem(c)
    adj = _device_adj_split(cuda, p.graph)
    adj.use_split = use_split
    feats = torch.cat((p.feats, p.feats[:more_meshes]))
    gup = torch.cat((p.grad_update, torch.zeros_like(p.grad_update[:more_meshes])))
    ops.dbg_csr_algo(algo)
    try:
        res = _run(cuda, p, adj, feats=feats, gup=gup)
    finally:
        ops.dbg_csr_algo("auto")
    paths = res[-1]
    what = f"{name}/{algo}/{'split' if use_split else 'plain'}/+{more_meshes}"
    print(f"\n{what}: {feats.shape[0] * c.n} rows, cut_len {p.cut_len}, worst sum {where} at {worst:.3f} of 2^24; paths "
          f"{ {k: v for k, v in paths.items() if v} }")
    for k, v in counts.items():
        assert paths[k] == v, (what, k, paths)
    out, gf, dws, dbs, _ = res
    if more_meshes:
        ref = gx.reference(c)
        _same(out[c.batch:], ref.out[:more_meshes], f"{what}: output of the further meshes")
        if c.backward:
            assert (gf[c.batch:] == 0).all(), f"{what}: grad_feats of the further meshes"
            gf = gf[:c.batch]
        out = out[:c.batch]
    _compare(p, (out, gf, dws, dbs, paths), what)
    return paths


# hidden layers on csrqs_kernel (forward and backward), the output layer both ways on csr3s_kernel
_ALL_SPLIT = dict(stack_split=1, stack_quad=1, stack_rows=0, csr3_split=2)


@pytest.mark.parametrize("name", ["split_last_in_s", "split_last_in_c"])
def test_split_four_vertices_per_thread(cuda, name):
    """n = 1028, batch 12, cut_len 99: VPT 4, the third per-thread slot holds four live vertices (a centre or two among
    them) and the fourth none, so threads 4 .. 511 of slot 2 and all of slot 3 copy vertex n-1 — a member of S in one variant,
    a centre in the other: they must add nothing to its class sum.  16 parts of one or two quads; the tail quad carries a
    pass-through channel; wave 0 of slot 0 walks one slot pair, others six."""
    _split_case(cuda, name, _ALL_SPLIT)


def test_split_uneven_parts(cuda):
    """n = 516, batch 24 (a multiple of 8): 10 parts over 25 quads, two or three quads each; slot 1 holds four vertices."""
    _split_case(cuda, "split_uneven_parts", _ALL_SPLIT)


def test_split_mesh_smaller_than_the_workgroup(cuda):
    """n = 96, batch 136: 416 of the 512 threads own no vertex; ``parts == 1``, so one workgroup parks and walks all 25
    quads through the double buffer; 136 = 17 x 8 meshes over the XCD groups."""
    _split_case(cuda, "split_small_mesh", _ALL_SPLIT)


def test_split_six_vertices_per_thread(cuda):
    """n = 2564, batch 5: VPT 6, slot 5 holds four vertices (vertex n-1 a centre); ``parts`` clamped to one quad each; the
    workgroups of meshes 5 .. 7 of the XCD group exit."""
    _split_case(cuda, "split_six_per_thread", _ALL_SPLIT)


@pytest.mark.parametrize("name", ["split_cut_12", "split_cut_128"])
def test_split_other_cuts(cuda, name):
    """cut_len 12 (three quads, no tail quad, 16 parts clamped to 3) and 128 (the widest the split kernels take)."""
    assert gx.problem(gx.SPLIT_CASES[name]).cut_len == int(name.rsplit("_", 1)[1])
    _split_case(cuda, name, _ALL_SPLIT)


def test_split_not_taken_past_128_channels(cuda):
    """cut_len 132: csrqs_fits says no, the hidden layers fall back to the row kernels on the full CSR (hub rows on the heavy
    pass) — exact as well; the output layer keeps csr3s_kernel."""
    assert gx.problem(gx.SPLIT_CASES["split_cut_132"]).cut_len == 132
    _split_case(cuda, "split_cut_132", dict(stack_split=0, stack_quad=0, stack_rows=1, csr3_split=2))


def test_split_forward_only(cuda):
    """``torch.no_grad()``: the null sign array of csrqs_kernel<0>; ordinary densities."""
    _split_case(cuda, "split_forward_only", dict(stack_split=1, stack_quad=1, stack_rows=0, csr3_split=1))


def test_split_below_the_hybrid_threshold(cuda):
    """780 rows: the hidden layers on the row kernels (full CSR); the output layer and its transposed backward on
    csr3s_kernel with ``parts = 8`` over 260 vertices, which 8 does not divide."""
    _split_case(cuda, "split_below_threshold", dict(stack_split=0, stack_quad=0, stack_rows=1, csr3_split=2))


def test_split_mesh_past_the_lds_of_csr3s(cuda):
    """n = 3844: 3844 x 16 bytes are more than the 60 KB csr3s_kernel is given, so csr3_kernel + csr3_heavy_kernel must be
    what runs (and the hidden layers are past the six vertices per thread of csrqs_kernel)."""
    _split_case(cuda, "split_past_lds", dict(stack_split=0, stack_quad=0, stack_rows=1, csr3_split=0))


@pytest.mark.parametrize("algo,use_split,counts", [
    ("auto", False, dict(stack_split=0, stack_quad=0, stack_rows=1, csr3_split=0)),     # the plain CSR everywhere
    ("rows", True, dict(stack_split=0, stack_quad=0, stack_rows=1, csr3_split=2)),      # row kernels; csr3s for the output layer
    ("rows", False, dict(stack_split=0, stack_quad=0, stack_rows=1, csr3_split=0))])
def test_split_and_plain_aggregation_agree_on_the_reference(cuda, algo, use_split, counts):
    """The first shape again without the split and on the forced row kernels: the same fp64 reference, bit for bit, as
    test_split_four_vertices_per_thread — so the split path and the plain path equal each other too."""
    _split_case(cuda, "split_last_in_s", counts, algo=algo, use_split=use_split)


def test_split_is_batch_invariant(cuda):
    """The 12 meshes of the first shape inside a batch of 20 (10 parts instead of 16, 24 mesh slots instead of 16): the same
    bits for them, whatever the workgroup and the part that computes them."""
    _split_case(cuda, "split_last_in_s", _ALL_SPLIT, more_meshes=8)


@pytest.mark.parametrize("name", list(gx.LAYER_CASES))
def test_single_layer_on_hub_rows(cuda, name):
    """``ops.gcn_layer`` with a CSR handle on the hub-row graph: a hidden layer with the cut and ReLU, odd sizes with the cut and
    no activation, and the 3-channel output (every channel aggregated), forward and backward."""
    from a3vt_amd import ops
    c = gx.LAYER_CASES[name]
    p = gx.layer_problem(c)
    shares = gx.layer_sums(p)
    assert max(shares.values()) <= 1.0, shares
    y_ref, gx_ref, gw_ref, gb_ref = gx.layer_reference(c)
    adj = _device_adj(cuda, p.graph)
    assert adj.max_degree > 64 and adj.split is None
    x = torch.nn.functional.pad(p.x, (0, (-c.kin) % 4)).to(cuda).requires_grad_(True)
    w, b = p.weight.to(cuda).requires_grad_(True), p.bias.to(cuda).requires_grad_(True)
    y = ops.gcn_layer(x, adj, w, b, p.cut_len, c.relu)
    (y * p.grad_y.to(cuda)).sum().backward()
    torch.cuda.synchronize()
    print(f"\n{name}: worst sum at {max(shares.values()):.2e} of 2^24")
    _same(y, y_ref, "y")
    _same(x.grad[..., :c.kin], gx_ref, "grad_x")
    assert (x.grad[..., c.kin:] == 0).all()
    _same(w.grad, gw_ref, "grad_weight")
    _same(b.grad, gb_ref, "grad_bias")
    assert (b.grad[p.cut_len:] == 0).all()


def test_rowgemm_shape_fuzz_exact(cuda):
    """Every launch path of ``a3vt_rowgemm`` (the 48 shapes of test_gpu_kernels.test_rowgemm_shape_fuzz) on integer operands in
    [-3, 3]: sum |terms| <= 9 K <= 4068, far inside 2^24 — the product equals the float64 one bit for bit."""
    from a3vt_amd import ops
    for m, k, n in _fuzz_shapes(48, 20261002):
        assert 9 * k <= gx.LIMIT
        g = torch.Generator().manual_seed(m * 7 + k * 3 + n)
        a = torch.randint(-3, 4, (m, k), generator=g).float()
        w = torch.randint(-3, 4, (k, n), generator=g).float()
        c = ops.rowgemm(a.to(cuda), w.to(cuda))
        _same(c, (a.double() @ w.double()).float(), f"rowgemm {(m, k, n)}")
