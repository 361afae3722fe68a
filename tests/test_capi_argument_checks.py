"""CPU tests (no GPU, no compute): the C ABI's argument checks return an error code and a message instead of touching memory
— every call below passes NULL / misaligned / out-of-range arguments, fake device addresses that must never be dereferenced on
the host, or host arrays of EXACTLY the size the call may write.  ``tools/asan_host.sh`` runs this file against a build of
the library whose host side is compiled with AddressSanitizer (CPU only), so an entry point that reads or writes past one of
these arrays is caught (verdict r05 #9)."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    from a3vt_amd import lib
    return lib.load()


def _err(L):
    return L.a3vt_last_error().decode()


FAKE = ctypes.c_void_p(0x7F0000001000)       # a "device pointer": 16-byte aligned, never mapped on the host
FAKE_ODD = ctypes.c_void_p(0x7F0000001008)   # 8 mod 16


def test_counters_write_exactly_n_entries(L):
    for n in (0, 1, 3, 12, 40):
        buf = (ctypes.c_longlong * max(n, 1))()
        kept = L.a3vt_dbg_path_counts(buf, n, 0)
        assert kept >= 12
    tot, cnt = (ctypes.c_double * 3)(), (ctypes.c_int * 3)()
    assert L.a3vt_profile_read_classes(tot, cnt, 3) >= 0         # (the number of classes the library keeps)
    assert L.a3vt_profile_read_classes(None, cnt, 3) < 0
    work = (ctypes.c_ulonglong * 8)()
    L.a3vt_dbg_nn_work(0, work)                                   # (reads device counters: an error code without a GPU, never a crash)


def test_csr_and_split_validators_on_host_arrays(L):
    from a3vt_amd import mesh as amesh
    v, f = amesh.icosphere(2)
    csr = amesh.CSRAdjacency.from_pairs(*amesh.vision_pairs(f, v.shape[0]), v.shape[0])
    rp = np.ascontiguousarray(csr.rowptr, dtype=np.int32)
    col = np.ascontiguousarray(csr.col, dtype=np.int32)
    assert L.a3vt_csr_validate(rp.ctypes.data, col.ctypes.data, v.shape[0], col.size) == 0
    bad = col.copy()
    bad[-1] = v.shape[0]                                   # a column index one past the end
    assert L.a3vt_csr_validate(rp.ctypes.data, bad.ctypes.data, v.shape[0], col.size) != 0
    assert L.a3vt_csr_validate(rp.ctypes.data, col.ctypes.data, v.shape[0], col.size - 1) != 0    # nnz disagrees with rowptr
    assert L.a3vt_csr_validate(None, col.ctypes.data, v.shape[0], col.size) != 0
    rp2 = rp.copy()
    rp2[3] = rp2[2] - 1                                    # not monotone
    assert L.a3vt_csr_validate(rp2.ctypes.data, col.ctypes.data, v.shape[0], col.size) != 0
    # the split validator: P's rowptr is checked whole before any row of P is read
    sp = csr.split()
    n = v.shape[0]
    p_rp, p_col = np.ascontiguousarray(sp.rowptr, dtype=np.int32), np.ascontiguousarray(sp.col, dtype=np.int32)
    scale, cls = np.ascontiguousarray(sp.scale, dtype=np.float32), np.ascontiguousarray(sp.cls, dtype=np.uint8)
    check = lambda prp: L.a3vt_adj_split_validate(rp.ctypes.data, col.ctypes.data, csr.val.ctypes.data, n, prp.ctypes.data,   # noqa: E731
                                                  p_col.ctypes.data, scale.ctypes.data, cls.ctypes.data)
    assert check(p_rp) == 0
    # row 0 is intact, but its second neighbour j has a row end past P: the symmetry search of (0, j) would probe p_col[nnz(P)]
    j = int(p_col[p_rp[0] + 1])
    bad = p_rp.copy()
    bad[j + 1] = 2 * p_col.size - bad[j] + 1
    assert check(bad) != 0 and "adj_split" in _err(L)
    bad = p_rp.copy()
    bad[n] += 1                                            # one entry more than P has
    assert check(bad) != 0


def test_size_queries_never_fail_on_odd_sizes(L):
    for b, n, i, h, nl, c in ((1, 1, 1, 4, 1, 0), (64, 2562, 50, 300, 20, 99), (8, 10242, 448, 300, 20, 99), (3, 17, 600, 304, 2, 304),
                              (0, 0, 0, 0, 0, 0), (-1, 5, 5, 5, 5, 5)):
        for mode in (0, 1, 2, 3):
            L.a3vt_gcn_stack_scratch_bytes_mode(b, n, i, h, nl, c, 1, mode)
        L.a3vt_gcn_stack_scratch_bytes(b, n, i, h, nl, c, 1)
        L.a3vt_gcn_stack_mask_bytes(b, n, h, nl, c)
        ab, mb = ctypes.c_size_t(), ctypes.c_size_t()
        L.a3vt_gcn_stack_stash_bytes(b, n, h, nl, c, 2, ctypes.byref(ab), ctypes.byref(mb))
    assert L.a3vt_gcn_stack_stash_bytes(2, 10, 300, 3, 99, 0, None, None) != 0
    assert L.a3vt_bnrelu_scratch_bytes(0) == 0 and L.a3vt_bnrelu_scratch_bytes(16) > 0
    assert L.a3vt_bias_grad_scratch_bytes(0, 16) == 0
    L.a3vt_chamfer_workspace_bytes(3, 64, 10000, 10000)
    L.a3vt_chamfer_workspace_bytes(0, 0, 0, 0)


def test_size_queries_agree_with_each_other(L):
    """Relations between the size queries of the GCN entry points, over every 13th shape of the grid below (13 is coprime to
    every axis length, so each value of each axis is visited; 222 shapes).  Nothing is allocated and no device is touched."""
    import itertools
    grid = itertools.product((1, 2, 13, 64), (162, 1824, 2562), (3, 50, 300, 448, 600), (16, 64, 300, 304), (1, 2, 3, 20), (0, 1, 2))
    ab, mb = ctypes.c_size_t(), ctypes.c_size_t()
    shapes = 0
    for b, n, fin, h, nl, ci in itertools.islice(grid, 0, None, 13):
        c = (0, round(0.33 * h), h)[ci]
        shapes += 1
        what = (b, n, fin, h, nl, c)
        by_mode = [[L.a3vt_gcn_stack_scratch_bytes_mode(b, n, fin, h, nl, c, back, mode) for mode in range(4)] for back in (0, 1)]
        for back in (0, 1):
            modes = [m for m in range(4) if m != 2 or nl >= 2]          # the bf16 storage mode needs a hidden layer
            assert L.a3vt_gcn_stack_scratch_bytes(b, n, fin, h, nl, c, back) == max(by_mode[back][m] for m in modes) > 0, what
        assert all(by_mode[1][m] >= by_mode[0][m] for m in range(4)), what
        assert L.a3vt_gcn_stack_scratch_bytes(b, n, fin, h, nl, c, 1) >= L.a3vt_gcn_stack_scratch_bytes(b, n, fin, h, nl, c, 0), what
        for mode in range(4):
            assert L.a3vt_gcn_stack_stash_bytes(b, n, h, nl, c, mode, ctypes.byref(ab), ctypes.byref(mb)) == 0, what
            if nl == 1:
                assert (ab.value, mb.value) == (0, 0), what
            elif mode != 2:
                assert mb.value == L.a3vt_gcn_stack_mask_bytes(b, n, h, nl, c), what
                assert ab.value == (nl - 1) * b * n * h * 4, what
        if nl == 1:
            assert L.a3vt_gcn_stack_mask_bytes(b, n, h, nl, c) == 0, what
        ld = (fin + 3) // 4 * 4
        assert L.a3vt_gcn_layer_scratch_bytes(b, n, ld, h, c, 1) > L.a3vt_gcn_layer_scratch_bytes(b, n, ld, h, c, 0) > 0, what
        assert L.a3vt_qnet_input_scratch_bytes(b, n, h, c, 1) > L.a3vt_qnet_input_scratch_bytes(b, n, h, c, 0) > 0, what
    assert shapes == 222


def test_entry_points_refuse_bad_arguments_before_touching_them(L):
    f32 = ctypes.c_float
    # BatchNorm + ReLU: fewer than two rows, misaligned maps, one running statistic without the other, short scratch
    need = L.a3vt_bnrelu_scratch_bytes(16)
    args = lambda **kw: [kw.get("x", FAKE), kw.get("rows", 100), kw.get("c", 16), FAKE, FAKE, None, f32(1e-5), f32(0.1),   # noqa: E731
                         kw.get("rm", FAKE), kw.get("rv", FAKE), None, kw.get("y", FAKE), FAKE, FAKE, kw.get("sb", need), None]
    assert L.a3vt_bnrelu_fwd(*args(rows=1)) != 0
    assert L.a3vt_bnrelu_fwd(*args(x=FAKE_ODD)) != 0
    assert L.a3vt_bnrelu_fwd(*args(rv=None)) != 0
    assert L.a3vt_bnrelu_fwd(*args(sb=need - 1)) != 0
    assert L.a3vt_bnrelu_fwd(*args(c=0)) != 0
    assert L.a3vt_bnrelu_bwd(FAKE, None, 100, 16, FAKE, FAKE, FAKE, FAKE, None, FAKE, need, None) != 0
    # batched weight cast: too many tensors; a NULL entry among host arrays of exactly n entries
    n = 3
    src = (ctypes.c_void_p * n)(FAKE.value, None, FAKE.value)
    dst = (ctypes.c_void_p * n)(FAKE.value, FAKE.value, FAKE.value)
    outer = (ctypes.c_longlong * n)(4, 4, 4)
    inner = (ctypes.c_int * n)(3, 3, 3)
    hw = (ctypes.c_int * n)(25, 25, 25)
    assert L.a3vt_cast_weights_bf16(n, src, dst, outer, inner, hw, None) != 0
    assert L.a3vt_cast_weights_bf16(97, src, dst, outer, inner, hw, None) != 0
    assert L.a3vt_cast_weights_bf16(0, None, None, None, None, None, None) == 0
    # bias gradient, stack calls: NULL operands
    assert L.a3vt_bias_grad_nhwc(None, 1, 100, 16, FAKE, FAKE, 1 << 20, None) != 0
    assert L.a3vt_bias_grad_nhwc(FAKE_ODD, 1, 100, 16, FAKE, FAKE, 1 << 20, None) != 0
    assert L.a3vt_gcn_stack_fwd(None, 52, 50, None, None, 20, 300, 99, None, None, None, 7, 2562, 64, 0, None, None, None, None, None) != 0
    assert _err(L) != ""
    assert L.a3vt_gcn_stack_fwd(FAKE, 51, 50, FAKE, FAKE, 20, 300, 99, FAKE, FAKE, FAKE, 7, 2562, 64, 7, None, None, FAKE, FAKE, None) != 0   # mode 7
    # a split with one of its arrays missing, in the exact fp32 and the bf16 storage modes (weights: fake host arrays)
    from a3vt_amd import lib
    for part in ((FAKE, None, None, None), (FAKE, FAKE, FAKE, None), (None, FAKE, FAKE, FAKE)):
        sp = ctypes.byref(lib.AdjSplit(*[p.value if p else None for p in part], 10, 0, 0))
        for mode in (0, 2):
            assert L.a3vt_gcn_stack_fwd_adj(FAKE, 52, 50, FAKE, FAKE, 20, 300, 99, FAKE, FAKE, FAKE, 7, sp, 2562, 64, mode,
                                            FAKE, FAKE, FAKE, FAKE, None) != 0
            assert "argument check failed" in _err(L)
            assert L.a3vt_gcn_stack_bwd_adj(FAKE, 52, 50, FAKE, FAKE, 20, 300, 99, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 7, sp, 2562, 64,
                                            mode, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 0, None) != 0
            assert "argument check failed" in _err(L)
    assert L.a3vt_dbg_csr_algo(9) != 0


def test_conv5_and_adam_entry_points_refuse_bad_arguments(L):
    """Round 6 entry points: the direct convolution's weight gradient and the one-launch optimizer step."""
    # shapes: only the five layer shapes of the pyramid; scratch sizes are 0 for everything else
    assert L.a3vt_conv5_supported(16, 16, 1) == 1 and L.a3vt_conv5_supported(3, 16, 2) == 1 and L.a3vt_conv5_supported(64, 64, 1) == 0
    for cin, cout in ((3, 3), (3, 16), (16, 16), (16, 32), (32, 32)):
        assert L.a3vt_conv5_wrw_scratch_bytes(cin, cout) > 0
    assert L.a3vt_conv5_wrw_scratch_bytes(64, 64) == 0 and L.a3vt_conv5_wrw_scratch_bytes(0, 0) == 0
    need = L.a3vt_conv5_wrw_scratch_bytes(16, 16)
    wg = lambda **kw: [kw.get("x", FAKE), kw.get("gy", FAKE), kw.get("b", 2), kw.get("h", 20), kw.get("w", 20), kw.get("cin", 16),   # noqa: E731
                       kw.get("cout", 16), kw.get("s", 1), kw.get("gw", FAKE), kw.get("scr", FAKE), kw.get("sb", need), None]
    assert L.a3vt_conv5_weight_grad(*wg(x=None)) != 0
    assert L.a3vt_conv5_weight_grad(*wg(gw=None)) != 0
    assert L.a3vt_conv5_weight_grad(*wg(x=FAKE_ODD)) != 0            # 16-channel maps: 16-byte aligned
    assert L.a3vt_conv5_weight_grad(*wg(scr=FAKE_ODD)) != 0
    assert L.a3vt_conv5_weight_grad(*wg(sb=need - 1)) != 0
    assert L.a3vt_conv5_weight_grad(*wg(cin=64, cout=64)) != 0
    assert L.a3vt_conv5_weight_grad(*wg(s=2)) != 0                   # 16 -> 16 exists at stride 1 only
    assert L.a3vt_conv5_weight_grad(*wg(h=2)) != 0 and L.a3vt_conv5_weight_grad(*wg(b=0)) != 0
    assert "argument check failed" in _err(L)
    # Adam: an empty table is a no-op; NULL tables, step 0 and hyper-parameters outside their ranges are refused
    d = ctypes.c_double
    ad = lambda **kw: [kw.get("p", FAKE), FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, kw.get("n", 4), d(kw.get("lr", 3e-4)), d(kw.get("b1", 0.9)),   # noqa: E731
                       d(kw.get("b2", 0.999)), d(1e-8), d(0.0), kw.get("step", 1), None]
    assert L.a3vt_adam_step(None, None, None, None, None, None, None, 0, d(3e-4), d(0.9), d(0.999), d(1e-8), d(0.0), 1, None) == 0
    assert L.a3vt_adam_step(*ad(p=None)) != 0
    assert L.a3vt_adam_step(*ad(step=0)) != 0
    assert L.a3vt_adam_step(*ad(b1=1.0)) != 0 and L.a3vt_adam_step(*ad(b2=-0.1)) != 0 and L.a3vt_adam_step(*ad(lr=-1.0)) != 0
    assert L.a3vt_adam_step(*ad(n=-1)) != 0
    assert L.a3vt_adam_chunk_elems() == 4096


def test_sampling_entry_points_refuse_bad_arguments(L):
    """a3vt_face_cdf, a3vt_sample_points_fwd and a3vt_sample_points_bwd: an empty mesh, an empty draw or a NULL operand is
    refused by the argument check (the backward would otherwise divide by n_vert's tile count on the host); the forward also
    refuses injected faces without their u / v, and a missing CDF when nothing is injected."""
    u64 = ctypes.c_uint64
    cdf = lambda **kw: [kw.get("verts", FAKE), kw.get("faces", FAKE), kw.get("b", 2), kw.get("nv", 162), kw.get("nf", 320),   # noqa: E731
                        kw.get("cdf", FAKE), None]
    fwd = lambda **kw: [kw.get("verts", FAKE), kw.get("faces", FAKE), kw.get("cdf", FAKE), kw.get("b", 2), kw.get("nv", 162),   # noqa: E731
                        kw.get("nf", 320), kw.get("draws", 3), kw.get("num", 100), kw.get("fi", None), kw.get("u", None),
                        kw.get("v", None), u64(1), u64(0), kw.get("pts", FAKE), FAKE, FAKE, FAKE, None]
    bwd = lambda **kw: [kw.get("faces", FAKE), kw.get("b", 2), kw.get("nv", 162), kw.get("nf", 320), kw.get("draws", 3),   # noqa: E731
                        kw.get("num", 100), kw.get("fi", FAKE), kw.get("u", FAKE), kw.get("v", FAKE), kw.get("gp", FAKE),
                        kw.get("gv", FAKE), None]
    for fn, args, sizes, operands in ((L.a3vt_face_cdf, cdf, ("b", "nv", "nf"), ("verts", "faces", "cdf")),
                                      (L.a3vt_sample_points_fwd, fwd, ("b", "nv", "nf", "draws", "num"), ("verts", "faces", "pts")),
                                      (L.a3vt_sample_points_bwd, bwd, ("b", "nv", "nf", "draws", "num"),
                                       ("faces", "fi", "u", "v", "gp", "gv"))):
        for name in sizes:
            for bad in (0, -1):
                assert fn(*args(**{name: bad})) != 0, (fn.__name__, name, bad)
                assert "argument check failed" in _err(L)
        for name in operands:
            assert fn(*args(**{name: None})) != 0, (fn.__name__, name)
            assert "argument check failed" in _err(L)
    assert L.a3vt_sample_points_fwd(*fwd(fi=FAKE)) != 0 and "without u_in/v_in" in _err(L)
    assert L.a3vt_sample_points_fwd(*fwd(fi=FAKE, u=FAKE)) != 0 and "without u_in/v_in" in _err(L)
    assert L.a3vt_sample_points_fwd(*fwd(fi=FAKE, v=FAKE)) != 0 and "without u_in/v_in" in _err(L)
    assert L.a3vt_sample_points_fwd(*fwd(cdf=None)) != 0 and "cdf required" in _err(L)


def test_posenc_entry_points_refuse_bad_arguments(L):
    """The vertex-feature encoder's four entries (csrc/posenc.hip for input_size 50, csrc/posenc_wide.hip for the wide sizes):
    NULL operands, an empty batch, a size the pair does not serve and a row stride the rows do not fit are refused before
    anything is launched.  Rule of the narrow pair (include/a3vt.h): any ld_feats >= input_size, any float-aligned base — so a
    stride of 50 and a base 8 bytes off a 16-byte boundary are NOT argument errors (the backward then loads element by
    element; tests/test_gpu_posenc_edges.py runs both), and nothing here may pass such a call its fake pointers."""
    fwd = lambda **kw: [kw.get("verts", FAKE), kw.get("mask", FAKE), kw.get("m", 100), kw.get("i", 50), kw.get("params", FAKE),   # noqa: E731
                        kw.get("feats", FAKE), kw.get("ld", 52), None]
    bwd = lambda **kw: [kw.get("verts", FAKE), kw.get("mask", FAKE), kw.get("m", 100), kw.get("i", 50), kw.get("params", FAKE),   # noqa: E731
                        kw.get("gfeats", FAKE), kw.get("ld", 52), kw.get("gverts", FAKE), kw.get("gparams", FAKE),
                        kw.get("scratch", FAKE), None]
    wfwd = lambda **kw: [kw.get("verts", FAKE), kw.get("mask", FAKE), kw.get("m", 100), kw.get("i", 448), kw.get("params", FAKE),   # noqa: E731
                         kw.get("feats", FAKE), kw.get("ld", kw.get("i", 448)), kw.get("acts", FAKE), kw.get("scratch", FAKE),
                         kw.get("bf16", 0), None]
    wbwd = lambda **kw: [kw.get("verts", FAKE), kw.get("mask", FAKE), kw.get("m", 100), kw.get("i", 448), kw.get("params", FAKE),   # noqa: E731
                         kw.get("gfeats", FAKE), kw.get("ld", kw.get("i", 448)), kw.get("acts", FAKE), kw.get("gverts", FAKE),
                         kw.get("gparams", FAKE), kw.get("scratch", FAKE), kw.get("bf16", 0), None]
    for fn, args, operands in ((L.a3vt_posenc_mask_fwd, fwd, ("verts", "mask", "params", "feats")),
                               (L.a3vt_posenc_mask_bwd, bwd, ("verts", "mask", "params", "gfeats", "gverts", "gparams", "scratch")),
                               (L.a3vt_posenc_wide_fwd, wfwd, ("verts", "mask", "params", "feats", "acts", "scratch")),
                               (L.a3vt_posenc_wide_bwd, wbwd, ("verts", "mask", "params", "gfeats", "acts", "gverts", "gparams",
                                                               "scratch"))):
        for name in operands:
            assert fn(*args(**{name: None})) != 0, (fn.__name__, name)
            assert "argument check failed" in _err(L)
        for m in (0, -1):
            assert fn(*args(m=m)) != 0, (fn.__name__, m)
            assert "argument check failed" in _err(L)
    # the narrow pair serves input_size 50 only, and a row must hold its 50 columns
    for fn, args in ((L.a3vt_posenc_mask_fwd, fwd), (L.a3vt_posenc_mask_bwd, bwd)):
        for i in (48, 52, 448):
            assert fn(*args(i=i, ld=448)) != 0 and "input_size == 50 only" in _err(L), (fn.__name__, i)
        for ld in (49, 48, 3, 0, -52):
            assert fn(*args(ld=ld)) != 0 and "ld_feats >= input_size" in _err(L), (fn.__name__, ld)
    # the wide pair: sizes it does not serve, and rows with pad columns (ld != input_size)
    for fn, args in ((L.a3vt_posenc_wide_fwd, wfwd), (L.a3vt_posenc_wide_bwd, wbwd)):
        for i in (8, 12, 50, 52, 504, 624, 632, 1032, 0, -16):
            assert fn(*args(i=i)) != 0 and "posenc_wide_supported" in _err(L), (fn.__name__, i)
        for i, ld in ((448, 452), (448, 444), (16, 20), (496, 512)):
            assert fn(*args(i=i, ld=ld)) != 0 and "ld_feats == input_size" in _err(L), (fn.__name__, i, ld)


def test_posenc_size_queries(L):
    """a3vt_posenc_wide_supported: input_size % 8 == 0, 16 <= input_size <= 496 (the last layer's weight gradient must fit the
    rows the weight-gradient kernel can stage; 504 .. 624 used to be admitted, ran their forward and failed in the backward);
    the byte counts are 0 for every other size and for an empty batch."""
    want = {8: 0, 16: 1, 24: 1, 52: 0, 448: 1, 496: 1, 504: 0, 624: 0, 632: 0, 1024: 0, 1032: 0}
    for i, ok in want.items():
        assert L.a3vt_posenc_wide_supported(i) == ok, i
        for back in (0, 1):
            assert (L.a3vt_posenc_wide_scratch_bytes(100, i, back) > 0) == bool(ok), (i, back)
        assert (L.a3vt_posenc_wide_acts_bytes(100, i) > 0) == bool(ok), i
        for m in (0, -1):
            assert L.a3vt_posenc_wide_acts_bytes(m, i) == 0 and L.a3vt_posenc_wide_scratch_bytes(m, i, 1) == 0, (i, m)
    assert [i for i in range(-8, 1100) if L.a3vt_posenc_wide_supported(i)] == list(range(16, 497, 8))
    for i in (16, 448, 496):
        for m in (1, 17, 300):
            assert L.a3vt_posenc_wide_scratch_bytes(m, i, 1) > L.a3vt_posenc_wide_scratch_bytes(m, i, 0) > 0
            # E' (68), H1' and H2' rows of every vertex fit the activation buffer
            assert L.a3vt_posenc_wide_acts_bytes(m, i) >= 4 * m * (68 + (i // 4 + 5) + (i // 2 + 5))
    # the narrow backward's scratch: one slab of packed gradients per workgroup, 4 x 16 vertices each, at most 512
    n = L.a3vt_posenc_param_count(50)
    for m, slabs in ((1, 1), (64, 1), (65, 2), (32768, 512), (32773, 512), (65557, 512)):
        assert L.a3vt_posenc_scratch_bytes(m, 50) == slabs * n * 4, m
    assert L.a3vt_posenc_scratch_bytes(0, 50) == n * 4 and L.a3vt_posenc_scratch_bytes(-5, 50) == n * 4      # never 0, never negative
