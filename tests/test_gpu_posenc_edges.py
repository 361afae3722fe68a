"""The vertex-feature encoder kernels at their edges: csrc/posenc.hip (input_size 50: scalar forward, persistent MFMA
backward) and csrc/posenc_wide.hip (augmented products on rowgemm / dw) against the rounding-aware float64 reference of
tests/posenc_ref.py — elementwise, every tensor on its own largest reference element (helpers.rel_err).

Bounds = 16 x the error of the same formula evaluated in float32 on the CPU (tests/test_posenc_ref_host.py measures, prints
and asserts the figures; the margin covers device sinf / cosf against the host's, MFMA chains against sequential sums and
the slab-order sums):

    tensor                                        float32 CPU, measured      figure cited   bound (x 16)   old bound
    features                                      9.42e-8 (I = 50, 65 557)   9.5e-8         1.52e-6        1e-5
    grad_verts                                    5.33e-7 (I = 496)          5.4e-7         8.64e-6        1e-4
    dW1 db1 dW2 db2 dW3 db3, each, m <= 2048      4.92e-7 (dW1, I = 496)     5.0e-7         8.0e-6         1e-4 (packed, max-norm)
    the same, m > 2048 (sums of 65 557 rows)      1.69e-6 (db1)              1.7e-6         2.72e-5        1e-4 (packed, max-norm)
    dEmb, m <= 2048                               1.44e-7                    1.5e-7         2.4e-6         1e-4 (packed, max-norm)
    dEmb, m > 2048                                8.44e-7                    8.5e-7         1.36e-5        1e-4 (packed, max-norm)

On the MI355X the kernels come in at: features <= 1.5e-7, grad_verts <= 5.6e-7 (I = 496; 2.3e-7 at I = 50), every weight /
bias gradient <= 6.1e-7 and dEmb <= 1.8e-7 over all the cases of this file, large m included (MFMA tiles and slab sums grow slower than a row-after-row
sum) — no bound had to be widened.

Gradients are compared after the upstream-gradient rows of near-kink vertices (any |pre-activation| < tau = 1e-6) have been
zeroed by posenc_ref.make_case, which asserts that at most 1e-3 of the rows are; where tau comes from is written there.
Observed share of zeroed rows (seed 1 throughout): none in every case below m = 1551 (one row of 300 would be over the cap);
one vertex, 6.4e-4, at m = 1551 and 3 x 517; 2.1e-4 at m = 32 768 / 32 773; 1.4e-4 at m = 65 557 (1.2e-4 at |p| <= 1.5).
Each test prints its case's share and every figure before it asserts.
"""
import ctypes
import functools

import pytest
import torch

import posenc_ref as R
from helpers import rel_err

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = 0x5EED5EED      # guard words around the buffers of the direct calls (as int32)


# ------------------------------------------------------------------------------------------------ cases (built once, never changed)
@functools.lru_cache(maxsize=None)
def narrow_case(B, N, ld=52, seed=1, pmax=0.3, kind="plain"):
    m = B * N
    mask = gscale = params = None
    tau = R.TAU
    if kind == "rounds":          # the rounds of the persistent loop differ starkly: anything a wave carries from tile to tile shows
        first = torch.arange(m) < 32768
        mask = torch.where(first, 3.0, 0.0)
        gscale = torch.where(first, 1.0, 1e-3)
    elif kind.startswith("token"):
        mask = torch.full((m,), float(kind[5:]))
    elif kind == "hand":
        mask = torch.tensor(R.HAND_MASK).repeat(m // 10)
    elif kind in ("w1zero", "w1zero_b2zeros"):
        # W1 = 0, b1 = 0: every first-layer pre-activation is EXACTLY zero in the kernels and in the reference alike (sums of
        # exact zeros), and every second-layer one is exactly b2: nothing lies "within rounding" of a kink, so tau = 0
        params = R.make_params(50, seed + 17)
        params[0].zero_()
        params[1].zero_()
        if kind == "w1zero_b2zeros":
            params[3][::3] = 0.0
        tau = 0.0
    return R.make_case(B, N, 50, ld, seed, pmax, mask, params, gscale, tau)


@functools.lru_cache(maxsize=None)
def wide_case(I, m, kind="plain"):
    mask = None
    if kind.startswith("token"):
        mask = torch.full((m,), float(kind[5:]))
    elif kind == "hand":
        mask = torch.tensor(R.HAND_MASK).repeat(m // 10)
    pmax = 1.5 if m in (17, 300) else 0.3
    return R.make_case(1, m, I, I, 1, pmax, mask)


# ------------------------------------------------------------------------------------------------ running and checking
def run(case, cuda, gout=None):
    from a3vt_amd import ops
    packed = case["packed"].to(cuda).requires_grad_(True)
    vd = case["verts"].to(cuda).requires_grad_(True)
    f = ops.PosEncMaskFn.apply(vd, case["mask"].to(cuda), packed, case["I"], case["ld"])
    f.backward((case["gout"] if gout is None else gout).to(cuda))
    return f.detach(), vd.grad, packed.grad


def same_bits(a, b):
    return all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


def check(case, out, what, segments=None, emb_rows=False):
    """Features, grad_verts (per segment of vertices, each on its own scale) and the seven parameter gradients against the
    reference, each within its bound; forward pad columns exactly zero.  Returns the unpacked parameter gradients."""
    f, gv, gp = out
    I, m, ref = case["I"], case["B"] * case["N"], case["ref"]
    f = f.reshape(m, -1)
    figs = [("feats", rel_err(f[:, :I], ref["feats"]), R.BOUNDS["feats"])]
    for a, b in segments or [(0, m)]:
        figs.append((f"grad_verts[{a}:{b}]", rel_err(gv.reshape(m, 3)[a:b], ref["grad_verts"][a:b]), R.BOUNDS["grad_verts"]))
    grads = R.unpack(gp.cpu(), I)
    size = "" if m <= 2048 else "_large"
    emb_bound = R.BOUNDS["emb" + size]
    for n, a, b in zip(R.SHORT, grads, ref["grad_params"]):
        assert a.shape == b.shape
        figs.append((n, rel_err(a, b), emb_bound if n == "dEmb" else R.BOUNDS["weights" + size]))
    if emb_rows:
        for t in range(4):
            if ref["grad_params"][6][t].abs().max() > 0:
                figs.append((f"dEmb[{t}]", rel_err(grads[6][t], ref["grad_params"][6][t]), emb_bound))
    print(f"\n{what}: m={m} I={I} ld={case['ld']} zeroed rows {case['kink_share']:.1e}  "
          + "  ".join(f"{n} {v:.1e}" for n, v, _ in figs))
    if f.shape[1] > I:
        assert f[:, I:].abs().max().item() == 0.0 and not torch.signbit(f[:, I:]).any(), "forward pad columns must be +0.0"
    for n, v, bound in figs:
        assert v < bound, f"{what}: {n} {v:.2e} >= {bound:.2e}"
    return grads


def poison_workspace(cuda, nbytes):
    from a3vt_amd import ops
    ops.workspace("posenc", nbytes, cuda).view(torch.uint8).fill_(0xFF)


def narrow_scratch_bytes(m):
    from a3vt_amd import lib
    return lib.load().a3vt_posenc_scratch_bytes(m, 50)


# ------------------------------------------------------------------------------------------------ narrow kernel, I = 50
@pytest.mark.parametrize("B,N", [(1, 1), (1, 15), (1, 16), (1, 17), (1, 48), (1, 64), (1, 65), (3, 7)])
def test_narrow_small_m_ladder(cuda, B, N):
    """One vertex, one short of a tile, a tile, one over; a workgroup with idle waves (m <= 48), exactly full, one over."""
    case = narrow_case(B, N)
    check(case, run(case, cuda), f"narrow {B}x{N}")


@pytest.mark.parametrize("m", [32768, 32773, 65557])
def test_narrow_persistent_rounds(cuda, m):
    """32 768: every wave of the 512-workgroup grid takes exactly one tile; 32 773: wave 0 takes a second one with 5 live and 11
    dead vertices; 65 557: every wave a second, two a third, the last ragged.  First-round vertices carry token 3 and gradients
    of order 1, the rest token 0 and gradients of order 1e-3, and grad_verts / the embedding rows are compared per round on
    their own scale — so what a wave's rows (dE over G's columns 52..63, the one-hot columns, dead lanes) carry from one tile to
    the next would show.  Bit-repeatable, and independent of what the shared workspace held."""
    case = narrow_case(1, m, kind="rounds")
    out = run(case, cuda)
    segs = [(0, 32768)] + ([(32768, m)] if m > 32768 else [])
    grads = check(case, out, f"narrow rounds m={m}", segments=segs, emb_rows=True)
    assert grads[6][1].abs().max() == 0 and grads[6][2].abs().max() == 0          # tokens nobody uses
    if m == 32768:
        assert grads[6][0].abs().max() == 0
    assert same_bits(run(case, cuda), out)
    poison_workspace(cuda, narrow_scratch_bytes(m))
    assert same_bits(run(case, cuda), out)


@pytest.mark.parametrize("ld", [50, 52, 64])
@pytest.mark.parametrize("m", [17, 1551])
def test_narrow_row_strides(cuda, m, ld):
    """ld = 52 is the models' stride; 64 leaves columns the backward never reads; 50 has no pad column and puts every odd
    gradient row 8 bytes off a 16-byte boundary (the backward then loads element by element: include/a3vt.h)."""
    case = narrow_case(1, m, ld=ld)
    out = run(case, cuda)
    assert out[0].shape == (1, m, ld)
    check(case, out, f"narrow ld={ld}")
    assert same_bits(out[1:], run(narrow_case(1, m, ld=52), cuda)[1:])      # same inputs, same sums: the stride changes no bit


@pytest.mark.parametrize("ld", [52, 64])
@pytest.mark.parametrize("fill", [NAN, 1e30], ids=["nan", "1e30"])
def test_narrow_upstream_pad_columns_are_never_used(cuda, ld, fill):
    for m in (17, 1551):
        case = narrow_case(1, m, ld=ld)
        base = run(case, cuda)
        g = case["gout"].clone()
        g[..., 50:] = fill
        out = run(case, cuda, gout=g)
        assert same_bits(out[1:], base[1:]), f"m={m}: pad columns of the upstream gradient reached a result"


@pytest.mark.parametrize("tok", [0, 1, 2, 3])
def test_narrow_single_token_leaves_the_other_embedding_rows_zero(cuda, tok):
    case = narrow_case(1, 300, kind=f"token{tok}")
    grads = check(case, run(case, cuda), f"narrow all-token-{tok}")
    for t in range(4):
        if t != tok:
            assert grads[6][t].abs().max().item() == 0.0, f"embedding row {t} has no vertex"


def test_narrow_tokens_truncate_and_clamp(cuda):
    case = narrow_case(1, 130, kind="hand")          # [-2, -0.5, 0, 0.9, 1.5, 2.999, 3, 3.7, 7, 1e6] x 13
    assert case["ref"]["tok"][:10].tolist() == [0, 0, 0, 0, 1, 2, 3, 3, 3, 3]
    check(case, run(case, cuda), "narrow hand-written mask", emb_rows=True)


@pytest.mark.parametrize("kind", ["w1zero", "w1zero_b2zeros"])
def test_narrow_exact_relu_zeros(cuda, kind):
    """relu'(0) = 0: with W1 = 0 and b1 = 0 every first-layer pre-activation is exactly 0, so dW1, db1 and grad_verts are
    exactly 0; units of the second layer whose bias is exactly 0 then sit at exactly 0 as well and get no gradient."""
    case = narrow_case(1, 300, kind=kind)
    assert case["ref"]["pre1"].abs().max() == 0
    out = run(case, cuda)
    grads = check(case, out, f"narrow {kind}")
    assert out[1].abs().max().item() == 0.0 and grads[0].abs().max().item() == 0.0 and grads[1].abs().max().item() == 0.0
    assert grads[2].abs().max().item() == 0.0                      # dW2 = dh2^T h1, h1 = 0
    if kind == "w1zero_b2zeros":
        dead = case["params"][3] == 0
        assert dead.sum() == 9 and (case["ref"]["pre2"][:, dead] == 0).all()
        assert grads[3][dead].abs().max().item() == 0.0 and grads[4][:, dead].abs().max().item() == 0.0
        assert grads[3][~dead & (case["params"][3] > 0)].abs().min().item() > 0.0


@pytest.mark.parametrize("m", [1551, 65557])
def test_narrow_positions_to_1p5(cuda, m):
    """|p| <= 1.5: sin / cos arguments up to 18 pi x 1.5 = 85 rad, formed as a float32 product of a float32 frequency."""
    case = narrow_case(1, m, pmax=1.5)
    check(case, run(case, cuda), f"narrow |p|<=1.5 m={m}")


@pytest.mark.parametrize("B,N", [(1, 17), (3, 517), (1, 65557)])
def test_narrow_repeatable_and_independent_of_the_workspace(cuda, B, N):
    case = narrow_case(B, N)
    out = run(case, cuda)
    check(case, out, f"narrow {B}x{N}")
    assert same_bits(run(case, cuda), out)
    poison_workspace(cuda, narrow_scratch_bytes(B * N))
    assert same_bits(run(case, cuda), out)


def _guarded(n, cuda, lead=64):
    """n float32 words between `lead` and 64 sentinel words; (whole buffer as int32, the view)."""
    whole = torch.full((lead + n + 64,), SENTINEL, dtype=torch.int32, device=cuda)
    return whole, whole[lead:lead + n].view(torch.float32)


def _intact(whole, n, lead=64):
    return bool((whole[:lead] == SENTINEL).all() and (whole[lead + n:] == SENTINEL).all())


def _nan_tailed(t, cuda, lead=0):
    """t's elements at float offset `lead` of a buffer that is NaN before and for 16 x 64 floats after."""
    flat = t.reshape(-1)
    buf = torch.full((lead + flat.numel() + 1024,), NAN, dtype=torch.float32, device=cuda)
    buf[lead:lead + flat.numel()] = flat.to(cuda)
    return buf, buf[lead:lead + flat.numel()]


@pytest.mark.parametrize("ld,goff", [(52, 0), (52, 2), (50, 0), (50, 1)], ids=["ld52", "ld52-base8B", "ld50", "ld50-base4B"])
@pytest.mark.parametrize("m", [17, 32773])
def test_narrow_direct_calls_stay_inside_their_buffers(cuda, m, ld, goff):
    """The C entries themselves: every output and the scratch sit between sentinel words, every input is followed by NaN rows
    (a read past m would poison a parameter gradient through 0 x NaN), and grad_feats starts `goff` floats off a 16-byte
    boundary (the backward's element path)."""
    from a3vt_amd import lib
    L = lib.load()
    case = narrow_case(1, m, ld=ld, kind="rounds" if m > 32768 else "plain")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nparam = L.a3vt_posenc_param_count(50)
    nscr = L.a3vt_posenc_scratch_bytes(m, 50) // 4
    keep = [_nan_tailed(case["verts"], cuda), _nan_tailed(case["mask"], cuda), _nan_tailed(case["gout"], cuda, lead=4 + goff)]
    verts, mask, gfeats = (v for _, v in keep)
    assert gfeats.data_ptr() % 16 == 4 * goff
    packed = case["packed"].to(cuda)
    (wf, feats), (wv, gv), (wp, gp), (ws, scr) = (_guarded(n, cuda) for n in (m * ld, m * 3, nparam, nscr))
    lib.check(L.a3vt_posenc_mask_fwd(lib.ptr(verts), lib.ptr(mask), m, 50, lib.ptr(packed), lib.ptr(feats), ld, stream), "fwd")
    lib.check(L.a3vt_posenc_mask_bwd(lib.ptr(verts), lib.ptr(mask), m, 50, lib.ptr(packed), lib.ptr(gfeats), ld, lib.ptr(gv),
                                     lib.ptr(gp), lib.ptr(scr), stream), "bwd")
    torch.cuda.synchronize()
    assert _intact(wf, m * ld) and _intact(wv, m * 3) and _intact(wp, nparam) and _intact(ws, nscr)
    segs = [(0, 32768), (32768, m)] if m > 32768 else None
    check(case, (feats.reshape(1, m, ld), gv.reshape(1, m, 3), gp), f"narrow direct m={m} ld={ld} goff={goff}", segments=segs)
    # the same bits as through the autograd function, whichever way the gradient rows were loaded
    assert same_bits((feats.reshape(1, m, ld), gv.reshape(1, m, 3), gp), run(case, cuda))


# ------------------------------------------------------------------------------------------------ wide kernel
@pytest.mark.parametrize("m", [1, 17, 129, 300])
@pytest.mark.parametrize("I", [16, 24, 496])
def test_wide_sizes(cuda, I, m):
    """The smallest supported size, the next one and the largest (496: the last layer's weight gradient stages 256-float H2'
    rows beside 496-float gradient rows, all that dw_kernel's stage holds); |p| <= 1.5 at m = 17 and 300.  Per-tensor
    gradients, bit-repeatable, independent of a poisoned workspace."""
    from a3vt_amd import lib
    case = wide_case(I, m)
    out = run(case, cuda)
    check(case, out, f"wide I={I}")
    assert same_bits(run(case, cuda), out)
    poison_workspace(cuda, lib.load().a3vt_posenc_wide_scratch_bytes(m, I, 1))
    assert same_bits(run(case, cuda), out)


@pytest.mark.parametrize("I", [16, 496])
def test_wide_independent_of_poisoned_activation_and_scratch_buffers(cuda, I):
    """Direct calls with `acts` and `scratch` of exactly the advertised sizes (between sentinel words) filled with 0x00 and
    then 0xFF bytes: the same bits as through the autograd function.  (Through ops the activation buffer is a fresh
    torch.empty whose contents the caching allocator decides; the direct call is the arrangement that does not depend on it.)"""
    from a3vt_amd import lib
    L = lib.load()
    m = 129
    case = wide_case(I, m)
    ref_out = run(case, cuda)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    verts, mask, gfeats, packed = (case[k].to(cuda).contiguous() for k in ("verts", "mask", "gout", "packed"))
    nacts, nscr = L.a3vt_posenc_wide_acts_bytes(m, I) // 4, L.a3vt_posenc_wide_scratch_bytes(m, I, 1) // 4
    assert nacts > 0 and nscr >= L.a3vt_posenc_wide_scratch_bytes(m, I, 0) // 4 > 0
    for byte in (0x00, 0xFF):
        (wa, acts), (ws, scr) = _guarded(nacts, cuda), _guarded(nscr, cuda)
        acts.view(torch.uint8).fill_(byte)
        scr.view(torch.uint8).fill_(byte)
        (wf, feats), (wv, gv), (wp, gp) = (_guarded(n, cuda) for n in (m * I, m * 3, packed.numel()))
        lib.check(L.a3vt_posenc_wide_fwd(lib.ptr(verts), lib.ptr(mask), m, I, lib.ptr(packed), lib.ptr(feats), I, lib.ptr(acts),
                                         lib.ptr(scr), 0, stream), "wide fwd")
        scr.view(torch.uint8).fill_(byte)               # the scratch is free between the two calls
        lib.check(L.a3vt_posenc_wide_bwd(lib.ptr(verts), lib.ptr(mask), m, I, lib.ptr(packed), lib.ptr(gfeats), I, lib.ptr(acts),
                                         lib.ptr(gv), lib.ptr(gp), lib.ptr(scr), 0, stream), "wide bwd")
        torch.cuda.synchronize()
        assert _intact(wa, nacts) and _intact(ws, nscr) and _intact(wf, m * I) and _intact(wv, m * 3) and _intact(wp, packed.numel())
        assert same_bits((feats.reshape(1, m, I), gv.reshape(1, m, 3), gp), ref_out), f"buffers filled with {byte:#x}"


@pytest.mark.parametrize("tok", [0, 1, 2, 3])
def test_wide_single_token_leaves_the_other_embedding_rows_zero(cuda, tok):
    case = wide_case(24, 129, kind=f"token{tok}")
    grads = check(case, run(case, cuda), f"wide all-token-{tok}")
    for t in range(4):
        if t != tok:
            assert grads[6][t].abs().max().item() == 0.0, f"embedding row {t} has no vertex"


def test_wide_tokens_truncate_and_clamp(cuda):
    case = wide_case(16, 130, kind="hand")
    check(case, run(case, cuda), "wide hand-written mask", emb_rows=True)


@pytest.mark.parametrize("I", [8, 12, 52, 504, 624, 632, 1032])
def test_wide_unsupported_sizes_raise_and_launch_nothing(cuda, I):
    from a3vt_amd import lib, ops
    L = lib.load()
    m = 5
    assert L.a3vt_posenc_wide_supported(I) == 0
    assert L.a3vt_posenc_wide_acts_bytes(m, I) == 0 and L.a3vt_posenc_wide_scratch_bytes(m, I, 1) == 0
    packed = torch.zeros(L.a3vt_posenc_param_count(I), device=cuda)
    verts, mask = torch.zeros(1, m, 3, device=cuda), torch.zeros(1, m, 1, device=cuda)
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.PosEncMaskFn.apply(verts, mask, packed, I, I)
    # the C entries refuse too, and nothing they were given is written
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    bufs = [_guarded(n, cuda, lead=0) for n in (m * I, m * 3, packed.numel(), 4096, 4096)]
    for whole, _ in bufs:
        whole.fill_(SENTINEL)
    feats, gv, gp, acts, scr = (v for _, v in bufs)
    gfeats = torch.ones(m, I, device=cuda)
    assert L.a3vt_posenc_wide_fwd(lib.ptr(verts), lib.ptr(mask), m, I, lib.ptr(packed), lib.ptr(feats), I, lib.ptr(acts),
                                  lib.ptr(scr), 0, stream) != 0
    assert L.a3vt_posenc_wide_bwd(lib.ptr(verts), lib.ptr(mask), m, I, lib.ptr(packed), lib.ptr(gfeats), I, lib.ptr(acts),
                                  lib.ptr(gv), lib.ptr(gp), lib.ptr(scr), 0, stream) != 0
    torch.cuda.synchronize()
    assert all(bool((whole == SENTINEL).all()) for whole, _ in bufs)
