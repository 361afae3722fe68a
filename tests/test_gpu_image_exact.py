"""-m gpu: the image pyramid's bf16 kernels — csrc/conv5.hip (5 x 5 convolutions of layers 0-6: forward, input gradients,
weight gradients) and csrc/bnrelu.hip (training BatchNorm2d + ReLU and its backward) — against the float64 references of
``oracle.image`` (anchored on the CPU by tests/test_oracle_image_emulation.py), with bounds tight enough to see a wrong rounding.

A. conv5 on EXACTLY SUMMABLE data: small integers (and weights that are exact bf16 ties), so every product and partial sum
   is an integer multiple of a power of two below 2^24 and fp32 accumulation is exact in any order: the bf16 outputs must be
   the float64 result rounded once to nearest even, bit for bit, and the fp32 weight gradients the exact sums.
B. conv5 on random data: every bf16 output in the rounding interval of the float64 value with a margin from the summation depth.
C. BatchNorm + ReLU against float64, teacher-forced on the device's own statistics and ReLU mask; bounds from the depth of the
   kernels' fp32 sums (the launch geometry of bnrelu_wgs, mirrored below).
D. Every output written, nothing else: all kernels above write into buffers pre-filled with a NaN pattern with guard bands.
E. The autograd wiring of a conv -> BatchNorm + ReLU -> conv chain (Image_Encoder._block_nhwc) against the same references.
"""
import math

import pytest
import torch

from oracle import image as oi

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                  # unit roundoff of fp32 (round to nearest)
PAT16, PAT32 = 0x7FC1, 0x7FC00001   # quiet-NaN patterns no kernel computes from finite inputs
GUARD = 64                      # guard bytes on each side of an output (a multiple of 16: the output stays 16-byte aligned)


def _L():
    from a3vt_amd import lib
    return lib.load()


def _ptr(t):
    from a3vt_amd import lib
    return lib.ptr(t)


def _check(rc, what):
    from a3vt_amd import lib
    lib.check(rc, what)


def _stream():
    from a3vt_amd import ops
    return ops._stream()


class Guarded:
    """An output of ``n`` elements (bf16 or fp32) inside a buffer filled with a NaN pattern, GUARD bytes on both sides."""

    def __init__(self, n, dtype, dev):
        self.int_t, self.pat = (torch.int16, PAT16) if dtype == torch.bfloat16 else (torch.int32, PAT32)
        self.g = GUARD // (2 if dtype == torch.bfloat16 else 4)
        self.n = n
        self.buf = torch.full((self.g + n + self.g,), self.pat, dtype=self.int_t, device=dev)
        self.out = self.buf[self.g:self.g + n].view(dtype)

    def verify(self, what):
        torch.cuda.synchronize()
        b = self.buf
        assert bool((b[:self.g] == self.pat).all()) and bool((b[self.g + self.n:] == self.pat).all()), f"{what}: wrote outside its output"
        left = int((b[self.g:self.g + self.n] == self.pat).sum())
        assert left == 0, f"{what}: {left} of {self.n} output elements never written"
        return self.out


# ---- conv5 through the C ABI -------------------------------------------------------------------------------------------------------
def _nhwc(t, dev):
    """NCHW float values -> a contiguous [B][H][W][C] bf16 device tensor."""
    return t.permute(0, 2, 3, 1).contiguous().to(dev).to(torch.bfloat16)


def _nchw64(t):
    """A [B][H][W][C] device tensor -> NCHW float64 on the CPU."""
    return t.double().cpu().permute(0, 3, 1, 2)


def _image(w, flip):
    from a3vt_amd import ops
    return ops._conv5_image(w, flip)


def conv5_dev(x, w, bias, stride, pad=1, flip=0):
    """a3vt_conv5_nhwc on x [B][H][W][cin] bf16 (flip: the input-gradient form of w, whose cin is then the output) -> NHWC bf16."""
    B, H, W, cin = x.shape
    cout = w.shape[1] if flip else w.shape[0]
    Ho, Wo = (H + 2 * pad - 5) // stride + 1, (W + 2 * pad - 5) // stride + 1
    out = Guarded(B * Ho * Wo * cout, torch.bfloat16, x.device)
    _check(_L().a3vt_conv5_nhwc(_ptr(x), B, H, W, cin, cout, stride, pad, _ptr(_image(w, flip)), _ptr(bias), _ptr(out.out),
                                _stream()), "conv5_nhwc")
    return out.verify(f"conv5 {cin}->{cout} s{stride} pad {pad}").view(B, Ho, Wo, cout)


def up3_dev(gy, w):
    """a3vt_conv5_input_grad_3x16s2: gy [B][ho][wo][16] -> gx [B][2 ho + 2][2 wo + 2][3]."""
    B, ho, wo, _ = gy.shape
    out = Guarded(B * (2 * ho + 2) * (2 * wo + 2) * 3, torch.bfloat16, gy.device)
    _check(_L().a3vt_conv5_input_grad_3x16s2(_ptr(gy), B, ho, wo, _ptr(_image(w, 1)), _ptr(out.out), _stream()), "up3")
    return out.verify("conv5 UP3").view(B, 2 * ho + 2, 2 * wo + 2, 3)


def wgrad_dev(x, gy, cout, stride):
    L = _L()
    B, H, W, cin = x.shape
    need = L.a3vt_conv5_wrw_scratch_bytes(cin, cout)
    scratch = torch.empty(need, dtype=torch.uint8, device=x.device)
    out = Guarded(cout * cin * 25, torch.float32, x.device)
    _check(L.a3vt_conv5_weight_grad(_ptr(x), _ptr(gy), B, H, W, cin, cout, stride, _ptr(out.out), _ptr(scratch), need, _stream()),
           "conv5_weight_grad")
    return out.verify(f"conv5 weight gradient {cin}->{cout} s{stride}").view(cout, cin, 5, 5).double().cpu()


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _tie_weights(shape, g):
    """fp32 weights that are exact bf16 ties: +-2^e (1 + t 2^-8), t odd (nine significant bits), e in {0, 1}; some zeros."""
    t = torch.randint(0, 16, shape, generator=g) * 2 + 1
    e = torch.randint(0, 2, shape, generator=g)
    s = torch.randint(0, 3, shape, generator=g) - 1
    return (s * torch.exp2(e.double()) * (1 + t * 2.0 ** -8)).float()


# (cin, cout, stride, B, H, W): maps off the 16 x 16 forward and 8 x 32 weight-gradient tiles, the smallest maps the launchers
# take, odd and even sizes at stride 2, and the pyramid's own maps at batch 64 on 256^2 images (Image_Encoder.forward: 256 ->
# 254 -> 126 -> 124 -> 122 -> 60 -> 58 -> 56)
EXACT = [(3, 3, 1, 2, 3, 3), (3, 3, 1, 2, 3, 5), (3, 3, 1, 3, 17, 35), (3, 3, 1, 64, 256, 256),
         (3, 16, 2, 2, 3, 3), (3, 16, 2, 2, 5, 4), (3, 16, 2, 3, 37, 30), (3, 16, 2, 2, 36, 41), (3, 16, 2, 64, 254, 254),
         (16, 16, 1, 2, 3, 3), (16, 16, 1, 1, 3, 5), (16, 16, 1, 3, 37, 29), (16, 16, 1, 2, 33, 18), (16, 16, 1, 64, 126, 126),
         (16, 32, 2, 2, 3, 3), (16, 32, 2, 2, 37, 30), (16, 32, 2, 2, 20, 35), (16, 32, 2, 64, 122, 122),
         (32, 32, 1, 2, 3, 5), (32, 32, 1, 3, 23, 31), (32, 32, 1, 1, 18, 17), (32, 32, 1, 64, 60, 60)]


def _exact_case(cin, cout, stride, B, H, W, ties, seed):
    g = torch.Generator().manual_seed(seed)
    big = B * H * W > 2 ** 20
    xr = 2 if big else 4                                   # (keeps the weight-gradient sums below 2^24 on the full maps)
    x = _ints((B, cin, H, W), -xr, xr, g)
    w = _tie_weights((cout, cin, 5, 5), g) if ties else _ints((cout, cin, 5, 5), -3, 3, g).float()
    bias = (torch.randint(-40, 41, (cout,), generator=g).float() * 0.25)   # quarter values: the sum plus bias is not a bf16 value
    return x, w, bias, xr


_EXACT_IDS = lambda c: "{}-{}s{}_{}x{}x{}".format(*c)  # noqa: E731


# (the tie weights on the smaller maps only: the pyramid's maps repeat what those pin, at 2 s of float64 convolution each)
@pytest.mark.parametrize("case,ties", [(c, False) for c in EXACT] + [(c, True) for c in EXACT if c[3] * c[4] * c[5] <= 2 ** 20],
                         ids=lambda v: _EXACT_IDS(v) if isinstance(v, tuple) else ("tie_weights" if v else "int_weights"))
def test_conv5_exact_integer_data(cuda, case, ties):
    cin, cout, stride, B, H, W = case
    x, w, bias, xr = _exact_case(cin, cout, stride, B, H, W, ties, seed=sum(case) + 7 * ties)
    wb = oi.bf16_rne(w.double())                          # the weight image: one rounding to nearest even
    wmax = float(wb.abs().max())
    assert 25 * cin * xr * wmax * 2 ** 8 < 2 ** 24       # every partial sum is an exact fp32 (multiples of 2^-8 at most)
    xd, wd, bd = _nhwc(x, cuda), w.to(cuda), bias.to(cuda)
    ref = oi.conv5_forward(x, wb, None, stride)[0]
    for b in (None, bd):
        y = _nchw64(conv5_dev(xd, wd, b, stride))
        want = oi.bf16_rne(ref + (bias.double().view(1, -1, 1, 1) if b is not None else 0.0))
        bad = int((y != want).sum())
        assert bad == 0, f"forward (bias {b is not None}): {bad} of {y.numel()} outputs differ from one rounding of the exact sum"
    g = torch.Generator().manual_seed(sum(case) + 1)
    gy = _ints(ref.shape, -2, 2, g) if B * H * W <= 2 ** 20 else _ints(ref.shape, -1, 1, g)
    gyd = _nhwc(gy, cuda)
    if not ties:
        # the weight gradient: fp32 output, exact sums of exact products
        assert gy.shape[0] * gy.shape[2] * gy.shape[3] * xr * float(gy.abs().max()) < 2 ** 24
        gw_ref = torch.nn.grad.conv2d_weight(x, w.shape, gy, stride=stride, padding=1)     # (exact: integers below 2^24)
        gw = wgrad_dev(xd, gyd, cout, stride)
        assert torch.equal(gw, gw_ref), float((gw - gw_ref).abs().max())
    if stride == 1 and cin != 3:
        gx = _nchw64(conv5_dev(gyd, wd, None, 1, pad=3, flip=1))
        assert torch.equal(gx, oi.bf16_rne(oi.conv5_input_grad(gy, wb)[0])), "stride-1 input gradient"
    if (cin, cout) == (3, 16) and H % 2 == 0 and W % 2 == 0:
        gx = _nchw64(up3_dev(gyd, wd))
        assert gx.shape == x.shape
        assert torch.equal(gx, oi.bf16_rne(oi.conv5_input_grad_up3(gy, wb)[0])), "layer-1 input gradient (UP3)"


# ---- B: random data -----------------------------------------------------------------------------------------------------------
# Margin of an fp32 sum: |fp32 - exact| <= depth * 2^-24 * sum|terms|, depth = the longest chain of roundings a term passes.
# v_mfma_f32_16x16x32_bf16 multiplies exactly (8 x 8 significant bits) and adds 32 products and its accumulator: at most 6
# roundings deep even if it rounds at every level of a pairwise tree, then one more per later k-step: 13 (16 input channels),
# 25 (32) or 4 (3-channel layers) k-steps -> depth <= 25 + 6, plus the bias add.  KAPPA = 64 is twice that.  The weight
# gradients' residuals (printed below) come from the same instruction and sit far inside such bounds.
KAPPA = 64
RANDOM = [(16, 16, 1, 3, 37, 29), (32, 32, 1, 2, 23, 31), (16, 32, 2, 2, 37, 30), (3, 3, 1, 2, 40, 33), (3, 16, 2, 3, 40, 34),
          (16, 16, 1, 8, 64, 64)]


def _interval_check(dev, val, abs_sum, what, kappa=KAPPA, min_exact=0.85):
    lo, hi = oi.bf16_interval(val, kappa * U * abs_sum)
    ok = oi.in_interval(dev, lo, hi)
    frac = float((lo == hi).double().mean())
    print(f"[{what}] {dev.numel()} outputs, {frac:.3f} with no allowance (lo == hi)")
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} outputs outside their rounding interval"
    assert frac >= min_exact, (what, frac)


@pytest.mark.parametrize("case", RANDOM, ids=_EXACT_IDS)
def test_conv5_random_data_in_rounding_interval(cuda, case):
    cin, cout, stride, B, H, W = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, cin, H, W, generator=g).bfloat16().double()
    w = torch.randn(cout, cin, 5, 5, generator=g) * 0.08
    bias = torch.randn(cout, generator=g) * 0.3
    wb = w.bfloat16().double()          # (fp32 -> bf16: one rounding)
    xd, wd, bd = _nhwc(x, cuda), w.to(cuda), bias.to(cuda)
    for b in (None, bd):
        y = conv5_dev(xd, wd, b, stride)
        val, a = oi.conv5_forward(x, wb, bias if b is not None else None, stride)
        _interval_check(_nchw64(y), val, a, f"forward {cin}->{cout} s{stride} bias {b is not None}")
    gy = torch.randn(val.shape, generator=g).bfloat16().double()
    gyd = _nhwc(gy, cuda)
    if stride == 1 and cin != 3:
        val, a = oi.conv5_input_grad(gy, wb)
        _interval_check(_nchw64(conv5_dev(gyd, wd, None, 1, pad=3, flip=1)), val, a, f"input gradient {cin}<-{cout}")
    if (cin, cout) == (3, 16) and H % 2 == 0 and W % 2 == 0:
        val, a = oi.conv5_input_grad_up3(gy, wb)
        _interval_check(_nchw64(up3_dev(gyd, wd)), val, a, "input gradient UP3")
    # weight gradient: fp32 sums over B Ho Wo pixels (MFMA chains over a workgroup's tiles, then a fixed-order reduce of at
    # most 512 partial images: 16 + 32 additions)
    gw_ref, gw_abs = oi.conv5_weight_grad(x, gy, stride)
    gw = wgrad_dev(xd, gyd, cout, stride)
    res = float(((gw - gw_ref).abs() / (U * gw_abs)).max())
    rel = float((gw - gw_ref).norm() / gw_ref.norm())
    print(f"[weight gradient {cin}->{cout} s{stride}] max |err| / (2^-24 sum|terms|) = {res:.2f}, rel L2 {rel:.2e}")
    assert res <= 256, res
    assert rel < 1e-5, rel


# ---- C: BatchNorm + ReLU ----------------------------------------------------------------------------------------------------------
def _bn_wgs(n_elem, c, per_thread, cap):
    """bnrelu_wgs (csrc/bnrelu.hip): workgroups of a launch."""
    m = c // math.gcd(c, 2048)
    cap = min(cap, 1024)
    want = (n_elem // 8 + 256 * per_thread - 1) // (256 * per_thread)
    n = min(want, cap) // m * m
    return max(n, m)


def _bn_depth(n_elem, c, wgs):
    """Longest chain of fp32 additions behind a per-channel sum of a launch of ``wgs`` workgroups: a thread's register slot
    over its pieces, then bn_fold (a lane butterfly + the four waves; 3 channels: three residues first; other channel counts:
    the owner thread walks the workgroup's slots of its channel), then float64 and one rounding to fp32."""
    pieces = -(-(-(-n_elem // 8)) // (wgs * 256))
    p = c // 8
    if c % 8 == 0 and p <= 64 and (p & (p - 1)) == 0:
        fold = int(math.log2(64 // p)) + 3
    elif c == 3:
        fold = 2 + 6 + 3
    else:
        fold = -(-2048 // c) + 1
    return pieces + fold + 1


def bn_fwd_dev(x, gamma, beta, eps, momentum, rm, rv, nb, pre_bias=None):
    """a3vt_bnrelu_fwd on x [rows][C] bf16 -> (y [rows][C], save [4][C]: mean, invstd, scale, shift)."""
    L = _L()
    rows, C = x.shape
    y = Guarded(rows * C, torch.bfloat16, x.device)
    save = torch.empty(4, C, dtype=torch.float32, device=x.device)
    need = L.a3vt_bnrelu_scratch_bytes(C)
    scratch = torch.zeros(need, dtype=torch.uint8, device=x.device)
    _check(L.a3vt_bnrelu_fwd(_ptr(x), rows, C, _ptr(gamma), _ptr(beta), _ptr(pre_bias), eps, momentum, _ptr(rm), _ptr(rv), _ptr(nb),
                             _ptr(y.out), _ptr(save), _ptr(scratch), need, _stream()), "bnrelu_fwd")
    return y.verify(f"bnrelu_fwd {rows} x {C}").view(rows, C), save


def bn_bwd_dev(dy, x, save):
    L = _L()
    rows, C = x.shape
    dx = Guarded(rows * C, torch.bfloat16, x.device)
    dg, db, cs = (torch.full((C,), float("nan"), device=x.device) for _ in range(3))
    need = L.a3vt_bnrelu_scratch_bytes(C)
    scratch = torch.zeros(need, dtype=torch.uint8, device=x.device)
    _check(L.a3vt_bnrelu_bwd(_ptr(dy), _ptr(x), rows, C, _ptr(save), _ptr(dx.out), _ptr(dg), _ptr(db), _ptr(cs), _ptr(scratch), need,
                             _stream()), "bnrelu_bwd")
    return dx.verify(f"bnrelu_bwd {rows} x {C}").view(rows, C), dg, db, cs


def _col(t):
    """[rows][C] -> (rows, C, 1, 1) float64 on the CPU: the (N, C, H, W) layout of oracle.image."""
    return t.double().cpu().view(t.shape[0], t.shape[1], 1, 1)


def _bn_inputs(rows, C, seed, special):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g) * (torch.rand(C, generator=g) * 2 + 0.3) + torch.randn(C, generator=g) * 2
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.3
    if special and C >= 4:
        x[:, 0] = 1.5                                       # a constant channel: variance 0
        beta[1] = -200.0                                    # pre-activations all negative (|xhat| <= sqrt(rows) < 200)
        x[:, 2] = 200.0 + 2.5 * torch.randn(rows, generator=g)   # |mean| / std = 80
    return x.bfloat16(), gamma, beta


# channel counts: the pyramid's (3 ... 256), the fold forms (power-of-two periods up to 64 pieces, 3 channels, the generic walk)
# and the final kernels' rounds of 256 channels (512, 1000, 1024); odd counts give grids of C / gcd(C, 2048) workgroups.  Row
# counts from 2 up, rows * C not a multiple of 8 (a ragged last piece), and the pyramid's maps at batch 64.
BN_CASES = [(3, 2), (3, 8191), (8, 2), (8, 4099), (16, 8192), (32, 4097), (64, 3000), (128, 1001), (256, 513), (512, 300),
            (1024, 77), (5, 7), (5, 6001), (7, 8191), (48, 35), (48, 5000), (127, 999), (1000, 129),
            (3, 64 * 256 * 256), (3, 64 * 254 * 254), (16, 64 * 126 * 126), (32, 64 * 60 * 60), (64, 64 * 28 * 28)]


@pytest.mark.parametrize("C,rows", BN_CASES, ids=lambda v: str(v))
def test_bnrelu_against_float64(cuda, C, rows):
    eps, momentum = 1e-5, 0.1
    special = 1000 <= rows <= 8192 and C >= 8
    x, gamma, beta = _bn_inputs(rows, C, seed=C * 7 + rows, special=special)
    pre_bias = torch.randn(C) * 0.5 if C % 2 else None
    rm0, rv0 = torch.randn(C) * 0.1, torch.rand(C) + 0.5
    xd, gd, bd = x.to(cuda), gamma.to(cuda), beta.to(cuda)
    rm, rv, nb = rm0.to(cuda), rv0.to(cuda), torch.tensor(5, dtype=torch.int64, device=cuda)
    y, save = bn_fwd_dev(xd, gd, bd, eps, momentum, rm, rv, nb, pre_bias.to(cuda) if pre_bias is not None else None)
    n = rows * C
    X = _col(x)
    ref = oi.bn_relu_forward(X, gamma, beta, eps, momentum, rm0, rv0, pre_bias)
    mean_d, invstd_d, scale_d, shift_d = (save[i].double().cpu() for i in range(4))
    # ---- statistics: fp32 partial sums of depth D of d = x - x[row 0] and d^2 (bnrelu_stats_kernel), then float64
    D = _bn_depth(n, C, _bn_wgs(n, C, 4, max(16, 8192 // C)))
    Dv = X - X[:1]
    sabs, ssq = Dv.abs().sum(dim=(0, 2, 3)), (Dv * Dv).sum(dim=(0, 2, 3))
    md = Dv.mean(dim=(0, 2, 3)).abs()
    e_mean = (D + 1) * U * sabs / rows + U * ref["mean"].abs()
    e_var = (D + 1) * U * ssq / rows + 2 * md * (D + 1) * U * sabs / rows + U * ref["var"]
    assert bool(((mean_d - ref["mean"]).abs() <= e_mean).all()), float((mean_d - ref["mean"]).abs().max())
    var_d = 1.0 / invstd_d ** 2 - eps
    rel_var = (var_d - ref["var"]).abs() / (ref["var"] + eps)
    e_inv = (e_var / (ref["var"] + eps)) / 2 + 8 * U
    assert bool(((invstd_d / ref["invstd"] - 1).abs() <= e_inv).all()), float(((invstd_d / ref["invstd"] - 1).abs() / e_inv).max())
    print(f"[bnrelu {rows} x {C}] depth {D}; variance error relative max {float(rel_var.max()):.2e}")
    if special:
        # |mean| / std = 80: E[x^2] - mean^2 summed as x and x^2 lost 1.5e-4 of the variance here (4 099 x 8); with the pivot
        # the cancellation is gone and the error is that of any channel
        assert float(rel_var[2]) <= 5e-6, float(rel_var[2])
    tm = ref["mean"] + (pre_bias.double() if pre_bias is not None else 0.0)
    e_rm = momentum * (e_mean + 2 * U * tm.abs()) + 4 * U * ref["running_mean"].abs()
    assert bool(((rm.double().cpu() - ref["running_mean"]).abs() <= e_rm + 1e-30).all())
    e_rv = momentum * (e_var * rows / (rows - 1) + 2 * U * ref["var"]) + 4 * U * ref["running_var"].abs()
    assert bool(((rv.double().cpu() - ref["running_var"]).abs() <= e_rv).all())
    assert int(nb) == 6
    # ---- y: in the rounding interval of the float64 value (margin: the statistics' and coefficients' fp32 errors) ...
    sc = (gamma.double() * ref["invstd"]).view(1, -1, 1, 1)
    mu = ref["mean"].view(1, -1, 1, 1)
    m_y = 2 * (sc.abs() * ((e_inv.view(1, -1, 1, 1) + 4 * U) * (X - mu).abs() + e_mean.view(1, -1, 1, 1))
               + 2 * U * ((beta.double().view(1, -1, 1, 1) - mu * sc).abs() + ref["y_pre"].abs()))
    lo, hi = oi.bf16_interval(ref["y_pre"], m_y)
    Y = _col(y)
    ok = (Y >= lo.clamp_min(0)) & (Y <= hi.clamp_min(0))
    print(f"[bnrelu {rows} x {C}] y: {float((lo == hi).double().mean()):.3f} with no allowance")
    assert bool(ok.all()), f"y: {int((~ok).sum())} of {n} outside the rounding interval"
    # ... and, given the device's own coefficients, one fma then one rounding to bf16, bit for bit
    y_emul = torch.relu((X * scale_d.view(1, -1, 1, 1) + shift_d.view(1, -1, 1, 1)).float()).bfloat16().double()
    assert torch.equal(Y, y_emul), int((Y != y_emul).sum())
    # ---- backward, teacher-forced on the device's mask (y > 0) and statistics
    gy = torch.randn(rows, C, generator=torch.Generator().manual_seed(rows + C)).bfloat16()
    dx, dg, db, cs = bn_bwd_dev(gy.to(cuda), xd, save)
    mask = Y > 0
    dx_ref, dg_ref, db_ref, a_dg, a_db = oi.bn_relu_backward(X, _col(gy), mask, gamma, mean_d, invstd_d)
    Db = _bn_depth(n, C, _bn_wgs(n, C, 4, max(16, 8192 // C)))
    e_db = Db * U * a_db + U * db_ref.abs()
    e_dg = (Db + 3) * U * a_dg + U * dg_ref.abs()
    dgc, dbc = dg.double().cpu(), db.double().cpu()
    assert bool(((dbc - db_ref).abs() <= e_db).all()), float(((dbc - db_ref).abs() / e_db.clamp_min(1e-300)).max())
    assert bool(((dgc - dg_ref).abs() <= e_dg).all()), float(((dgc - dg_ref).abs() / e_dg.clamp_min(1e-300)).max())
    # dx = scale g + a x + b, a and b from the device's sums: margin from their error and the coefficients' fp32 roundings
    v = lambda t: t.view(1, -1, 1, 1)  # noqa: E731
    scd = gamma.double() * invstd_d
    xh = (X - v(mean_d)) * v(invstd_d)
    ca = scd * dg_ref * invstd_d / rows
    cb = ca * mean_d - scd * db_ref / rows
    m_dx = 2 * (v(scd.abs()) * (v(e_db) / rows + xh.abs() * v(e_dg) / rows)
                + 6 * U * (v(ca.abs()) * (X.abs() + v(mean_d.abs())) + v(cb.abs()) + v(scd.abs()) * _col(gy).abs() + dx_ref.abs()))
    lo, hi = oi.bf16_interval(dx_ref, m_dx)
    DX = _col(dx)
    ok = (DX >= lo) & (DX <= hi)
    print(f"[bnrelu {rows} x {C}] dx: {float((lo == hi).double().mean()):.3f} with no allowance")
    assert bool(ok.all()), f"dx: {int((~ok).sum())} of {n} outside the rounding interval"
    if special:
        assert float(dgc[1]) == 0.0 and float(dbc[1]) == 0.0 and bool((DX[:, 1] == 0).all())   # the dead channel
    # dx_colsum: the sum of dx AS STORED (bf16), fp32 partial sums of the dx launch's depth
    Dc = _bn_depth(n, C, _bn_wgs(n, C, 4, max(16, 16384 // C)))
    s_ref, s_abs = DX.sum(dim=(0, 2, 3)), DX.abs().sum(dim=(0, 2, 3))
    e_cs = 2 * Dc * U * s_abs + U * s_ref.abs()
    csc = cs.double().cpu()
    assert bool(((csc - s_ref).abs() <= e_cs).all()), float(((csc - s_ref).abs() / e_cs.clamp_min(1e-300)).max())


# ---- E: autograd wiring ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(34, 30), (33, 31)], ids=["even_up3", "odd_miopen"])
def test_conv_bnrelu_conv_chain_gradients(cuda, hw):
    """ConvNHWCFn(add_bias=False) -> BNReLUFn(pre_bias=bias) -> ConvNHWCFn as Image_Encoder._block_nhwc chains layers 1 and 2
    (3 -> 16 stride 2, 16 -> 16), LIBRARY_CONV5 on; every gradient against the float64 references, teacher-forced on the
    device's intermediate tensors."""
    from a3vt_amd import ops
    H, W = hw
    g = torch.Generator().manual_seed(H * W)
    B = 4
    x = torch.randn(B, 3, H, W, generator=g).bfloat16().to(cuda).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    w1 = (torch.randn(16, 3, 5, 5, generator=g) * 0.2).to(cuda).requires_grad_(True)
    b1 = (torch.randn(16, generator=g) * 0.5).to(cuda).requires_grad_(True)
    w2 = (torch.randn(16, 16, 5, 5, generator=g) * 0.08).to(cuda).requires_grad_(True)
    b2 = (torch.randn(16, generator=g) * 0.3).to(cuda).requires_grad_(True)
    gamma = (torch.rand(16, generator=g) + 0.5).to(cuda).requires_grad_(True)
    beta = (torch.randn(16, generator=g) * 0.3).to(cuda).requires_grad_(True)
    rm, rv = torch.zeros(16, device=cuda), torch.ones(16, device=cuda)
    for k in ("conv5_fwd", "conv5_input_grad", "conv5_input_grad_3x16s2", "conv5_weight_grad", "bias_grad_from_bnrelu"):
        ops.STATS[k] = 0
    assert ops.LIBRARY_CONV5[0] and ops.LIBRARY_CONV5_WRW[0]
    h = ops.ConvNHWCFn.apply(x, w1, b1, [2, 2], [1, 1], False)
    h.retain_grad()
    y = ops.BNReLUFn.apply(h, gamma, beta, rm, rv, None, 1e-5, 0.1, b1)
    y.retain_grad()
    out = ops.ConvNHWCFn.apply(y, w2, b2, [1, 1], [1, 1])
    _, save = y.grad_fn.saved_tensors
    save = save.double().cpu()
    gout = torch.randn(out.shape, generator=g).bfloat16().to(cuda).contiguous(memory_format=torch.channels_last)
    out.backward(gout)
    torch.cuda.synchronize()
    assert ops.STATS["conv5_fwd"] == 2 and ops.STATS["conv5_input_grad"] == 1 and ops.STATS["conv5_weight_grad"] == 2
    assert ops.STATS["conv5_input_grad_3x16s2"] == (1 if H % 2 == 0 else 0)
    assert ops.STATS["bias_grad_from_bnrelu"] == 1
    c64 = lambda t: t.detach().double().cpu()  # noqa: E731
    X, Hh, Y, GO, GY, GH = c64(x), c64(h), c64(y), c64(gout), c64(y.grad), c64(h.grad)
    w1b, w2b = c64(w1).bfloat16().double(), c64(w2).bfloat16().double()
    # forward: h without its bias (left to the BatchNorm), running_mean with it
    val, a = oi.conv5_forward(X, w1b, None, 2)
    _interval_check(Hh, val, a, "chain: conv 3->16 s2 forward")
    f = oi.bn_relu_forward(Hh, c64(gamma), c64(beta), 1e-5, 0.1, torch.zeros(16), torch.ones(16), c64(b1))
    torch.testing.assert_close(c64(rm), f["running_mean"], rtol=1e-5, atol=1e-6)
    val, a = oi.conv5_forward(Y, w2b, c64(b2), 1)
    _interval_check(c64(out), val, a, "chain: conv 16->16 forward")
    # conv 2: weight / bias gradients, its input gradient
    gw, ga = oi.conv5_weight_grad(Y, GO, 1)
    assert bool(((c64(w2.grad) - gw).abs() <= 256 * U * ga).all())
    assert bool(((c64(b2.grad) - GO.sum(dim=(0, 2, 3))).abs() <= 1024 * U * GO.abs().sum(dim=(0, 2, 3))).all())   # (bias_grad_nhwc)
    val, a = oi.conv5_input_grad(GO, w2b)
    _interval_check(GY, val, a, "chain: conv 16<-16 input gradient")
    # BatchNorm + ReLU backward, teacher-forced on the device's mask and statistics; the bias gradient of conv 1 = the column
    # sum of the stored bf16 dx
    dx_ref, dg_ref, db_ref, a_dg, a_db = oi.bn_relu_backward(Hh, GY, Y > 0, c64(gamma), save[0], save[1])
    assert bool(((c64(beta.grad) - db_ref).abs() <= 64 * U * a_db).all())
    assert bool(((c64(gamma.grad) - dg_ref).abs() <= 64 * U * a_dg).all())
    rel = float((GH - dx_ref).norm() / dx_ref.norm())
    assert rel < 4e-3, rel                                 # (one bf16 rounding; the elementwise check is test_bnrelu_against_float64)
    assert bool(((c64(b1.grad) - GH.sum(dim=(0, 2, 3))).abs() <= 64 * U * GH.abs().sum(dim=(0, 2, 3))).all())
    # conv 1: weight gradient, and the input gradient (UP3 at even sizes, MIOpen at odd ones)
    gw, ga = oi.conv5_weight_grad(X, GH, 2)
    assert bool(((c64(w1.grad) - gw).abs() <= 256 * U * ga).all())
    if H % 2 == 0:
        val, a = oi.conv5_input_grad_up3(GH, w1b)
        _interval_check(c64(x.grad), val, a, "chain: conv 3<-16 s2 input gradient (UP3)")
    else:
        ref = torch.nn.grad.conv2d_input(X.shape, w1b, GH, stride=2, padding=1)
        rel = float((c64(x.grad) - ref).norm() / ref.norm())
        assert rel < 8e-3, rel


def test_image_encoder_wide_batchnorm_falls_back(cuda):
    """A BatchNorm of more than _BNRELU_MAX_C channels is not fused (BNReLUFn would refuse it): the block runs on MIOpen's
    BatchNorm, and the convolution in front keeps its own bias (no pre_bias to carry it into running_mean)."""
    from types import SimpleNamespace
    from torch import nn
    from a3vt_amd import ops
    from a3vt_amd.pterotactyl.reconstruction.vision import model
    args = SimpleNamespace(CNN_ker_size=5, num_CNN_blocks=6, layers_per_block=3, gemm_precision="bf16s")
    torch.manual_seed(4)
    enc = model.Image_Encoder(args).to(cuda).train()
    C = ops._BNRELU_MAX_C + 16
    conv0 = nn.Conv2d(3, C, 5, padding=1)
    with torch.no_grad():
        conv0.bias.fill_(3.0)
    enc.layers = nn.ModuleList([nn.Sequential(nn.BatchNorm2d(3), nn.ReLU(), conv0),
                                nn.Sequential(nn.BatchNorm2d(C), nn.ReLU(), nn.Conv2d(C, 4, 5, padding=1))]).to(cuda).train()
    assert not model.Image_Encoder._bn_fusable(enc.layers[1][0], torch.empty(0, dtype=torch.bfloat16))
    img = torch.rand(4, 3, 14, 14, device=cuda)
    maps = enc(img)
    sum(m.float().sum() for m in maps).backward()
    torch.cuda.synchronize()
    assert conv0.weight.grad is not None and conv0.bias.grad is not None
    # running_mean of the wide BatchNorm: 0.1 x the batch mean of conv0's output, bias included (3.0 + a small mean)
    with torch.no_grad():
        h = nn.functional.conv2d(nn.functional.relu(nn.functional.batch_norm(img, None, None, enc.layers[0][0].weight,
                                                                              enc.layers[0][0].bias, True)),
                                 conv0.weight, conv0.bias, padding=1)
    torch.testing.assert_close(enc.layers[1][0].running_mean, 0.1 * h.mean(dim=(0, 2, 3)), rtol=2e-2, atol=2e-3)
