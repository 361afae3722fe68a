"""GPU tests of ``a3vt_conv5f_nhwc`` (csrc/conv5f.hip) alone, against an fp64 direct convolution written here.

Bound per element (derived, not measured): with s = sum x w and a = sum |x| |w| in fp64 and K = 25 cin terms, ANY fp32 summation
order gives |fl(s) - s| <= gamma_K a; the epilogue adds two roundings; ReLU is 1-Lipschitz.  So
    |y - act(scale s + shift)| <= (K + 8) 2^-24 (|scale| a + |shift|).
Borders are checked exactly (all-ones data: small integers), as are repeatability and independence of the batch."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(3, 16, 2), (16, 16, 1), (16, 32, 2), (32, 32, 1), (32, 32, 2)]          # (cin, cout, stride)
SIZES = [(5, 5), (6, 9), (17, 16), (31, 29), (61, 61)]                              # (H, W): below, at and off any tile edge
# (H, W, B, pad): every size at pad 2 with B = 1 and 3, one case without padding and one with the largest
GEOMETRIES = [(h, w, b, 2) for (h, w) in SIZES for b in (1, 3)] + [(17, 16, 1, 0), (6, 9, 3, 4)]
U = 2.0 ** -24


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def out_size(n, pad, stride):
    return (n + 2 * pad - 5) // stride + 1


def conv5f(x, w, stride, pad, scale=None, shift=None, relu=0):
    """The kernel on device tensors: x (B,H,W,cin), w (cout,cin,5,5) -> (B,Ho,Wo,cout)."""
    from a3vt_amd import lib
    L = lib.load()
    B, H, W, cin = x.shape
    cout = w.shape[0]
    img = torch.empty(L.a3vt_conv5f_image_bytes(cin, cout), dtype=torch.uint8, device=x.device)
    lib.check(L.a3vt_conv5f_weight_image(_ptr(w), cout, cin, _ptr(img), _stream()), "conv5f_weight_image")
    y = torch.full((B, out_size(H, pad, stride), out_size(W, pad, stride), cout), float("nan"), device=x.device)
    lib.check(L.a3vt_conv5f_nhwc(_ptr(x), B, H, W, cin, cout, stride, pad, _ptr(img), _ptr(scale), _ptr(shift), relu, _ptr(y),
                                 _stream()), "conv5f_nhwc")
    return y


def direct_conv64(x, w, stride, pad):
    """fp64 direct convolution on the CPU: s = sum x w and a = sum |x| |w| per output element, (B,Ho,Wo,cout) each."""
    x, w = x.double().cpu(), w.double().cpu()
    B, H, W, cin = x.shape
    Ho, Wo = out_size(H, pad, stride), out_size(W, pad, stride)
    xp = torch.zeros(B, H + 2 * pad, W + 2 * pad, cin, dtype=torch.float64)
    xp[:, pad:pad + H, pad:pad + W] = x
    s = torch.zeros(B, Ho, Wo, w.shape[0], dtype=torch.float64)
    a = torch.zeros_like(s)
    for ky in range(5):
        for kx in range(5):
            win = xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]      # (B,Ho,Wo,cin)
            s += torch.einsum("bhwc,oc->bhwo", win, w[:, :, ky, kx])
            a += torch.einsum("bhwc,oc->bhwo", win.abs(), w[:, :, ky, kx].abs())
    return s, a


@functools.lru_cache(maxsize=None)
def problem(shape, geometry):
    """Seeded inputs of a case and their fp64 sums (computed once, shared by the tests, never modified)."""
    cin, cout, stride = shape
    H, W, B, pad = geometry
    g = torch.Generator().manual_seed(1000 * cin + 100 * stride + 10 * H + W + B + pad)
    x = torch.randn(B, H, W, cin, generator=g)
    w = torch.randn(cout, cin, 5, 5, generator=g) / (25 * cin) ** 0.5
    scale = torch.randn(cout, generator=g) + 0.25          # both signs
    shift = torch.randn(cout, generator=g)
    assert (scale < 0).any() and (scale > 0).any()
    s, a = direct_conv64(x, w, stride, pad)
    return x, w, scale, shift, s, a


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dto%ds%d" % s)
def test_against_fp64_direct_convolution(cuda, shape):
    cin, cout, stride = shape
    K = 25 * cin
    for geometry in GEOMETRIES:
        x, w, scale, shift, s, a = problem(shape, geometry)
        xd, wd, scd, shd = x.to(cuda), w.to(cuda), scale.to(cuda), shift.to(cuda)
        for relu, affine in ((1, True), (0, True), (0, False), (1, False)):
            y = conv5f(xd, wd, stride, geometry[3], scd if affine else None, shd if affine else None, relu).double().cpu()
            want = scale.double() * s + shift.double() if affine else s.clone()
            bound = (K + 8) * U * ((scale.double().abs() * a + shift.double().abs()) if affine else a)
            if relu:
                want = want.clamp_min(0.0)
            assert y.shape == want.shape
            assert torch.isfinite(y).all(), f"{shape} {geometry}: an output element was not written"
            err = (y - want).abs()
            worst = (err / bound.clamp_min(1e-300)).max().item()
            print(f"{shape} {geometry} relu={relu} affine={affine}: max err {err.max().item():.3e}, worst err / bound {worst:.3f}")
            assert (err <= bound).all(), f"{shape} {geometry} relu={relu} affine={affine}: err / bound = {worst:.3f}"
            if relu:
                assert (y >= 0).all()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dto%ds%d" % s)
def test_borders_exact(cuda, shape):
    """All-ones data: every output is cin x (the number of taps inside the map), an integer <= 800 — compared with ==."""
    cin, cout, stride = shape
    for (H, W, B, pad) in ((6, 9, 1, 2), (17, 16, 2, 2), (61, 61, 1, 2), (6, 9, 1, 4), (5, 5, 1, 0), (31, 29, 1, 1)):
        y = conv5f(torch.ones(B, H, W, cin, device=cuda), torch.ones(cout, cin, 5, 5, device=cuda), stride, pad).cpu()
        inside = lambda n, o: sum(1 for k in range(5) if 0 <= o * stride + k - pad < n)       # noqa: E731
        cy = torch.tensor([inside(H, o) for o in range(out_size(H, pad, stride))], dtype=torch.float32)
        cx = torch.tensor([inside(W, o) for o in range(out_size(W, pad, stride))], dtype=torch.float32)
        want = (cin * cy[:, None] * cx[None, :])[None, :, :, None].expand_as(y)
        assert torch.equal(y, want), f"{shape} H={H} W={W} pad={pad}: {(y != want).sum().item()} border counts differ"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dto%ds%d" % s)
def test_repeatable_and_batch_invariant(cuda, shape):
    cin, cout, stride = shape
    for geometry in ((31, 29, 3, 2), (61, 61, 3, 2), (6, 9, 3, 4)):
        x, w, scale, shift, _, _ = problem(shape, geometry)
        xd, wd, scd, shd = x.to(cuda), w.to(cuda), scale.to(cuda), shift.to(cuda)
        y1 = conv5f(xd, wd, stride, geometry[3], scd, shd, 1)
        y2 = conv5f(xd, wd, stride, geometry[3], scd, shd, 1)
        assert torch.equal(y1, y2), "two calls differ"
        for b in (0, 2):
            alone = conv5f(xd[b:b + 1].contiguous(), wd, stride, geometry[3], scd, shd, 1)
            assert torch.equal(alone[0], y1[b]), f"sample {b} of a batch of 3 differs from the same sample alone"


def test_relu_keeps_nan(cuda):
    """The epilogue's ReLU keeps a NaN, as ``torch.relu`` does: a NaN in one sample's corner pixel gives the NaN pattern of the
    unfused torch composition (conv2d, scale and shift, relu), and the other samples keep the bits of the clean run."""
    shape, geometry = SHAPES[0], GEOMETRIES[1]
    assert geometry == (5, 5, 3, 2)
    x, w, scale, shift, _, _ = problem(shape, geometry)
    bad = x.clone()
    bad[1, 0, 0, 1] = float("nan")
    wd, scd, shd = w.to(cuda), scale.to(cuda), shift.to(cuda)
    clean = conv5f(x.to(cuda), wd, shape[2], geometry[3], scd, shd, 1)
    y = conv5f(bad.to(cuda), wd, shape[2], geometry[3], scd, shd, 1)
    ref = torch.nn.functional.conv2d(bad.permute(0, 3, 1, 2), w, stride=shape[2], padding=geometry[3])
    ref = torch.relu(ref * scale[None, :, None, None] + shift[None, :, None, None]).permute(0, 2, 3, 1)
    want = torch.isnan(ref)
    assert want[1].any() and not want[1].all() and not want[0].any() and not want[2].any()
    assert torch.isfinite(clean).all()
    assert torch.equal(torch.isnan(y).cpu(), want)
    assert torch.equal(y[0], clean[0]) and torch.equal(y[2], clean[2])
    assert torch.equal(y[1][~want[1].to(cuda)], clean[1][~want[1].to(cuda)])
