"""CPU: anchors for ``oracle.image``, the float64 references tests/test_gpu_image_exact.py holds the image pyramid's bf16
kernels (csrc/conv5.hip, csrc/bnrelu.hip) to.

1. The bf16 rounding helper rounds ONCE, to nearest even: exact ties, ties +- a tiny amount, the double-rounding
   counterexample torch's own float64 -> bf16 conversion gets wrong, and fp32 inputs against torch's (single) fp32 -> bf16 rounding.
2. The explicit BatchNorm + ReLU backward equals float64 autograd of ``relu(batch_norm(x))`` to 1e-12.
3. The kernels' formulation of the input gradients — flipped weights with padding 3, and layer 1's through the zero-upsampled
   map — equals ``torch.nn.grad.conv2d_input`` exactly on integer data; the other references equal torch's own products.
"""
import pytest
import torch

from oracle import image as oi


def _bf(xs):
    return torch.tensor(xs, dtype=torch.float64)


def test_bf16_rne_ties_go_to_even():
    u = 2.0 ** -8                       # half a bf16 ulp at 1
    v = _bf([1 + u, 1 + 3 * u, 1 + 5 * u, -(1 + u), -(1 + 3 * u), 2 + 2 * u, 256 + 1, 256 + 3, 0.0, -0.0])
    want = _bf([1.0, 1 + 4 * u, 1 + 4 * u, -1.0, -(1 + 4 * u), 2.0, 256.0, 256 + 4, 0.0, 0.0])
    assert torch.equal(oi.bf16_rne(v), want)


def test_bf16_rne_near_ties_go_the_right_way():
    u, t = 2.0 ** -8, 2.0 ** -40
    v = _bf([1 + u + t, 1 + u - t, 1 + 3 * u - t, 1 + 3 * u + t, -(1 + u + t), -(1 + u - t)])
    want = _bf([1 + 2 * u, 1.0, 1 + 2 * u, 1 + 4 * u, -(1 + 2 * u), -1.0])
    assert torch.equal(oi.bf16_rne(v), want)


def test_bf16_rne_rounds_once_where_torch_rounds_twice():
    v = _bf([1 + 2.0 ** -8 + 2.0 ** -30])
    assert float(oi.bf16_rne(v)) == 1 + 2.0 ** -7
    assert float(v.to(torch.bfloat16).double()) == 1.0          # (fp64 -> fp32 -> bf16: the first rounding makes a tie)
    lo, hi = oi.bf16_interval(v)
    assert float(lo) == float(hi) == 1 + 2.0 ** -7
    lo, hi = oi.bf16_interval(_bf([1 + 2.0 ** -8]), 2.0 ** -20)  # a margin across the tie: both neighbours
    assert float(lo) == 1.0 and float(hi) == 1 + 2.0 ** -7


def test_bf16_rne_matches_torch_on_fp32_inputs():
    """An fp32 value is exact in float64, so one rounding from either is the same: against torch's fp32 -> bf16 (nearest even)
    over many binades, subnormals and exact ties included."""
    g = torch.Generator().manual_seed(0)
    f = torch.randn(200000, generator=g) * torch.exp2(torch.randint(-140, 120, (200000,), generator=g).float())
    ties = (torch.randint(-2 ** 15, 2 ** 15, (20000,), generator=g).float() * 2 + 1) * 2.0 ** -20   # 17 significant bits: ties
    f = torch.cat([f, ties, torch.tensor([2.0 ** -130, 3 * 2.0 ** -134, 2.0 ** -126 * (1 + 2.0 ** -8)])])
    assert torch.equal(oi.bf16_rne(f.double()), f.to(torch.bfloat16).double())


def test_bn_backward_equals_float64_autograd():
    g = torch.Generator().manual_seed(1)
    for shape in ((4, 5, 7, 3), (2, 16, 9, 9), (3, 3, 1, 2)):
        C = shape[1]
        x = (torch.randn(shape, generator=g, dtype=torch.float64) * 1.3 + torch.randn(1, C, 1, 1, generator=g, dtype=torch.float64))
        gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
        beta = torch.randn(C, generator=g, dtype=torch.float64) * 0.3
        dy = torch.randn(shape, generator=g, dtype=torch.float64)
        eps = 1e-5
        xa, ga, ba = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
        y = torch.relu(torch.nn.functional.batch_norm(xa, rm, rv, ga, ba, True, 0.1, eps))
        y.backward(dy)
        f = oi.bn_relu_forward(x, gamma, beta, eps, 0.1, torch.zeros(C), torch.ones(C))
        assert torch.allclose(f["y"], y.detach(), rtol=0, atol=1e-12)
        torch.testing.assert_close(f["running_mean"], rm, rtol=0, atol=1e-12)
        torch.testing.assert_close(f["running_var"], rv, rtol=0, atol=1e-12)
        dx, dgam, dbet, _, _ = oi.bn_relu_backward(x, dy, f["y"] > 0, gamma, f["mean"], f["invstd"])
        for a, b in ((dx, xa.grad), (dgam, ga.grad), (dbet, ba.grad)):
            assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), float((a - b).abs().max())


def test_bn_forward_pre_bias_moves_the_running_mean_only():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, 4, 5, 6, generator=g, dtype=torch.float64)
    gamma, beta, pb = torch.ones(4), torch.zeros(4), torch.randn(4, generator=g)
    a = oi.bn_relu_forward(x, gamma, beta, 1e-5, 0.25, torch.zeros(4), torch.ones(4))
    b = oi.bn_relu_forward(x, gamma, beta, 1e-5, 0.25, torch.zeros(4), torch.ones(4), pre_bias=pb)
    assert torch.equal(a["y"], b["y"]) and torch.equal(a["running_var"], b["running_var"])
    torch.testing.assert_close(b["running_mean"], 0.25 * (x + pb.double().view(1, -1, 1, 1)).mean(dim=(0, 2, 3)), rtol=0, atol=1e-15)


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).double()


@pytest.mark.parametrize("cin,cout,hw", [(16, 16, (9, 7)), (32, 32, (5, 6)), (3, 3, (4, 3)), (16, 16, (3, 3)), (16, 16, (3, 5))])
def test_flipped_weight_input_gradient_is_conv2d_input(cin, cout, hw):
    x_shape = (2, cin) + hw
    w = _ints((cout, cin, 5, 5), -3, 3, 1)
    gy = _ints((2, cout, hw[0] - 2, hw[1] - 2), -2, 2, 2)        # (stride 1, padding 1, 5 x 5: the output is 2 pixels smaller)
    ref = torch.nn.grad.conv2d_input(x_shape, w, gy, padding=1)
    got, a = oi.conv5_input_grad(gy, w)
    assert torch.equal(got, ref)
    assert bool((a >= got.abs()).all())


@pytest.mark.parametrize("ho,wo", [(1, 1), (3, 5), (6, 4), (11, 8)])
def test_zero_upsampled_layer1_input_gradient_is_conv2d_input(ho, wo):
    """Layer 1 (3 -> 16, stride 2, padding 1) on a 2 ho + 2 by 2 wo + 2 map: the gradient of its input is the stride-1 form on
    the zero-upsampled gy, flipped weights, padding 3 — what ``a3vt_conv5_input_grad_3x16s2`` computes."""
    w = _ints((16, 3, 5, 5), -3, 3, 3)
    gy = _ints((2, 16, ho, wo), -2, 2, 4)
    ref = torch.nn.grad.conv2d_input((2, 3, 2 * ho + 2, 2 * wo + 2), w, gy, stride=2, padding=1)
    got, _ = oi.conv5_input_grad_up3(gy, w)
    assert got.shape == ref.shape and torch.equal(got, ref)


def test_forward_and_weight_gradient_references():
    x = _ints((2, 16, 9, 8), -4, 4, 5)
    w = _ints((32, 16, 5, 5), -3, 3, 6)
    b = torch.arange(32, dtype=torch.float32) * 0.25 - 3.5
    y, a = oi.conv5_forward(x, w, b, stride=2)
    assert torch.equal(y, torch.nn.functional.conv2d(x, w, b.double(), stride=2, padding=1))
    assert bool((a >= y.abs()).all())
    gy = _ints(y.shape, -2, 2, 7)
    gw, ga = oi.conv5_weight_grad(x, gy, stride=2)
    xx, ww = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    torch.nn.functional.conv2d(xx, ww, None, stride=2, padding=1).backward(gy)
    assert torch.equal(gw, ww.grad) and bool((ga >= gw.abs()).all())
