"""oracle.image — float64 references of the image pyramid's bf16 kernels (TEST INFRASTRUCTURE ONLY).

``conv5.hip`` (the 5 x 5 convolutions of layers 0-6: forward, input gradients, weight gradients) and ``bnrelu.hip`` (training
BatchNorm2d + ReLU and its backward), written out in float64 on the bf16 VALUES the kernels read, plus the one helper their
tests need to compare a bf16 result with an fp64 value: the interval of bf16 values a correctly rounded fp32 result can round to.

Convolution references return ``(value, abs_sum)``: ``abs_sum`` is the sum of the magnitudes of the terms of each output (for
margins of the form ``k * 2^-24 * abs_sum``).  Tensors are NCHW float64 on the CPU; weights OIHW.
"""
import torch
import torch.nn.functional as F


def bf16_rne(v):
    """float64 -> the nearest bf16 value (ties to even), ONE rounding, as float64.

    Not ``v.to(torch.bfloat16)``: torch converts float64 to bf16 through float32, i.e. it rounds twice
    (1 + 2^-8 + 2^-30 -> 1 + 2^-8 -> 1.0 instead of 1 + 2^-7).  Normal numbers keep 8 significant bits; below 2^-126 the bf16
    spacing is 2^-133 (subnormals).  Overflow past the bf16 range is not modelled (the tests stay far below it)."""
    v = v.double()
    _, e = torch.frexp(v)                                  # |v| = m 2^e, m in [0.5, 1): spacing of 8 significant bits 2^(e - 8)
    q = torch.ldexp(torch.ones_like(v), torch.clamp(e - 8, min=-133))
    return torch.round(v / q) * q                          # (scaling by a power of two is exact; torch.round: half to even)


def bf16_interval(v, margin=0.0):
    """The bf16 values an fp32 result within ``margin`` of the exact value ``v`` can round to (nearest even): the closed
    interval ``[lo, hi]`` (float64).  Rounding is monotone, so the ends are the roundings of ``v - margin`` and ``v + margin``."""
    v = v.double()
    m = torch.as_tensor(margin, dtype=torch.float64)
    return bf16_rne(v - m), bf16_rne(v + m)


def in_interval(dev, lo, hi):
    """Elementwise ``lo <= dev <= hi`` for a device bf16 tensor (any device) against float64 ends."""
    d = dev.detach().double().cpu()
    return (d >= lo) & (d <= hi)


# ---- conv5.hip ------------------------------------------------------------------------------------------------------------------
def _conv(x, w, stride, padding):
    return F.conv2d(x.double(), w.double(), None, stride=stride, padding=padding)


def conv5_forward(x, w, bias=None, stride=1):
    """``conv5_kernel`` / ``conv5c3_kernel``: 5 x 5, padding 1, on the bf16 values of x and the bf16 weight image ``w``;
    ``bias`` (fp32) is added before the one rounding to bf16."""
    y, a = _conv(x, w, stride, 1), _conv(x.abs(), w.abs(), stride, 1)
    if bias is not None:
        b = bias.double().view(1, -1, 1, 1)
        y, a = y + b, a + b.abs()
    return y, a


def flip_weight(w):
    """The input-gradient form of a (cout, cin, 5, 5) weight: (cin, cout, 5, 5) with both taps reversed (``flip != 0`` of
    ``conv5_weight_image_kernel``)."""
    return w.double().transpose(0, 1).flip(2, 3)


def conv5_input_grad(gy, w):
    """The input gradient of a stride-1 layer as the kernel forms it: the forward kernel on gy with the flipped weights,
    padding 3 (equals ``torch.nn.grad.conv2d_input(..., padding=1)``: tests/test_oracle_image_emulation.py)."""
    wf = flip_weight(w)
    return _conv(gy, wf, 1, 3), _conv(gy.abs(), wf.abs(), 1, 3)


def zero_upsample(gy):
    """(B, C, ho, wo) -> (B, C, 2 ho, 2 wo) with gy at the even positions and zeros elsewhere (UP3's view of its input)."""
    B, C, ho, wo = gy.shape
    u = torch.zeros(B, C, 2 * ho, 2 * wo, dtype=torch.float64)
    u[:, :, ::2, ::2] = gy.double()
    return u


def conv5_input_grad_up3(gy, w):
    """The input gradient of layer 1 (3 <- 16, stride 2; ``a3vt_conv5_input_grad_3x16s2``) on an input map of 2 ho + 2 by
    2 wo + 2 pixels: the stride-1 form on the zero-upsampled gy, flipped weights, padding 3."""
    u, wf = zero_upsample(gy), flip_weight(w)
    return _conv(u, wf, 1, 3), _conv(u.abs(), wf.abs(), 1, 3)


def conv5_weight_grad(x, gy, stride=1):
    """gw[co][ci][ky][kx] = sum over (b, oy, ox) of gy[b][co][oy][ox] * x[b][ci][oy s + ky - 1][ox s + kx - 1] (padding 1)."""
    shape = (gy.shape[1], x.shape[1], 5, 5)
    gw = torch.nn.grad.conv2d_weight(x.double(), shape, gy.double(), stride=stride, padding=1)
    a = torch.nn.grad.conv2d_weight(x.double().abs(), shape, gy.double().abs(), stride=stride, padding=1)
    return gw, a


# ---- bnrelu.hip -----------------------------------------------------------------------------------------------------------------
def bn_relu_forward(x, gamma, beta, eps, momentum, running_mean, running_var, pre_bias=None):
    """Training BatchNorm2d + ReLU over (N, H, W) per channel of a bf16-valued (N, C, H, W) map, in float64.

    Returns a dict: ``mean``, ``var`` (biased), ``invstd``, ``y_pre`` (before the ReLU), ``y``, and the running statistics as
    ``nn.BatchNorm2d`` leaves them: ``running_mean`` takes the mean of ``x + pre_bias`` (a Conv2d bias the producer did not
    add), ``running_var`` the unbiased variance."""
    xd = x.double()
    n = xd.numel() // xd.shape[1]
    mean = xd.mean(dim=(0, 2, 3))
    var = ((xd - mean.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))
    invstd = 1.0 / torch.sqrt(var + eps)
    g, b = gamma.double(), beta.double()
    y_pre = (xd - mean.view(1, -1, 1, 1)) * (g * invstd).view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
    mean_in = mean + (pre_bias.double() if pre_bias is not None else 0.0)
    rm = running_mean.double() + momentum * (mean_in - running_mean.double())
    rv = running_var.double() + momentum * (var * n / (n - 1) - running_var.double())
    return {"mean": mean, "var": var, "invstd": invstd, "y_pre": y_pre, "y": torch.relu(y_pre),
            "running_mean": rm, "running_var": rv}


def bn_relu_backward(x, dy, mask, gamma, mean, invstd):
    """Backward of ``relu(batch_norm(x))`` (training) in float64 with an EXPLICIT ReLU mask (the device's own ``y > 0`` in the
    GPU tests: teacher forcing) and the statistics ``mean`` / ``invstd`` the forward used.

    g = dy where mask, else 0;  dbeta = sum g;  dgamma = sum g xhat;  dx = gamma invstd (g - dbeta / n - xhat dgamma / n).
    Returns ``(dx, dgamma, dbeta, abs_dgamma, abs_dbeta)`` — the last two: sums of |g xhat| and |g| (for margins)."""
    xd = x.double()
    n = xd.numel() // xd.shape[1]
    view = lambda t: t.double().view(1, -1, 1, 1)  # noqa: E731
    g = torch.where(mask.bool(), dy.double(), torch.zeros((), dtype=torch.float64))
    xhat = (xd - view(mean)) * view(invstd)
    dbeta, dgamma = g.sum(dim=(0, 2, 3)), (g * xhat).sum(dim=(0, 2, 3))
    dx = view(gamma) * view(invstd) * (g - view(dbeta) / n - xhat * view(dgamma) / n)
    return dx, dgamma, dbeta, (g * xhat).abs().sum(dim=(0, 2, 3)), g.abs().sum(dim=(0, 2, 3))
