#!/usr/bin/env python
"""Accuracy of training-mode ``BatchNorm2d + ReLU`` forward / backward in fp32 on the GPU, MIOpen's kernels against torch's own
(``torch.backends.cudnn.enabled = False``), both against the same computation in fp64.  Measured on an MI355X (ROCm 7, torch's
bundled MIOpen): at (2,16,61,61) — block 1 of the touch chart predictor at batch 2 — MIOpen's backward gives the input gradient to
6.3e-4 and the weight gradient to 3.2e-2 (relative to the largest entry) where torch's kernels give 1.3e-7 / 1.0e-7; at (2,32,31,31)
both are at 1e-7.  This is why ``reconstruction/touch/model.py::BatchNorm2d`` keeps training passes off MIOpen.
Run on the GPU box:  python tools/experiments/miopen_bn_bwd_accuracy.py"""
import torch

dev = torch.device("cuda", 0)
g = torch.Generator().manual_seed(0)


def rel(a, b):
    return ((a.double() - b).abs().max() / b.abs().max()).item()


for batch, c, n in ((2, 16, 61), (2, 32, 31), (64, 16, 61)):
    x = torch.randn(batch, c, n, n, generator=g, dtype=torch.float64) * 2 + 1
    gy = torch.randn(batch, c, n, n, generator=g, dtype=torch.float64)

    def run(dtype, miopen):
        torch.backends.cudnn.enabled = miopen
        bn = torch.nn.BatchNorm2d(c).to(dtype).to(dev).train()
        xx = x.to(dtype).to(dev).requires_grad_(True)
        y = torch.relu(bn(xx))
        y.backward(gy.to(dtype).to(dev))
        torch.backends.cudnn.enabled = True
        return y.detach().cpu(), xx.grad.cpu(), bn.weight.grad.cpu()

    ref = run(torch.float64, False)
    for name, out in (("MIOpen", run(torch.float32, True)), ("torch ", run(torch.float32, False))):
        print(f"({batch},{c},{n},{n}) {name}: y {rel(out[0], ref[0]):.2e}  dx {rel(out[1], ref[1]):.2e}  dgamma {rel(out[2], ref[2]):.2e}")
