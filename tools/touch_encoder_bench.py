#!/usr/bin/env python
"""The touch chart predictor's eval forward (``Encoder.forward`` under ``no_grad``) at B = 12 (one environment step: 3 environments
x 4 fingers) and B = 600 (a greedy ``best_step``: x 50 candidates), ALTERNATING in one process between

* fused: ``fused_stem=True``  — blocks 1-3 on ``a3vt_conv5f_nhwc`` (csrc/conv5f.hip), BatchNorm + ReLU in the epilogue; and
* torch: ``fused_stem=False`` — every layer on torch's modules (MIOpen convolutions, batch-norm and ReLU kernels).

After warm-up every call is bracketed by device events on the stream; p10 / median / p90 over ``--calls`` calls per round,
``--rounds`` rounds per path, in turn.  The stem alone (blocks 1-3) is timed the same way, and the fused stem's rate at B = 600
is given as a fraction of the 157.3 TFLOP/s fp32 matrix peak (2 flops per multiply-add of the nine convolutions).
The rule for ``model.FUSED_STEM_DEFAULT``: on only if the fused forward's p90 lies below the torch forward's p10 at both sizes.
Run on the GPU box:  python tools/touch_encoder_bench.py"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=40, help="timed calls per round and path")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--batches", type=int, nargs="+", default=[12, 600])
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from a3vt_amd import synthetic  # noqa: E402
from a3vt_amd.pterotactyl.reconstruction.touch import model  # noqa: E402
from a3vt_amd.pterotactyl.utility import utils  # noqa: E402

dev = torch.device("cuda", 0)
PEAK = 157.3e12


def stem_macs(net):
    """Multiply-adds per image of the nine convolutions of blocks 1-3 on a 121 x 121 image."""
    n, total = 121, 0
    for block in net.CNN_layers[:model.FUSED_BLOCKS]:
        for conv in (block.double_conv[0], block.double_conv[3], block.double_conv[6]):
            n = (n + 2 * conv.padding[0] - 5) // conv.stride[0] + 1
            total += n * n * conv.out_channels * conv.in_channels * 25
    return total


def timed(fn, calls):
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


torch.manual_seed(0)
nets = {"fused": model.Encoder(fused_stem=True).to(dev).eval(), "torch": model.Encoder(fused_stem=False).to(dev).eval()}
nets["torch"].load_state_dict(nets["fused"].state_dict())
template = utils.load_mesh_touch("touch_chart")[0]
macs = stem_macs(nets["fused"])
print(f"stem: {macs / 1e6:.1f} M multiply-adds per image (blocks 1-3, nine 5 x 5 convolutions)")
verdict = []
for B in a.batches:
    batch = synthetic.touch_batch(B, 8, seed=B)
    x = batch["sim_touch"].to(dev)
    ref = {k: v.to(dev) for k, v in batch["ref"].items()}
    verts = template.view(1, -1, 3).repeat(B, 1, 1)
    with torch.no_grad():
        diff = (nets["fused"](x, ref, verts) - nets["torch"](x, ref, verts)).abs().max().item()
        print(f"B = {B}: max |fused - torch| of the forward = {diff:.3e}")
        for what in ("forward", "stem"):
            fns = {k: ((lambda n=n: n(x, ref, verts)) if what == "forward" else (lambda n=n: n.stem(x))) for k, n in nets.items()}
            for k in fns:
                for _ in range(a.warmup):
                    fns[k]()
            torch.cuda.synchronize()
            ms = {k: [] for k in fns}
            for _ in range(a.rounds):
                for k in fns:
                    ms[k] += timed(fns[k], a.calls)
            pct = {k: np.percentile(v, [10, 50, 90]) for k, v in ms.items()}
            for k in fns:
                line = f"B = {B:4d} {what:8s} {k:6s}: p10 {pct[k][0]:8.3f} ms  median {pct[k][1]:8.3f}  p90 {pct[k][2]:8.3f}   ({len(ms[k])} calls)"
                if what == "stem":
                    rate = 2.0 * macs * B / (pct[k][1] * 1e-3)
                    line += f"   {rate / 1e12:6.2f} TFLOP/s = {rate / PEAK:.3f} of the fp32 matrix peak"
                print(line)
            below = pct["fused"][2] < pct["torch"][0]
            print(f"B = {B:4d} {what:8s} fused / torch = {pct['fused'][1] / pct['torch'][1]:.3f} (medians); fused p90 {'<' if below else '>='} torch p10")
            if what == "forward":
                verdict.append(below)
print(f"rule for the default: fused p90 < torch p10 at every size: {all(verdict)} -> FUSED_STEM_DEFAULT = {all(verdict)}")
