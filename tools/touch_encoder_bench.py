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

import ab_protocol as ab  # noqa: E402  (tools/ is this script's directory)

ap = argparse.ArgumentParser()
ab.add_arguments(ap, calls=40, rounds=3, warmup=10, out=False, what="path")
ap.add_argument("--batches", type=int, nargs="+", default=[12, 600])
a = ap.parse_args()

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
            # device events alone, no synchronise between the calls
            res = ab.alternate(fns, a.calls, a.rounds, a.warmup, clocks=("device",))
            for k in fns:
                s = res[k]["device"]
                line = f"B = {B:4d} {what:8s} {k:6s}: p10 {s['p10']:8.3f} ms  median {s['median']:8.3f}  p90 {s['p90']:8.3f}   ({a.calls * a.rounds} calls)"
                if what == "stem":
                    rate = 2.0 * macs * B / (s["median"] * 1e-3)
                    line += f"   {rate / 1e12:6.2f} TFLOP/s = {rate / PEAK:.3f} of the fp32 matrix peak"
                print(line)
            below = ab.wins(res, "fused", "torch", "device")
            print(f"B = {B:4d} {what:8s} fused / torch = {res['fused']['device']['median'] / res['torch']['device']['median']:.3f} (medians); "
                  f"fused p90 {'<' if below else '>='} torch p10")
            if what == "forward":
                verdict.append(below)
print(f"rule for the default: fused p90 < torch p10 at every size: {all(verdict)} -> FUSED_STEM_DEFAULT = {all(verdict)}")
