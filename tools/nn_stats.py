#!/usr/bin/env python
"""Work counters of the pruned nearest-neighbour search (ops.nn_work, the library's own a3vt_dbg_nn_work): blocks and groups
of 16 candidates evaluated and point-to-box tests per wave of 64 queries, and the most groups any one wave evaluated.
python tools/nn_stats.py [--shapes 3x64x10000,...] [--gap 0.05] [--geometry bench]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from a3vt_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="3x64x10000,3x64x25000,3x8x50000")
ap.add_argument("--geometry", default="synthetic", choices=["synthetic", "bench"],
                help="synthetic: sphere 0.4 (+gap) against the ellipsoid (0.5, 0.3, 0.2); bench: what bench.py's untrained network "
                     "sees — a sphere of radius 0.25 against ellipsoids with semi-axes U(0.05, 0.16) (a3vt_amd.synthetic.gt_cloud)")
ap.add_argument("--gap", type=float, default=0.05)
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.manual_seed(0)


def surface(*shape, radii):
    u = torch.randn(*shape, 3, device=dev)
    return u / u.norm(dim=-1, keepdim=True) * torch.tensor(radii, device=dev)


for shape in args.shapes.split(","):
    draws, B, N = (int(v) for v in shape.split("x"))
    if args.geometry == "bench":
        from a3vt_amd.synthetic import gt_cloud
        x, y = surface(draws, B, N, radii=(0.25, 0.25, 0.25)), gt_cloud(B, N, 0).to(dev)
    x = x if args.geometry == "bench" else surface(draws, B, N, radii=(0.4, 0.4, 0.4)) + args.gap
    y = y if args.geometry == "bench" else surface(B, N, radii=(0.5, 0.3, 0.2))
    ops.nn_work(True)
    try:
        ops.chamfer_nn(x, y, algo="pruned")
    finally:
        c = ops.nn_work(False)
    w = max(c["waves"], 1)
    print(f"{shape:>14s} gap {args.gap}: {c['waves']} waves, {c['blocks'] / w:.1f} blocks ({c['groups'] / w:.1f} groups of 16) evaluated "
          f"and {c['box_tests'] / w:.1f} point-box tests per wave (of {(N + 63) // 64} blocks); worst wave: {c['max_groups_per_wave']} groups")
