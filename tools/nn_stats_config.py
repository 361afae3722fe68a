#!/usr/bin/env python
"""Work counters of the pruned search (ops.nn_work) inside a training step of BASELINE configs[3] / configs[4] (their own
geometry, not a synthetic sphere): python tools/nn_stats_config.py [--which 3]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from a3vt_amd import ops  # noqa: E402
from a3vt_amd.synthetic import NamedStep, named_config  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--which", type=int, default=3)
ap.add_argument("--batch", type=int, default=0)
args = ap.parse_args()
dev = torch.device("cuda", 0)
cfg = named_config(args.which, dev, "bf16s", args.batch or None)
step = NamedStep(cfg)
for k in range(6):
    ops.nn_work(True)
    try:
        step()
    finally:
        c = ops.nn_work(False)
    w = max(c["waves"], 1)
    print(f"step {k}: {c['waves']} waves, {c['blocks'] / w:.1f} blocks ({c['groups'] / w:.1f} groups of 16) evaluated, "
          f"{c['box_tests'] / w:.1f} point-box tests per wave; worst wave {c['max_groups_per_wave']} groups")
