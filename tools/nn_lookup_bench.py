#!/usr/bin/env python
"""One lookup of the nearest-neighbour latent policy at the reference's defaults — a bank of 15 400 latents (7 700 objects in
batches of 3, 40 % of them, 5 steps, 3 elements) of width 200, E = 3 elements, k = 25, the taken mask of step 4 (four of 50
actions performed per element) — ALTERNATING in one process between

* fused: ``LatentBank.lookup`` as ``Engine.choose`` ships it — the observation's latents and mask go to the device,
         ``ops.latent_nearest`` (``a3vt_latent_nearest``: two launches), one copy of E integers to the host; and
* loop:  ``reference_lookup``, the reference's per-element loop (``policies/NearestNeighbor/train.py:115-137``) on torch ops — a
         broadcast subtract / square / mean and a ``topk`` per element, then a Python walk that indexes the host list of actions
         with a device scalar: one device synchronisation per candidate.

Every call starts from host tensors (``obs["latent"]``, ``obs["mask"]``) and ends with host integers, so the host wall clock around
a call measures all of it, synchronisations included — they are the point.  Device events bracket the same call on the stream.
Medians with p10 / p90 over ``--calls`` calls per round and form, ``--rounds`` rounds, in turn, after ``--warmup`` calls of each.
Both forms must choose the same actions.  The result goes to stdout and, with ``--out``, to a file
(``profiles/nn_lookup_ab.txt``).  Run on the GPU box:  python tools/nn_lookup_bench.py --out profiles/nn_lookup_ab.txt"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ab_protocol as ab  # noqa: E402  (tools/ is this script's directory)

ap = argparse.ArgumentParser()
ab.add_arguments(ap, calls=100, rounds=5, warmup=20)
ap.add_argument("--bank_rows", type=int, default=15400)
ap.add_argument("--dim", type=int, default=200)
ap.add_argument("--env", type=int, default=3)
ap.add_argument("--num_actions", type=int, default=50)
ap.add_argument("--num_grasps", type=int, default=5)
ap.add_argument("--taken", type=int, default=4, help="actions already performed per element (the mask of step 4)")
a = ab.parse(ap)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from a3vt_amd.pterotactyl.policies.NearestNeighbor import train as nn  # noqa: E402

ab.require_gpu("nn_lookup_bench")
dev = torch.device("cuda", 0)
k = a.num_grasps * 5
g = np.random.default_rng(0)
bank = nn.LatentBank(a.num_actions)
bank.append(g.standard_normal((a.bank_rows, a.dim)).astype(np.float32), g.integers(0, a.num_actions, a.bank_rows))
latents = torch.from_numpy(g.standard_normal((a.env, a.dim)).astype(np.float32))        # obs["latent"]: a host tensor
mask = torch.zeros(a.env, a.num_actions)                                                  # obs["mask"]: a host tensor
# the policy performs what its nearest entries say, and an episode's latents move little: the mask holds the actions of each
# element's nearest entries, so the walk skips them as it does at step 4 of an episode
dev_bank, _ = bank.to(dev)
order = ((dev_bank.unsqueeze(0) - latents.to(dev).unsqueeze(1)) ** 2).mean(dim=2).argsort(dim=1)[:, :k].cpu()
for e in range(a.env):
    for j in order[e]:
        if mask[e].sum() == a.taken:
            break
        mask[e, bank.actions[int(j)]] = 1


def fused():
    return [int(v) for v in bank.lookup(latents, mask, k, device=dev)]


def loop():
    return [int(v) for v in nn.reference_lookup(dev_bank, bank.actions, latents, mask, k)]


forms = {"fused": fused, "loop": loop}
chosen = {name: fn() for name, fn in forms.items()}
same = chosen["fused"] == chosen["loop"]
# both clocks; fn() ends with host integers, everything it launched has finished: the host clock stops before the synchronise
res = ab.alternate(forms, a.calls, a.rounds, a.warmup)
result = {"bank_rows": a.bank_rows, "dim": a.dim, "env": a.env, "k": k, "num_actions": a.num_actions, "taken": a.taken,
          "calls": a.calls * a.rounds, "warmup": a.warmup, "same_actions": same, "actions": chosen["fused"],
          "device": torch.cuda.get_device_name(0)}
lines = [f"# one nearest-neighbour lookup, library call vs the reference's loop on torch ops; ms per call; {result['device']}",
         f"# bank {a.bank_rows} x {a.dim}, E = {a.env}, k = {k}, {a.taken} of {a.num_actions} actions taken per element; "
         f"{a.calls * a.rounds} calls per form in {a.rounds} alternating rounds after {a.warmup} warm-up calls"]
for name in forms:
    result[name] = res[name]
    for clock in ("host", "device"):
        s = result[name][clock]
        lines.append(f"# {name:5s} {clock:6s}: median {s['median']:8.4f}  p10 {s['p10']:8.4f}  p90 {s['p90']:8.4f}")
result["speedup_host_median"] = result["loop"]["host"]["median"] / result["fused"]["host"]["median"]
result["fused_p90_below_loop_p10"] = ab.wins(res, "fused", "loop", "host")
lines.append(json.dumps(result))
lines.append(f"# same actions: {same}; host wall loop / fused = {result['speedup_host_median']:.2f} (medians); fused p90 below loop p10: "
             f"{result['fused_p90_below_loop_p10']} -> FUSED_LOOKUP_DEFAULT = {result['fused_p90_below_loop_p10'] and same}")
ab.emit(lines, a.out)
if not same:
    raise SystemExit(f"nn_lookup_bench: the two forms chose different actions: {chosen}")
