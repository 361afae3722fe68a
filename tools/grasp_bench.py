#!/usr/bin/env python
"""Time ``KinematicGrasp.grasp_table`` (placement on the host, then ``a3vt_grasp_close``, csrc/grasp_close.hip) on one GPU, by
``ab_protocol.py``'s clocks: host wall and device events, median (p10, p90).

**The closing rule is a kinematic stand-in for pybullet's five ``stepSimulation`` calls.  Nothing here is compared with pybullet.**
The parent commit cannot grasp, so there is no old form, no ratio and no default to decide: the numbers are recorded.

Sizes: 1 and 8 objects of an icosphere-5 (20 480 faces; the copies scaled per axis) x 50 actions at ``--steps`` 64.  Reported per
size: one ``grasp_table`` call (host wall, which holds the placement; the placement's own host time), ``ops.grasp_close`` alone on
inputs already on the device (device events and host wall), the candidate triangles per workgroup (``ops.grasp_candidates``) against the LDS capacity, and the launches
from the library's counters.  For scale only, NOT a target: one call of the vectorised float64 NumPy path on the first size.

    python tools/grasp_bench.py --hand tests/golden/allegro_hand.npz --out profiles/grasp_close.txt"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ab_protocol as ab  # noqa: E402  (tools/ is this script's directory)
from a3vt_amd import mesh, ops  # noqa: E402
from a3vt_amd.pterotactyl.simulator.hand import HandModel  # noqa: E402
from a3vt_amd.pterotactyl.simulator.physics.grasping import KinematicGrasp, hull_facets, place_hand  # noqa: E402

p = argparse.ArgumentParser()
ab.add_arguments(p, calls=4, rounds=5, warmup=2)
p.add_argument("--hand", default=None, help="a hand URDF or .npz (default: PTEROTACTYL_HAND)")
p.add_argument("--level", type=int, default=5)
p.add_argument("--radius", type=float, default=0.08)
p.add_argument("--steps", type=int, default=64)
p.add_argument("--actions", type=int, default=50)
p.add_argument("--sizes", type=int, nargs="+", default=[1, 8])
p.add_argument("--numpy", type=int, default=1, help="calls of the NumPy path on the first size (0: none)")
a = ab.parse(p)
ab.require_gpu("grasp_bench")
dev = torch.device("cuda", 0)
hand = HandModel.load(a.hand)

v, f = mesh.icosphere(a.level)
v = np.asarray(v, np.float64)
v = v / np.linalg.norm(v, axis=1, keepdims=True) * a.radius
rng = np.random.default_rng(0)
lines = [f"# profiles/grasp_close.txt: `python tools/grasp_bench.py --hand tests/golden/allegro_hand.npz --out profiles/grasp_close.txt`, "
         f"one {torch.cuda.get_device_name(0)}",
         f"# KinematicGrasp.grasp_table: icosphere-{a.level} ({len(f)} faces, radius {a.radius} m, scaled per axis by 0.8..1.2) x {a.actions} "
         f"actions, steps {a.steps}; {a.warmup} warm-up, {a.rounds} rounds of {a.calls} calls; ms, median (p10, p90)",
         "# THE CLOSING RULE IS A KINEMATIC STAND-IN FOR PYBULLET'S stepSimulation: no frame has been compared with pybullet's",
         "# recorded numbers, not a gate: the parent commit cannot grasp"]
result = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "actions": a.actions, "faces": int(len(f)), "sizes": {}}
fmt = lambda s: f"{s['median']:9.3f} ({s['p10']:9.3f}, {s['p90']:9.3f})"  # noqa: E731
for n in a.sizes:
    geometry = {f"object{e}": ((v * (0.8 + 0.4 * rng.random(3))).astype(np.float32), f) for e in range(n)}
    ids = list(geometry)
    grasper = KinematicGrasp(hand, steps=a.steps, device=dev)
    placement = []

    def call():
        table = grasper.grasp_table(geometry, ids, a.actions, want_blocked_step=True)
        placement.append(grasper.placement_seconds * 1e3)
        return table
    ops.grasp_launches(reset=True)
    table = call()
    launches = ops.grasp_launches()
    placement.clear()
    res = ab.alternate({"grasp_table": call}, a.calls, a.rounds, a.warmup, clocks=("host",))["grasp_table"]
    # the closing alone, on inputs made ahead: the placements the table itself made, already on the device
    placed = [(e, act) for e in range(n) for act in range(a.actions) if table["present"][e, act].any()]
    verts, faces, offsets, base, poses = [], [], [0], 0, []
    for e, obj in enumerate(ids):
        ov, of = geometry[obj]
        facets = hull_facets(ov)
        poses += [place_hand(ov, act, a.actions, facets=facets) for (ee, act) in placed if ee == e]
        verts.append(ov)
        faces.append(np.asarray(of, np.int64) + base)
        base += len(ov)
        offsets.append(offsets[-1] + len(of))
    verts, faces, which = np.concatenate(verts), np.concatenate(faces), [e for e, _ in placed]
    base_pos, base_rot = np.array([q[0] for q in poses], np.float32), np.array([q[1] for q in poses], np.float32)
    on_dev = [torch.from_numpy(x).to(dev) for x in (verts, faces.astype(np.int32), base_pos, base_rot)]
    table_np = hand.table()
    close = lambda: ops.grasp_close(on_dev[0], on_dev[1], offsets, which, on_dev[2], on_dev[3], table_np, hand.q0, a.steps)  # noqa: E731
    kernel = ab.alternate({"grasp_close": close}, a.calls, a.rounds, a.warmup, host_stops="after")["grasp_close"]
    counts = ops.grasp_candidates(verts, faces, offsets, which, base_pos, base_rot, table_np)
    capacity = ops.grasp_limits()["capacity"]
    blocked = table["blocked_step"][table["present"].any(axis=2)]
    lines += [f"# {n} object(s): {len(placed)} grasps placed of {n * a.actions}; {launches['launches']} launch(es) in {launches['calls']} call",
              f"#   grasp_table, host wall        {fmt(res['host'])}   (placement, upload, the launches, the read of the frames)",
              f"#   of it placement               {fmt(ab.stats(placement))}   (host: one convex hull per object, one ray cast and pose per action)",
              f"#   ops.grasp_close alone, device events {fmt(kernel['device'])}   host wall {fmt(kernel['host'])}   (inputs on the device)",
              f"#   candidates per workgroup: min {counts.min()} median {int(np.median(counts))} max {counts.max()}; LDS capacity {capacity}: "
              f"{int((counts > capacity).sum())} of {counts.size} workgroups read the rest from global memory in every query",
              f"#   joints stopped before the last step: {int((blocked < a.steps).sum())} of {blocked.size}"]
    result["sizes"][n] = {"placed": len(placed), "launches": launches, "ms": res, "grasp_close_ms": kernel, "placement_ms": ab.stats(placement),
                          "candidates": {"min": int(counts.min()), "median": float(np.median(counts)), "max": int(counts.max())}}
    if a.numpy and n == a.sizes[0]:
        host = KinematicGrasp(hand, steps=a.steps, device="cpu")
        took = []
        for _ in range(a.numpy):
            t0 = time.perf_counter()
            host_table = host.grasp_table(geometry, ids, a.actions, want_blocked_step=True)
            took.append((time.perf_counter() - t0) * 1e3)
        same = float((host_table["blocked_step"] == table["blocked_step"]).mean())
        lines.append(f"#   for scale only, NOT a target: the vectorised float64 NumPy path, {a.numpy} call(s): {np.median(took):.0f} ms; "
                     f"blocked_step equal to the kernel's on {same:.4f} of the joints (undecided queries may differ)")
        result["sizes"][n]["numpy_ms"] = took
lines.append("# not measured: pybullet's frames, a data-set-scale run, real objects, other steps")
lines.append(json.dumps(result))
ab.emit(lines, a.out)
