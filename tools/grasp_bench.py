#!/usr/bin/env python
"""Time ``KinematicGrasp.grasp_table`` (placement on the host, then ``a3vt_grasp_close``, csrc/grasp_close.hip) on one GPU, by
``ab_protocol.py``'s clocks: host wall and device events, median (p10, p90).

**The closing rule is a kinematic stand-in for pybullet's five ``stepSimulation`` calls.  Nothing here is compared with pybullet.**
The parent commit cannot grasp, so there is no old form, no ratio and no default to decide: the numbers are recorded.

Sizes: 1 and 8 objects of an icosphere-5 (20 480 faces; the copies scaled per axis) x 50 actions at ``--steps`` 64.  Reported per
size: one ``grasp_table`` call (host wall, which holds the placement; the placement's own host time), ``ops.grasp_close`` alone on
inputs already on the device (device events and host wall), the candidate triangles per workgroup (``ops.grasp_candidates``) against the LDS capacity, and the launches
from the library's counters.  For scale only, NOT a target: one call of the vectorised float64 NumPy path on the first size.

    python tools/grasp_bench.py --hand tests/golden/allegro_hand.npz --out profiles/grasp_close.txt

``--placement both``: the A/B of the placement instead — ``grasp_table`` with ``placement="host"`` (``place_hand`` on SciPy's hull)
against ``placement="device"`` (``ops.hull_place``, csrc/hull_place.hip), ALTERNATING in this process at the same sizes: host wall,
the placement's share, ``ops.hull_place`` alone by device events, the pairs left undecided, and whether the two tables agree.  The
rule for ``DEVICE_PLACEMENT_DEFAULT``: device p90 below host p10 at every size.

    python tools/grasp_bench.py --hand tests/golden/allegro_hand.npz --placement both --out profiles/grasp_place_ab.txt"""
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
p.add_argument("--placement", choices=("host", "both"), default="host", help="both: the host / device placement A/B (see above)")
a = ab.parse(p)
ab.require_gpu("grasp_bench")
dev = torch.device("cuda", 0)
hand = HandModel.load(a.hand)

v, f = mesh.icosphere(a.level)
v = np.asarray(v, np.float64)
v = v / np.linalg.norm(v, axis=1, keepdims=True) * a.radius
rng = np.random.default_rng(0)


def placement_ab():
    """The host / device placement A/B -> the lines of profiles/grasp_place_ab.txt."""
    from a3vt_amd.pterotactyl.simulator.physics import grasping
    out = [f"# profiles/grasp_place_ab.txt: `python tools/grasp_bench.py --hand tests/golden/allegro_hand.npz --placement both --out "
           f"profiles/grasp_place_ab.txt`, one {torch.cuda.get_device_name(0)}",
           f"# KinematicGrasp.grasp_table, placement=\"host\" (place_hand on SciPy's hull) against placement=\"device\" (ops.hull_place): "
           f"icosphere-{a.level} ({len(v)} vertices, {len(f)} faces, radius {a.radius} m, scaled per axis by 0.8..1.2) x {a.actions} actions, "
           f"steps {a.steps}; the two forms alternating in one process, {a.warmup} warm-up, {a.rounds} rounds of {a.calls} calls; ms, median "
           f"(p10, p90)",
           "# the host placement is measured again here, beside the device form: profiles/grasp_close.txt's figure is not the yardstick"]
    result = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "actions": a.actions, "vertices": int(len(v)), "sizes": {}}
    verdicts = []
    for n in a.sizes:
        geometry = {f"object{e}": ((v * (0.8 + 0.4 * rng.random(3))).astype(np.float32), f) for e in range(n)}
        ids = list(geometry)
        graspers = {name: KinematicGrasp(hand, steps=a.steps, device=dev, placement=name) for name in ("device", "host")}
        share, tables = {"device": [], "host": []}, {}

        def form(name):
            def call():
                tables[name] = graspers[name].grasp_table(geometry, ids, a.actions, want_base=True, want_blocked_step=True)
                share[name].append(graspers[name].placement_seconds * 1e3)
            return call
        ops.hull_place_launches(reset=True)
        form("device")()
        launches = ops.hull_place_launches()
        for name in share:
            share[name].clear()
        res = ab.alternate({name: form(name) for name in ("device", "host")}, a.calls, a.rounds, a.warmup, clocks=("host",))
        for name in share:                                  # (the warm-up calls' shares are not timed calls)
            del share[name][:a.warmup]
        on_dev = torch.from_numpy(np.concatenate([geometry[obj][0] for obj in ids])).to(dev)
        offsets = np.cumsum([0] + [len(geometry[obj][0]) for obj in ids])
        dirs = grasping.directions(a.actions)
        kernel = ab.alternate({"hull_place": lambda: ops.hull_place(on_dev, offsets, dirs)}, a.calls, a.rounds, a.warmup,
                              host_stops="after")["hull_place"]
        status = ops.hull_place(on_dev, offsets, dirs)["status"].cpu().numpy()
        h, d = tables["host"], tables["device"]
        same = (h["base_pos"] == d["base_pos"]).all(axis=-1) & (h["base_rot"] == d["base_rot"]).all(axis=(-1, -2))
        # pairs whose poses differ by more than one float32 ulp: is it the same hit on another facet (a ray through an edge or a
        # vertex of the hull lies in two or more facets, and hull_hit takes whichever comes first)?
        ulps = lambda k: np.abs(h[k].astype(np.float64) - d[k].astype(np.float64)) / np.spacing(np.abs(h[k])).astype(np.float64)  # noqa: E731
        apart = (ulps("base_pos").max(axis=-1) > 1) | (ulps("base_rot").max(axis=(-1, -2)) > 1)
        t_dev = ops.hull_place(on_dev, offsets, dirs)["t"].cpu().numpy()
        same_hit = 0
        for e in sorted(set(np.argwhere(apart)[:, 0].tolist())):
            ov = geometry[ids[e]][0]
            facets = grasping.hull_facets(ov)
            for act in np.flatnonzero(apart[e]).tolist():
                found = grasping.hull_hit(ov, dirs[act], facets)
                same_hit += found is not None and bool(np.abs(found[0] - dirs[act] * t_dev[e, act]).max() <= 1e-12 * np.abs(found[0]).max())
        out += [f"# {n} object(s): {n * a.actions} pairs, {launches['launches']} hull_place launch(es) in {launches['calls']} call; status 0 / 1 / 2: "
                f"{int((status == 0).sum())} / {int((status == 1).sum())} / {int((status == 2).sum())} (status 2 pairs go to place_hand)"]
        won = ab.report(f"{n} object(s): grasp_table, host wall (placement, upload, the launches, the read of the frames)", res, "device", "host",
                        out, clock="host")
        verdicts.append(won)
        out += [f"#   of it placement, host form    {fmt(ab.stats(share['host']))}   (one convex hull per object, one ray cast and pose per action)",
                f"#   of it placement, device form  {fmt(ab.stats(share['device']))}   (upload of the vertices, ops.hull_place, the read of status)",
                f"#   ops.hull_place alone, device events {fmt(kernel['device'])}   host wall {fmt(kernel['host'])}   (vertices on the device)",
                f"#   the two tables: present equal: {bool(np.array_equal(h['present'], d['present']))}; base poses bit-equal on "
                f"{int(same.sum())} of {same.size} pairs, more than one float32 ulp apart on {int(apart.sum())}, of which {same_hit} have the "
                f"same hit point to 1e-12 (a ray through an edge or vertex of the hull: the facet is either's choice); blocked_step equal "
                f"on {float((h['blocked_step'] == d['blocked_step']).mean()):.4f} of the joints"]
        result["sizes"][n] = {"ms": res, "placement_ms": {k: ab.stats(x) for k, x in share.items()}, "hull_place_ms": kernel,
                              "status": [int((status == k).sum()) for k in range(3)], "wins": bool(won),
                              "bit_equal_pairs": int(same.sum()), "pairs_apart": int(apart.sum()), "apart_with_the_same_hit": int(same_hit)}
    met = all(verdicts)
    out += [f"# the rule for DEVICE_PLACEMENT_DEFAULT (device p90 below host p10 on host wall at every size): {'MET' if met else 'NOT MET'}; the "
            "constant stays False in this change either way: with it on, base poses may move by a float32 ulp and existing tests pin them",
            "# not measured: a data-set-scale bake, real objects, other vertex counts, more than 8 objects per call, vertices staged in LDS"]
    result["rule_met"] = bool(met)
    out.append(json.dumps(result))
    return out


fmt = lambda s: f"{s['median']:9.3f} ({s['p10']:9.3f}, {s['p90']:9.3f})"  # noqa: E731
if a.placement == "both":
    ab.emit(placement_ab(), a.out)
    raise SystemExit(0)
lines = [f"# profiles/grasp_close.txt: `python tools/grasp_bench.py --hand tests/golden/allegro_hand.npz --out profiles/grasp_close.txt`, "
         f"one {torch.cuda.get_device_name(0)}",
         f"# KinematicGrasp.grasp_table: icosphere-{a.level} ({len(f)} faces, radius {a.radius} m, scaled per axis by 0.8..1.2) x {a.actions} "
         f"actions, steps {a.steps}; {a.warmup} warm-up, {a.rounds} rounds of {a.calls} calls; ms, median (p10, p90)",
         "# THE CLOSING RULE IS A KINEMATIC STAND-IN FOR PYBULLET'S stepSimulation: no frame has been compared with pybullet's",
         "# recorded numbers, not a gate: the parent commit cannot grasp"]
result = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "actions": a.actions, "faces": int(len(f)), "sizes": {}}
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
