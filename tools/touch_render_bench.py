#!/usr/bin/env python
"""Time ``ops.touch_render`` (``a3vt_touch_render``, csrc/touch_render.hip) on one GPU.

Workload: an icosphere-5 (20 480 faces) of radius 0.16 at the origin; finger frames spread over it (a Fibonacci lattice), each
0.012 above the surface and looking at the centre, so every view touches.  Batch sizes: I = 12 (one ``RenderedSampler.sample`` at
E = 3) and I = 600 (one ``sample_many`` at K = 50).

Per batch size, device events around each call after the warm-up, median / p10 / p90 (``ab_protocol.stats``) in ms of
    render   the whole call (both launches, all outputs),
    finish   ``ops.touch_finish`` on the depth maps of that call (the second launch alone),
    depth    the first launch: render - finish of the same round (a difference of two measurements, not an event pair of its own),
and from them the ray-triangle tests per second of the depth launch.  The tests a launch makes are counted on the host by restating
the kernel's cull (bounding sphere against the tile's four side planes and the depth range) in NumPy for the first views of the
batch: a tile casts its 256 rays at every surviving face.

    python tools/touch_render_bench.py --out profiles/touch_render.txt"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ab_protocol as ab  # noqa: E402  (tools/ is this script's directory)
from a3vt_amd import mesh, ops  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--sizes", default="12,600")
ab.add_arguments(p, calls=100, rounds=None, warmup=20, what="batch size")
p.add_argument("--level", type=int, default=5)
p.add_argument("--stat-views", type=int, default=3, help="views whose cull is restated on the host")
a = ab.parse(p)
if a.warmup < 20 or a.calls < 100:
    raise SystemExit("touch_render_bench: at least 20 warm-up and 100 timed calls")
RADIUS, LIFT, RES, TILE = 0.16, 0.012, 121, 16
dev = torch.device("cuda", 0)


def frames(n):
    """n finger frames on a Fibonacci lattice: pos above the surface, rot's first column (the finger's +x) towards the centre."""
    i = np.arange(n) + 0.5
    z, phi = 1 - 2 * i / n, np.pi * (1 + 5 ** 0.5) * i
    normal = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1)
    x = -normal
    helper = np.where(np.abs(x[:, 2:3]) < 0.9, [[0.0, 0.0, 1.0]], [[1.0, 0.0, 0.0]])
    y = np.cross(helper, x)
    y /= np.linalg.norm(y, axis=1, keepdims=True)
    return (normal * (RADIUS + LIFT)).astype(np.float32), np.stack([x, y, np.cross(x, y)], 2).astype(np.float32)


def survivors(verts, faces, pos, rot, yfov, znear, zfar):
    """The kernel's cull in NumPy for one view -> faces surviving per tile, summed over the 64 tiles."""
    C = rot.astype(np.float64) @ np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])
    tri = verts[faces].astype(np.float64)
    centre = tri.mean(1)
    rad = np.linalg.norm(tri - centre[:, None], axis=2).max(1)
    q = (centre - pos) @ C
    w = -q[:, 2]
    rs = rad * 1.001 + 1e-6 * (np.abs(q[:, 0]) + np.abs(q[:, 1]) + np.abs(w))
    t = np.tan(yfov / 2)
    total = 0
    for ty in range(8):
        yt, yb = (1 - ty * TILE / RES * 2) * t, (1 - min(ty * TILE + TILE, RES) / RES * 2) * t
        for tx in range(8):
            xl, xr = (tx * TILE / RES * 2 - 1) * t, (min(tx * TILE + TILE, RES) / RES * 2 - 1) * t
            keep = ((q[:, 0] - xl * w) / np.sqrt(1 + xl * xl) >= -rs) & ((xr * w - q[:, 0]) / np.sqrt(1 + xr * xr) >= -rs) & \
                   ((q[:, 1] - yb * w) / np.sqrt(1 + yb * yb) >= -rs) & ((yt * w - q[:, 1]) / np.sqrt(1 + yt * yt) >= -rs) & \
                   (w + rs >= znear) & (w - rs <= zfar)
            total += int(keep.sum())
    return total


stats, source = ab.stats, ab.CudaSource()            # p10 / p90 by np.percentile, as every tool's; device events per call


def timed(fn):
    return ab.time_call(fn, source)["device"]


v, f = mesh.icosphere(a.level, RADIUS)
verts, faces = torch.from_numpy(v).to(dev), torch.from_numpy(f.astype(np.int32)).to(dev)
offsets = torch.tensor([0, len(f)], dtype=torch.int32, device=dev)
cam = ops.TOUCH_DEFAULTS
lines = [f"# profiles/touch_render.txt: `python tools/touch_render_bench.py --out profiles/touch_render.txt`, one "
         f"{torch.cuda.get_device_name(0)}",
         f"# icosphere-{a.level} ({len(f)} faces) of radius {RADIUS}, fingers {LIFT} above it looking at the centre; device events per "
         f"call, {a.warmup} warm-up and {a.calls} timed calls; ms",
         "# no comparison: the parent commit cannot render, and pyrender is not available"]
result = {"device": torch.cuda.get_device_name(0), "faces": int(len(f)), "warmup": a.warmup, "calls": a.calls, "sizes": {}}
for size in (int(s) for s in a.sizes.split(",")):
    pos, rot = frames(size)
    pos_d, rot_d, which = torch.from_numpy(pos).to(dev), torch.from_numpy(rot).to(dev), torch.zeros(size, dtype=torch.int32, device=dev)
    render = lambda: ops.touch_render(verts, faces, offsets, which, pos_d, rot_d)  # noqa: E731
    out = render()
    touching = int(out["status"].sum())
    finish = lambda: ops.touch_finish(out["depth"], pos_d, rot_d)  # noqa: E731
    for _ in range(a.warmup):
        render()
        finish()
    torch.cuda.synchronize()
    t_render, t_finish = [], []
    for _ in range(a.calls):
        t_render.append(timed(render))
        t_finish.append(timed(finish))
    n_stat = min(a.stat_views, size)
    kept = np.mean([survivors(v, f, pos[i], rot[i], cam["yfov"], cam["znear"], cam["zfar"]) for i in range(n_stat)])
    entry = {"render": stats(t_render), "finish": stats(t_finish), "depth": stats(np.array(t_render) - np.array(t_finish)),
             "views_touching": touching, "surviving_share": float(kept / (64 * len(f))), "tests_per_view": float(kept * 256)}
    entry["ray_triangle_tests_per_s"] = entry["tests_per_view"] * size / (entry["depth"]["median"] * 1e-3)
    result["sizes"][str(size)] = entry
    lines.append(f"# I = {size} ({touching} views touch; {out['count'].float().mean().item():.0f} contact points per view)")
    for name in ("render", "depth", "finish"):
        s = entry[name]
        lines.append(f"#   {name:7s} median {s['median']:9.4f}  p10 {s['p10']:9.4f}  p90 {s['p90']:9.4f}")
    lines.append(f"#   cull: {100 * entry['surviving_share']:.3f} % of (tile, face) pairs survive (first {n_stat} views), "
                 f"{entry['tests_per_view']:.3e} ray-triangle tests per view, {entry['ray_triangle_tests_per_s']:.3e} per second of the "
                 f"depth launch")
lines.append(json.dumps(result))
ab.emit(lines, a.out)
