#!/usr/bin/env python
"""Time one ``render_representations``-shaped ``ops.scene_render`` call (``a3vt_scene_render``, csrc/scene_render.hip) on one GPU.

Workload per object, three 512 x 512 images from the reference's camera and lights, as ``utility/pretty_render.py`` renders them:
    mesh          the prediction: the packaged 2 304-face chart atlas with ``add_faces``' tripled faces (6 912), scaled to the
                  objects' size,
    points        100 000 area-weighted samples of an icosphere of radius 0.2 as spheres of radius 0.01,
    ground_truth  an icosphere-5 (20 480 faces, tripled: 61 440) of radius 0.2.
Batch sizes: 1 object (3 images) and 16 (48 images: a validation batch), every object turned a little differently, all in one
call.  Device events around each call after the warm-up; median / p10 / p90 (``ab_protocol.stats``) in ms of the whole call, and of
calls holding only the mesh, only the points or only the ground-truth images of the same objects.

    python tools/scene_render_bench.py --out profiles/scene_render.txt"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ab_protocol as ab  # noqa: E402  (tools/ is this script's directory)
from a3vt_amd import mesh, ops  # noqa: E402
from a3vt_amd.pterotactyl.utility import pretty_render, utils  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--sizes", default="1,16")
ab.add_arguments(p, calls=50, rounds=None, warmup=10, what="batch size")
p.add_argument("--points", type=int, default=100000)
p.add_argument("--level", type=int, default=5)
a = ab.parse(p)
ab.require_gpu("scene_render_bench")
if a.warmup < 10 or a.calls < 50:
    raise SystemExit("scene_render_bench: at least 10 warm-up and 50 timed calls")
dev = torch.device("cuda", 0)
source = ab.CudaSource()
KINDS = ("mesh", "points", "ground_truth")


def timed(fn):
    return ab.time_call(fn, source)["device"]


def objects(n):
    """n objects -> per kind a list of ``CameraRenderer.scene()`` entries."""
    atlas_v, atlas_f = mesh.load_asset("vision_charts")
    atlas_v = atlas_v / np.abs(atlas_v).max() * 0.2
    ico_v, ico_f = mesh.icosphere(a.level, 0.2)
    camera = pretty_render.CameraRenderer()
    torch.manual_seed(0)
    out = {k: [] for k in KINDS}
    for i in range(n):
        turn = utils.euler_matrix([0.1 * i, -0.07 * i, 0.3 * i]).astype(np.float32)
        truth = torch.from_numpy(ico_v @ turn.T).to(dev)
        cloud = utils.batch_sample(truth[None], torch.from_numpy(ico_f.astype(np.int32)).to(dev), num=a.points)[0]
        for kind, add in (("mesh", lambda: camera.add_object(atlas_v @ turn.T, utils.add_faces(atlas_f))),
                          ("points", lambda: camera.add_points(cloud, 0.01, ops.RENDER_DEFAULTS["colour"])),
                          ("ground_truth", lambda: camera.add_object(truth, utils.add_faces(ico_f)))):
            add()
            out[kind].append(camera.scene())
            camera.remove_objects()
    return out


def packed(scenes):
    """The arguments of the one ``ops.scene_render`` call ``pretty_render.render_batch`` makes for ``scenes``, built once: the timed
    call is the library's alone (no concatenation, no copy back)."""
    tables = pretty_render.scene_tables(scenes)
    return lambda: ops.scene_render(**tables, want_prim=False)


lines = [f"# profiles/scene_render.txt: `python tools/scene_render_bench.py --out profiles/scene_render.txt`, one {torch.cuda.get_device_name(0)}",
         f"# per object three 512 x 512 images: the chart atlas with tripled faces (6 912), {a.points} spheres of radius 0.01, an "
         f"icosphere-{a.level} with tripled faces; device events per call, {a.warmup} warm-up and {a.calls} timed calls; ms",
         "# no comparison: the parent commit cannot render, and pyrender is not available; the shader is Lambert, not pyrender's"]
result = {"device": torch.cuda.get_device_name(0), "points": a.points, "level": a.level, "warmup": a.warmup, "calls": a.calls, "sizes": {}}
for size in (int(s) for s in a.sizes.split(",")):
    scenes = objects(size)
    forms = {"all": packed([scenes[k][i] for i in range(size) for k in KINDS])}
    forms.update({k: packed(scenes[k]) for k in KINDS})
    for fn in forms.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(a.calls):
        for k, fn in forms.items():
            times[k].append(timed(fn))
    entry = {k: ab.stats(v) for k, v in times.items()}
    result["sizes"][str(size)] = entry
    lines.append(f"# {size} object(s), {3 * size} images in one call")
    for k, s in entry.items():
        lines.append(f"#   {k:12s} median {s['median']:9.4f}  p10 {s['p10']:9.4f}  p90 {s['p90']:9.4f}")
lines.append(json.dumps(result))
ab.emit(lines, a.out)
