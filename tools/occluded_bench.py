#!/usr/bin/env python
"""A/B of the occluded vision images (``RenderedSampler``'s ``vision_occluded``: the object with the posed hand in front) on one
GPU, by ``ab_protocol.py``: three forms ALTERNATING in one process, median (p10, p90).

    posed       ``ops.scene_render_posed`` (``a3vt_scene_render_posed``, csrc/posed_render.hip): instances of shared parts, no
                posed triangle is written out
    torch       what the parent commit allows: the triangles posed with torch ops (a gather of the template vertices, a batched
                product, an add), then the parent's ``ops.scene_render``.  The index tables of that gather, the face table and the
                colours depend on which grasps are placed, not on the poses: they are made AHEAD and not timed
    pose_parts  ``ops.pose_parts`` (one launch, and one read of ``inst_part`` to size its output), then ``ops.scene_render``

Sizes: I = 3 (one ``sample``) and I = 150 (a greedy step's K = 50 candidates x E = 3) images at 256 x 256, icosphere-5 objects
(20 480 faces, scaled per axis), the golden hand at the kinematic grasp's poses for actions 0 .. K - 1.  Device events, host wall up
to the end of the device's work, and the allocator's peak above what was held before the call.

The rule for ``POSED_RENDER_DEFAULT`` (``policies/rendered.py``): True only if posed's p90 lies below pose_parts' p10 at both sizes
(host wall; the device clock's verdict is printed beside it).

    python tools/occluded_bench.py --hand tests/golden/allegro_hand.npz --meshes tests/golden/allegro_hand_visual.npz \\
        --out profiles/occluded_vision_ab.txt

**Lambert shading, not pyrender's; the poses are the kinematic grasp's, not Bullet's.  Nothing here is compared with either.**"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ab_protocol as ab  # noqa: E402  (tools/ is this script's directory)
from a3vt_amd import mesh, ops  # noqa: E402
from a3vt_amd.pterotactyl.policies.rendered import RenderedSampler  # noqa: E402
from a3vt_amd.pterotactyl.simulator.hand import HandModel, HandVisual  # noqa: E402
from a3vt_amd.pterotactyl.simulator.physics.grasping import GraspFrames, KinematicGrasp  # noqa: E402

p = argparse.ArgumentParser()
ab.add_arguments(p, calls=5, rounds=6, warmup=3)
p.add_argument("--hand", default=None, help="a hand URDF or .npz (default: PTEROTACTYL_HAND)")
p.add_argument("--meshes", default=None, help="the hand's visual meshes: a meshes_obj folder or .npz (default: PTEROTACTYL_HAND_MESHES)")
p.add_argument("--level", type=int, default=5)
p.add_argument("--radius", type=float, default=0.06)
p.add_argument("--objects", type=int, default=3)
p.add_argument("--candidates", type=int, nargs="+", default=[1, 50], help="K per size: I = K x objects images")
p.add_argument("--side", type=int, default=256)
p.add_argument("--steps", type=int, default=64)
a = ab.parse(p)
ab.require_gpu("occluded_bench")
dev = torch.device("cuda", 0)
hand, visual = HandModel.load(a.hand), HandVisual.load(a.meshes)

v, f = mesh.icosphere(a.level)
v = np.asarray(v, np.float64)
v = v / np.linalg.norm(v, axis=1, keepdims=True) * a.radius
rng = np.random.default_rng(0)
geometry = {f"object{e}": ((v * (0.8 + 0.4 * rng.random(3))).astype(np.float32), np.asarray(f, np.int64)) for e in range(a.objects)}
frames = GraspFrames(KinematicGrasp(hand, steps=a.steps, device=dev), geometry, num_actions=50)
sampler = RenderedSampler(frames, geometry, hand_visual=visual, resolution=[a.side, a.side], to_host=False)
sampler.load_objects(list(geometry))
table = sampler.parts
D = ops.VISION_DEFAULTS
scene = dict(yfov=D["yfov"], znear=D["znear"], zfar=D["zfar"], width=a.side, height=a.side, lights=D["lights"], ambient=D["ambient"],
             background=D["background"], want_prim=False)
up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
fmt = lambda s: f"{s['median']:9.3f} ({s['p10']:9.3f}, {s['p90']:9.3f})"  # noqa: E731
no_spheres = (torch.zeros((0, 3), device=dev), torch.zeros(0, device=dev), torch.zeros((0, 3), dtype=torch.uint8, device=dev))

lines = [f"# profiles/occluded_vision_ab.txt: `python tools/occluded_bench.py --hand tests/golden/allegro_hand.npz --meshes "
         f"tests/golden/allegro_hand_visual.npz --out profiles/occluded_vision_ab.txt`, one {torch.cuda.get_device_name(0)}",
         f"# occluded vision images, {a.side} x {a.side}: {a.objects} icosphere-{a.level} objects ({len(f)} faces each, radius {a.radius} m, scaled "
         f"per axis by 0.8..1.2), the golden hand ({visual.num_faces} faces in 21 nodes) at the kinematic grasp's poses (steps {a.steps}); the forms "
         f"alternating in one process, {a.warmup} warm-up, {a.rounds} rounds of {a.calls} calls; ms, median (p10, p90)",
         "# LAMBERT SHADING, NOT PYRENDER'S; THE POSES ARE THE KINEMATIC GRASP'S, NOT BULLET'S: nothing here is compared with either",
         "# posed: ops.scene_render_posed; torch: triangles posed with torch ops (index tables made ahead), then ops.scene_render — the "
         "parent commit's means; pose_parts: ops.pose_parts, then ops.scene_render"]
result = {"device": torch.cuda.get_device_name(0), "side": a.side, "object_faces": int(len(f)), "hand_faces": visual.num_faces, "sizes": {}}
verdicts = []
for K in a.candidates:
    lists = [[k % 50] * a.objects for k in range(K)]
    t = sampler.occluded_instances(lists)
    I, N = K * a.objects, len(t["inst_part"])
    inst = [up(t[name]) for name in ("inst_part", "inst_pos", "inst_rot", "inst_rgb")]
    cam = (up(t["cam_pos"]), up(t["cam_rot"]))
    # the torch form's static tables: per materialised vertex its instance and template vertex; the faces; the colours
    m0 = ops.pose_parts(table, *inst, inst_offset=t["inst_offset"])
    part = t["inst_part"].astype(np.int64)
    counts = np.diff(table.vert_offset)[part]
    vert_inst = up(np.repeat(np.arange(N), counts))
    vert_template = up(np.concatenate([np.arange(table.vert_offset[q], table.vert_offset[q + 1]) for q in part]).astype(np.int64))
    static_faces, static_rgb, face_offset, images = m0["faces"], m0["face_rgb"], list(m0["face_offset"]), list(range(I))

    def posed():
        return ops.scene_render_posed(table, *inst, t["inst_offset"], *cam, **scene)["rgb"]

    def torch_form():
        verts = torch.bmm(inst[2][vert_inst], table.verts[vert_template].unsqueeze(2)).squeeze(2) + inst[1][vert_inst]
        return ops.scene_render(verts, static_faces, static_rgb, *no_spheres, face_offset, [0] * (I + 1), images, *cam, **scene)["rgb"]

    def pose_parts():
        m = ops.pose_parts(table, *inst, inst_offset=t["inst_offset"])
        return ops.scene_render(m["verts"], m["faces"], m["face_rgb"], *no_spheres, list(m["face_offset"]), [0] * (I + 1), images, *cam,
                                **scene)["rgb"]

    forms = {"posed": posed, "torch": torch_form, "pose_parts": pose_parts}
    got = {name: fn().cpu().numpy() for name, fn in forms.items()}
    peak = {}
    for name, fn in forms.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        held = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        peak[name] = (torch.cuda.max_memory_allocated() - held) / 2 ** 20
        del out
    res = ab.alternate(forms, a.calls, a.rounds, a.warmup, host_stops="after")
    hand_pixels = float((got["posed"] != 255).any(axis=-1).mean())
    lines.append(f"# I = {I} images (K = {K} x E = {a.objects}): {N} instances, {int(m0['face_offset'][-1])} materialised faces, "
                 f"{int(m0['vert_base'][-1])} vertices; pixels that are not background {hand_pixels:.3f}")
    for name in forms:
        lines.append(f"#   {name:10s} device events {fmt(res[name]['device'])}   host wall {fmt(res[name]['host'])}   allocator peak "
                     f"{peak[name]:8.2f} MiB")
    lines.append(f"#   images: posed == pose_parts bit for bit: {bool(np.array_equal(got['posed'], got['pose_parts']))}; posed == torch on "
                 f"{float((got['posed'] == got['torch']).all(axis=-1).mean()):.6f} of the pixels (torch's product rounds otherwise than the fma chain)")
    for old in ("torch", "pose_parts"):
        for clock in ("device", "host"):
            lines.append(f"#   {clock:6s} {old} / posed = {res[old][clock]['median'] / res['posed'][clock]['median']:.2f} (medians); posed p90 below "
                         f"{old} p10: {ab.wins(res, 'posed', old, clock)}")
    verdicts.append({clock: bool(ab.wins(res, "posed", "pose_parts", clock)) for clock in ("host", "device")})
    result["sizes"][I] = {"ms": res, "peak_mib": peak, "instances": N, "faces": int(m0["face_offset"][-1])}
met = all(x["host"] for x in verdicts)
lines += [f"# the rule for POSED_RENDER_DEFAULT (posed p90 below pose_parts p10 on host wall at both sizes): {'MET' if met else 'NOT MET'}"
          f" (on device events: {'met' if all(x['device'] for x in verdicts) else 'not met'})",
          "# not measured: pyrender's images, Bullet's poses, real objects, a data-set-scale run, other resolutions"]
result["rule_met"] = bool(met)
lines.append(json.dumps(result))
ab.emit(lines, a.out)
