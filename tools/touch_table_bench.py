#!/usr/bin/env python
"""The per-episode touch table of ``ActiveTouch`` (``args.touch_table``) against the plain path, which asks the sampler and runs the
touch encoder at every step and for every candidate: E = 3 elements, A = K = 50 actions, 30 000 surface points and 30 000-point
clouds, 20 GCN layers x 300, both chart topologies (``finger`` and four fingers), and both samplers this package ships:

* ``recorded``: a ``RecordedSampler`` over synthetic records (``tools/env_bench.py``'s);
* ``rendered``: a ``RenderedSampler`` with ``to_host=True``, as the environment gets it today, on the icosphere-5 scene of
  ``tools/touch_render_bench.py`` (every object is that sphere; the frames of an object's A x 4 fingers lie on a Fibonacci
  lattice above it and look at its centre, so every view touches).

Protocol (``tools/ab_protocol.py``): table on and off alternate call by call in one process on one environment
(``args.touch_table`` switched per call).  Three operations are timed, each with device events around the call and the host clock
around the same window, stopped after a device synchronise: one ``reset`` (where the table is paid for), one ``greedy_choice`` and
one ``step`` (each after an untimed ``reset`` with the call's knob).  From the medians (host wall) the tool derives the number of
steps after which the table has paid for itself, for an episode of greedy steps (``greedy_choice`` + ``step``) and for an episode of
plain steps.  Not measured: a dataset tree as the frame source (600 ``*_ref_frame.npy`` reads per greedy step on the plain path),
and the reference's simulator.

    python tools/touch_table_bench.py --out profiles/touch_table_ab.txt"""
import argparse
import json
import os
import sys
import tempfile
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ab_protocol as ab  # noqa: E402  (tools/ is this script's directory)
import env_bench  # noqa: E402

RADIUS, LIFT = 0.16, 0.012                       # tools/touch_render_bench.py's scene
OPERATIONS = ("reset", "greedy_choice", "step")


def lattice_frames(n):
    """n finger frames on a Fibonacci lattice above the sphere, each finger's +x towards the centre (touch_render_bench's)."""
    i = np.arange(n) + 0.5
    z, phi = 1 - 2 * i / n, np.pi * (1 + 5 ** 0.5) * i
    normal = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1)
    x = -normal
    helper = np.where(np.abs(x[:, 2:3]) < 0.9, [[0.0, 0.0, 1.0]], [[1.0, 0.0, 0.0]])
    y = np.cross(helper, x)
    y /= np.linalg.norm(y, axis=1, keepdims=True)
    return (normal * (RADIUS + LIFT)).astype(np.float32), np.stack([x, y, np.cross(x, y)], 2).astype(np.float32)


def make_sampler(kind, objects, actions, level):
    from a3vt_amd import mesh
    from a3vt_amd.pterotactyl.policies import recorded, rendered
    if kind == "recorded":
        return recorded.RecordedSampler(env_bench.synthetic_records(objects, actions, 1))
    v, f = mesh.icosphere(level, RADIUS)
    pos, rot = lattice_frames(len(objects) * actions * 4)
    pos, rot = pos.reshape(len(objects), actions, 4, 3), rot.reshape(len(objects), actions, 4, 3, 3)
    frames = {(o, a): (pos[e, a], rot[e, a], np.ones(4, bool)) for e, o in enumerate(objects) for a in range(actions)}
    return rendered.RenderedSampler(frames, {o: (v, f.astype(np.int32)) for o in objects}, to_host=True)


def measure(kind, finger, a, root):
    from a3vt_amd.pterotactyl.policies import environment
    from a3vt_amd.pterotactyl.reconstruction.touch import model as touch_model
    from a3vt_amd.pterotactyl.reconstruction.vision import model as vision_model
    from a3vt_amd.pterotactyl.utility import utils
    from a3vt_amd.synthetic import gt_cloud
    tag = "finger" if finger else "four_fingers"
    config = dict(use_img=False, use_touch=True, finger=finger, num_grasps=5, num_GCN_layers=a.layers, hidden_GCN_size=300, cut=0.33)
    info, verts = utils.load_mesh_vision(SimpleNamespace(**config), "vision_charts")
    torch.manual_seed(0)
    deform = vision_model.Deformation(info, verts, SimpleNamespace(**config))
    with torch.no_grad():
        for gcn in (deform.mesh_deform_1, deform.mesh_deform_2):
            gcn.layers[-1].weight.mul_(0.02)
            gcn.layers[-1].bias.mul_(0.02)
    torch.manual_seed(0)
    where = os.path.join(root, kind, tag)
    locations = {"vision_location": env_bench.write_checkpoint(os.path.join(where, "vision"), config, deform),
                 "touch_location": env_bench.write_checkpoint(os.path.join(where, "touch"), {}, touch_model.Encoder())}
    args = SimpleNamespace(seed=0, eval=True, pretrained_recon=False, use_img=False, use_touch=True, finger=finger, num_grasps=5,
                           use_latent=False, num_actions=a.candidates, budget=5, env_batch_size=a.env, number_points=a.points,
                           loss_coeff=9000.0, batched_greedy=True, touch_table=False, **locations)
    objects = [f"object{e}" for e in range(a.env)]

    class Environment(environment.ActiveTouch):
        def get_loaders(self):                                       # no dataset: the batch below is synthetic
            pass

    env = Environment(args, sampler=make_sampler(kind, objects, a.candidates, a.level))
    g = torch.Generator().manual_seed(2)
    env.score_samples = (torch.randint(0, info["faces"].shape[0], (3, a.env, a.points), generator=g).to(torch.int32),
                         torch.rand(3, a.env, a.points, generator=g), torch.rand(3, a.env, a.points, generator=g))
    batch = {"names": ["/data/object_info/" + o for o in objects], "gt_points": gt_cloud(a.env, a.points, 3), "img": torch.zeros(a.env, 1)}
    actions = np.arange(a.env) % a.candidates
    seen = {}

    def knob(name):
        args.touch_table = name == "table"

    def fresh_episode(name):                                          # not timed
        knob(name)
        env.reset(batch)

    def call(operation, name):
        if operation == "reset":
            return lambda: env.reset(batch)
        if operation == "step":
            return lambda: seen.__setitem__(("step", name), env.step(actions)[0]["score"])
        return lambda: seen.__setitem__(("greedy_choice", name), env.greedy_choice())

    rec = {"sampler": kind, "topology": tag, "env": a.env, "actions": a.candidates, "points": a.points, "layers": a.layers,
           "calls": a.calls, "warmup": a.warmup}
    for operation in OPERATIONS:
        res = ab.alternate({name: call(operation, name) for name in ("table", "plain")}, 1, a.calls, a.warmup, host_stops="after",
                           before=knob if operation == "reset" else fresh_episode)
        rec[operation] = {name: dict(host=res[name]["host"], device=res[name]["device"]) for name in res}
        rec[operation]["table_p90_below_plain_p10"] = ab.wins(res, "table", "plain", "host")
    choice_t, choice_p = seen["greedy_choice", "table"], seen["greedy_choice", "plain"]
    rec["same_actions"] = bool(np.array_equal(choice_t[0], choice_p[0]))
    rec["table_rel_diff"] = float(((choice_t[1] - choice_p[1]).abs() / choice_p[1].abs()).max())
    rec["step_score_rel_diff"] = float(((seen["step", "table"] - seen["step", "plain"]).abs() / seen["step", "plain"].abs()).max())
    host = lambda operation, name: rec[operation][name]["host"]["median"]  # noqa: E731
    paid = host("reset", "table") - host("reset", "plain")
    for episode, operations in (("greedy", ("greedy_choice", "step")), ("plain", ("step",))):
        saved = sum(host(o, "plain") - host(o, "table") for o in operations)
        rec[f"{episode}_steps_to_pay"] = paid / saved if saved > 0 else None
    return rec


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--env", type=int, default=3)
    p.add_argument("--candidates", type=int, default=50, help="A = K: the actions of the table and the candidates of a greedy step")
    p.add_argument("--points", type=int, default=30000)
    p.add_argument("--layers", type=int, default=20)
    p.add_argument("--level", type=int, default=5, help="icosphere level of the rendered scene")
    p.add_argument("--samplers", default="recorded,rendered")
    ab.add_arguments(p, calls=10, rounds=None, warmup=2, what="form and operation")
    a = ab.parse(p)
    ab.require_gpu("touch_table_bench")
    lines = [f"# profiles/touch_table_ab.txt: `python tools/touch_table_bench.py --out profiles/touch_table_ab.txt`, one "
             f"{torch.cuda.get_device_name(0)}",
             f"# ActiveTouch with args.touch_table on (table) and off (plain), alternating call by call; E = {a.env}, A = K = "
             f"{a.candidates}, {a.points} points, {a.layers} x 300; {a.warmup} warm-up and {a.calls} timed calls per form and operation; ms",
             "# not measured: a dataset tree as the frame source, the reference's simulator"]
    with tempfile.TemporaryDirectory() as root:
        for kind in a.samplers.split(","):
            for finger in (True, False):
                rec = measure(kind, finger, a, root)
                lines.append(f"# {kind} sampler, {rec['topology']}: same actions {rec['same_actions']}, candidate tables differ by "
                             f"{rec['table_rel_diff']:.1e}, step scores by {rec['step_score_rel_diff']:.1e} (relative)")
                for operation in OPERATIONS:
                    for name in ("table", "plain"):
                        h, d = rec[operation][name]["host"], rec[operation][name]["device"]
                        lines.append(f"#   {operation:>13} {name:>5}: host wall median {h['median']:9.2f}  p10 {h['p10']:9.2f}  p90 "
                                     f"{h['p90']:9.2f}   device events median {d['median']:9.2f}  p10 {d['p10']:9.2f}  p90 {d['p90']:9.2f}")
                pay = lambda v: "never" if v is None else f"{v:.2f}"  # noqa: E731
                lines.append(f"#   the table has paid for itself after {pay(rec['greedy_steps_to_pay'])} greedy steps, or "
                             f"{pay(rec['plain_steps_to_pay'])} plain steps (host wall medians)")
                lines.append(json.dumps(rec))
    ab.emit(lines, a.out)


if __name__ == "__main__":
    main()
