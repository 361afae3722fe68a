#!/usr/bin/env python
"""The data-set bake's reads and writers, by ``ab_protocol.py``: the forms ALTERNATE in one process; the clock is the host wall per
call, from an idle device to the result on the host (both forms end there).

(a) ``RenderedSampler.sample_many(touch_point_cloud=True, to_host=True)`` with the clouds read back ``packed``
    (``ops.touch_pack``, csrc/touch_pack.hip: the offsets, one small read, then the rows that exist) against ``padded`` (the path
    the package had: the whole (I, 14641, 3) points buffer copied, sliced on the host), at I = 12 (one environment step: 3 objects
    x 4 fingers) and I = 1600 (one bake batch: 8 objects x 50 actions x 4 fingers).  Both forms render the same views and copy the
    same fp32 images and depths; only the clouds' way to the host differs, and the results are the same bits (checked here).
    Two scenes: every pixel in contact (the packed form has nothing to leave out), and a disc of contact (``scene``).
    The rule for ``rendered.PACK_POINTS_DEFAULT`` and ``data_making.BAKE_PACK_POINTS``: on only if the packed form's p90 lies below
    the padded form's p10 at both sizes, in both scenes.
(b) No A/B for the writers — the package could not write these files before: objects/s of ``save_image_info`` at batch 16 and of
    ``save_touch_signals`` at batch 8 (packed and padded), each with its file writes (a temporary directory) and without.

Objects are icospheres (level 5), frames on a Fibonacci lattice above them (``touch_table_bench.lattice_frames``).
Not measured here: a data-set-scale run, real ``grasp_info`` files, a file system other than the temporary directory's.

    python tools/touch_signals_bench.py --out profiles/touch_signals_ab.txt"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ab_protocol as ab  # noqa: E402  (tools/ is this script's directory)
from touch_table_bench import LIFT, RADIUS, lattice_frames  # noqa: E402


def scene(objects, actions, level, lift=LIFT):
    """``objects`` icospheres and a frame per (object, action, finger) ``lift`` above the surface, looking at the centre.  The
    sensor sees 0.025 deep: at ``touch_table_bench``'s lift of 0.012 every pixel of every view is in contact (14 641 points a view,
    the packed form's worst case: nothing to leave out); at 0.0249 the contact is a disc around the image's centre."""
    from a3vt_amd import mesh
    names = [f"object{e}" for e in range(objects)]
    v, f = mesh.icosphere(level, RADIUS)
    pos, rot = lattice_frames(objects * actions * 4)
    pos = (pos.astype(np.float64) * ((RADIUS + lift) / (RADIUS + LIFT))).astype(np.float32)
    pos, rot = pos.reshape(objects, actions, 4, 3), rot.reshape(objects, actions, 4, 3, 3)
    frames = {(o, k): (pos[e, k], rot[e, k], np.ones(4, bool)) for e, o in enumerate(names) for k in range(actions)}
    return names, {o: (v, f.astype(np.int32)) for o in names}, frames


def write_tree(root, names, geometry, frames):
    os.makedirs(os.path.join(root, "object_info"))
    for o in names:
        np.save(os.path.join(root, "object_info", f"{o}_verts.npy"), geometry[o][0])
        np.save(os.path.join(root, "object_info", f"{o}_faces.npy"), geometry[o][1])
    for (o, k), (pos, rot, _) in frames.items():
        d = os.path.join(root, "grasp_info", o, str(k))
        os.makedirs(d)
        for finger in range(4):
            np.save(os.path.join(d, f"{finger}_ref_frame.npy"), {"pos": pos[finger], "rot": rot[finger]}, allow_pickle=True)


def line(what, s, objects):
    return (f"#   {what}: median {s['median']:9.2f}  p10 {s['p10']:9.2f}  p90 {s['p90']:9.2f} ms = "
            f"{objects / (s['median'] * 1e-3):8.1f} objects/s")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--level", type=int, default=5, help="icosphere level of the objects")
    p.add_argument("--actions", type=int, default=50)
    p.add_argument("--image-batch", type=int, default=16)
    p.add_argument("--signal-batch", type=int, default=8)
    p.add_argument("--lifts", type=float, nargs="+", default=[LIFT, 0.0249], help="heights of the fingers above the surface in (a)")
    p.add_argument("--big-calls", type=int, default=4, help="timed calls per round and form at I = 1600 and of the writers")
    ab.add_arguments(p, calls=20, rounds=3, warmup=3)
    a = ab.parse(p)
    ab.require_gpu("touch_signals_bench")
    from a3vt_amd.pterotactyl.policies import rendered
    from a3vt_amd.pterotactyl.utility import data_making
    lines = [f"# profiles/touch_signals_ab.txt: `python tools/touch_signals_bench.py --out profiles/touch_signals_ab.txt`, one "
             f"{torch.cuda.get_device_name(0)}",
             f"# forms alternating in one process; {a.warmup} warm-up calls, {a.rounds} rounds of {a.calls} timed calls per form "
             f"({a.big_calls} at I = 1600 and for the writers); ms; host wall per call: idle device to the result on the host",
             "# not measured: a data-set-scale run; real grasp_info files; a file system other than the temporary directory's"]
    verdict = []
    for lift, objects, lists in ((h, o, n) for h in a.lifts for o, n in ((3, 1), (a.signal_batch, a.actions))):   # (a) I = 12, 1600
        names, geometry, frames = scene(objects, a.actions, a.level, lift)
        sampler = rendered.RenderedSampler(frames, geometry, to_host=True)
        sampler.load_objects(["/data/object_info/" + o for o in names])
        action_lists = [[k] * objects for k in range(lists)]
        forms = {name: (lambda on=on: sampler.sample_many(action_lists, touch_point_cloud=True, pack_points=on))
                 for name, on in (("packed", True), ("padded", False))}
        x, y = forms["packed"](), forms["padded"]()
        clouds = [(c, d) for r, s in zip(x, y) for cr, dr in zip(r["touch_point_cloud"], s["touch_point_cloud"]) for c, d in zip(cr, dr)]
        assert all(c.shape == d.shape and np.array_equal(c.view(np.uint32), d.view(np.uint32)) for c, d in clouds)
        rows, I = sum(len(c) for c, _ in clouds), objects * lists * 4
        big = I > 100
        res = ab.alternate(forms, a.big_calls if big else a.calls, a.rounds, 1 if big else a.warmup, clocks=("host",))
        won = ab.report(f"(a) sample_many(touch_point_cloud=True, to_host=True), I = {I} views {lift} above the surface: {rows} contact "
                        f"points ({rows / (I * 14641):.0%} of the pixels) = {rows * 12 / 1e6:.2f} MB "
                        f"packed against {I * 14641 * 12 / 1e6:.2f} MB padded", res, "packed", "padded", lines, clock="host")
        verdict.append(won)
    lines.append(f"# rule for rendered.PACK_POINTS_DEFAULT and data_making.BAKE_PACK_POINTS (packed p90 below padded p10 at both sizes, in every scene): "
                 f"met = {all(verdict)}" + ("" if all(verdict) else ": the defaults stay off, the kernel stays an option (pack_points=True)"))

    lines.append("# (b) the writers: no A/B, the files could not be written before")
    names, geometry, frames = scene(a.image_batch, 1, a.level)                         # save_image_info
    with tempfile.TemporaryDirectory() as root:
        write_tree(root, names, geometry, {})
        sampler = rendered.RenderedSampler({}, geometry, to_host=True)
        paths = [os.path.join(root, "object_info", o) for o in names]

        def images_only():
            sampler.load_objects(paths)
            return sampler.vision_images()
        forms = {"render": images_only, "save": lambda: data_making.save_image_info(root, batch=a.image_batch, overwrite=True)}
        res = ab.alternate(forms, a.big_calls, a.rounds, 1, clocks=("host",))
        assert forms["save"]()["written"] == a.image_batch
    lines.append(line(f"save_image_info, {a.image_batch} objects (icosphere {a.level}) in one batch, 256 x 256, without the file writes",
                      res["render"]["host"], a.image_batch))
    lines.append(line(f"save_image_info, the same with the file writes ({a.image_batch} files of 196608 bytes)", res["save"]["host"],
                      a.image_batch))
    for lift in a.lifts:                                                               # save_touch_signals
        names, geometry, frames = scene(a.signal_batch, a.actions, a.level, lift)
        with tempfile.TemporaryDirectory() as root:
            write_tree(root, names, geometry, frames)
            forms = {f"{how}{'' if write else '_dry'}": (lambda on=on, write=write: data_making.save_touch_signals(
                root, batch=a.signal_batch, num_actions=a.actions, overwrite=True, pack_points=on, write=write))
                for how, on in (("packed", True), ("padded", False)) for write in (False, True)}
            res = ab.alternate(forms, a.big_calls, a.rounds, 1, clocks=("host",))
            counts = forms["packed"]()
        lines.append(f"#   save_touch_signals, {a.signal_batch} objects x {a.actions} actions x 4 fingers = {counts['views']} views in one batch, "
                     f"{lift} above the surface: {counts['touch']} touch, {counts['no_touch']} no_touch, {counts['no_intersection']} "
                     "no_intersection")
        for name, what in (("packed_dry", "packed, without the file writes"), ("packed", f"packed, with them ({2 * counts['touch']} files)"),
                           ("padded_dry", "padded, without the file writes"), ("padded", "padded, with them")):
            lines.append(line(f"save_touch_signals {what}", res[name]["host"], a.signal_batch))
    ab.emit(lines, a.out)


if __name__ == "__main__":
    main()
