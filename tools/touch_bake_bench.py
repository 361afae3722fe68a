#!/usr/bin/env python
"""The touch-chart bake and the one-launch chart head (``ops.touch_chart_head``, csrc/chart_head.hip) against the formulation they
replace, by ``ab_protocol.py``: the forms ALTERNATE in one process, every call with device events around it and the host clock
from an idle device to the end of the work.

1. The head alone at n = 12 (one environment step: 3 elements x 4 fingers) and n = 600 (x 50 candidates): ``fused`` is one
   ``ops.touch_chart_head`` call with ``want_slots``, ``torch`` the parent's own lines after the convolutions, written out here
   (``touch_slots`` and ``Encoder.forward``: three ``Linear``, the template ``repeat`` and add, ``bmm``, two ``where``, the
   ``expand``), on the same features; both build the status code on the host and upload it, as ``touch_slots`` does.
2. ``scoring.touch_slots`` end to end at n = 600 (convolutions included), ``fused_head`` on against off.
3. ``touch_charts_batch`` of 8 objects (icosphere level 5, 50 actions, 4 fingers: 1600 rendered views) — ``nhwc``: as it stands
   (channels-last images into ``predict_features_nhwc``, then the head, on and off); ``nchw``: the formulation of
   ``ActiveTouch.build_touch_table`` (``movedim`` to channels first, ``/ 255``, ``touch_slots`` with the head off) — and
   ``save_touch_info`` on a tree of those objects, with its file writes: objects per second.

The rule for ``scoring.FUSED_HEAD_DEFAULT``: on only if the fused head's p90 lies below the torch tail's p10 at both sizes of 1, on
the host clock and on device events.  ``data_making.BAKE_FUSED_HEAD`` is the form of 3 with the lower median.
Not measured here: a data-set-scale run, and the recorded sampler on real files.

    python tools/touch_bake_bench.py --out profiles/touch_bake_ab.txt"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ab_protocol as ab  # noqa: E402  (tools/ is this script's directory)
from touch_table_bench import RADIUS, lattice_frames  # noqa: E402


def frames_of(n, seed):
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(n, 3, 3, generator=g, dtype=torch.float64))
    return q.float().contiguous(), (torch.rand(n, 3, generator=g) - 0.5) * 0.3


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", type=int, nargs="+", default=[12, 600])
    p.add_argument("--objects", type=int, default=8)
    p.add_argument("--actions", type=int, default=50)
    p.add_argument("--level", type=int, default=5, help="icosphere level of the rendered objects")
    p.add_argument("--bake-calls", type=int, default=5, help="timed calls per round and form of the bake (3)")
    ab.add_arguments(p, calls=20, rounds=3, warmup=5)
    a = ab.parse(p)
    ab.require_gpu("touch_bake_bench")
    from a3vt_amd import mesh, ops
    from a3vt_amd.pterotactyl.policies import rendered, scoring
    from a3vt_amd.pterotactyl.reconstruction.touch import model
    from a3vt_amd.pterotactyl.utility import data_making
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    net = model.Encoder().to(dev).eval()
    template = torch.from_numpy(mesh.load_asset("touch_chart")[0]).float().to(dev)
    lines = [f"# profiles/touch_bake_ab.txt: `python tools/touch_bake_bench.py --out profiles/touch_bake_ab.txt`, one "
             f"{torch.cuda.get_device_name(0)}",
             f"# forms alternating in one process; {a.warmup} warm-up calls, {a.rounds} rounds of {a.calls} timed calls per form "
             f"({a.bake_calls} for the bake); ms; host wall: idle device to the end of the work",
             "# not measured: a data-set-scale run; the recorded sampler on real files"]
    verdict = []
    for n in a.sizes:                                                                  # 1. the head alone
        g = torch.Generator().manual_seed(n)
        features = (torch.randn(n, 512, generator=g) * 2.0).to(dev)
        rot, pos = (t.to(dev) for t in frames_of(n, n + 1))
        status = np.array([("touch", "touch", "no_touch", "touch", "no_intersection")[i % 5] for i in range(n)], dtype=object)
        ref = {"rot": rot, "pos": pos}

        def code_of():                                                                 # touch_slots' own line: built on the host, uploaded
            return torch.from_numpy(np.where(status == "touch", 2, np.where(status == "no_touch", 1, 0)).astype(np.float32)).to(dev)

        def tail():                                      # the parent's lines after the convolutions: touch_slots + Encoder.forward
            code = code_of()
            verts = template.to(dev).view(1, -1, 3).repeat(n, 1, 1)
            with torch.no_grad():
                pred = net.transform_verts(verts + net.fc(features).view(-1, verts.shape[1], 3), ref)
            code = code.view(n, 1, 1)
            charts = torch.where(code == 2, pred, torch.where(code == 1, pos.view(n, 1, 3).expand_as(pred), torch.zeros_like(pred)))
            masks = code.expand(n, verts.shape[1], 1)
            return charts.reshape(n, verts.shape[1], 3).contiguous(), masks.reshape(n, verts.shape[1], 1).contiguous()

        def fused():                                     # what touch_slots does instead with fused_head
            return ops.touch_chart_head(features, net.fc, template, rot, pos, code_of().reshape(n).to(torch.int32), want_slots=True)[1:]
        forms = {"fused": fused, "torch": tail}
        diff = (forms["fused"]()[0] - forms["torch"]()[0]).abs().max().item()
        res = ab.alternate(forms, a.calls, a.rounds, a.warmup, host_stops="after")
        lines.append(f"# 1. the head alone, n = {n}: max |fused - torch| = {diff:.3e}")
        won = [ab.report(f"   n = {n}, {clock}", {k: {clock: v[clock]} for k, v in res.items()}, "fused", "torch", lines, clock=clock)
               for clock in ab.CLOCKS]
        verdict.append(all(won))
    lines.append(f"# rule for scoring.FUSED_HEAD_DEFAULT (fused p90 below torch p10 at every size, on both clocks): met = {all(verdict)}")

    n = max(a.sizes)                                                                   # 2. touch_slots end to end
    touch = torch.rand(n, 3, 121, 121, generator=torch.Generator().manual_seed(3)).to(dev)
    rot, pos = frames_of(n, 4)
    status = [("touch", "touch", "no_touch", "touch", "no_intersection")[i % 5] for i in range(n)]
    forms = {name: (lambda on=on: scoring.touch_slots(net, touch, {"rot": rot, "pos": pos}, status, template, fused_head=on))
             for name, on in (("fused", True), ("torch", False))}
    diff = (forms["fused"]()[0] - forms["torch"]()[0]).abs().max().item()
    res = ab.alternate(forms, a.calls, a.rounds, a.warmup, host_stops="after")
    lines.append(f"# 2. scoring.touch_slots end to end, n = {n}: max |fused - torch| = {diff:.3e}")
    for clock in ab.CLOCKS:
        ab.report(f"   n = {n}, {clock}", {k: {clock: v[clock]} for k, v in res.items()}, "fused", "torch", lines, clock=clock)

    objects = [f"object{e}" for e in range(a.objects)]                                 # 3. the bake
    v, f = mesh.icosphere(a.level, RADIUS)
    fpos, frot = lattice_frames(a.objects * a.actions * 4)
    fpos, frot = fpos.reshape(a.objects, a.actions, 4, 3), frot.reshape(a.objects, a.actions, 4, 3, 3)
    frames = {(o, k): (fpos[e, k], frot[e, k], np.ones(4, bool)) for e, o in enumerate(objects) for k in range(a.actions)}
    sampler = rendered.RenderedSampler(frames, {o: (v, f.astype(np.int32)) for o in objects}, to_host=False)
    names = ["/data/object_info/" + o for o in objects]

    def nchw():
        sampler.load_objects(names)
        table = sampler.sample_table(a.actions, fingers=None, to_host=False)
        codes = table["touch_code"].to(dev)
        status = np.array(["no_intersection", "no_touch", "touch"], dtype=object)[codes.cpu().numpy()]
        images = table["touch_signal"].to(torch.uint8).float().movedim(-1, -3) / 255.0
        charts, masks = scoring.touch_slots(net, images, {"rot": table["finger_transform_rot_M"], "pos": table["finger_transfrom_pos"]},
                                            status, template, fused_head=False)
        return torch.cat((charts, masks), dim=-1)
    forms = {"nhwc": lambda: data_making.touch_charts_batch(sampler, net, template, names, a.actions, fused_head=True),
             "nhwc_off": lambda: data_making.touch_charts_batch(sampler, net, template, names, a.actions, fused_head=False),
             "nchw": nchw}
    diff = (forms["nhwc"]() - forms["nchw"]()).abs().max().item()
    res = ab.alternate(forms, a.bake_calls, a.rounds, 2, host_stops="after")
    lines.append(f"# 3. touch_charts_batch, {a.objects} objects (icosphere {a.level}) x {a.actions} actions x 4 fingers = "
                 f"{a.objects * a.actions * 4} views: max |nhwc - nchw| = {diff:.3e}")
    for new in ("nhwc", "nhwc_off"):
        ab.report(f"   {new} against nchw, host", {k: {"host": res[k]["host"]} for k in (new, "nchw")}, new, "nchw", lines, clock="host")
    for name in forms:
        lines.append(f"#   {name:8s}: {a.objects / (res[name]['host']['median'] * 1e-3):8.1f} objects/s without the file writes")
    faster = "nhwc" if res["nhwc"]["host"]["median"] <= res["nhwc_off"]["host"]["median"] else "nhwc_off"
    lines.append(f"#   the lower median: {faster} -> data_making.BAKE_FUSED_HEAD = {faster == 'nhwc'}")
    with tempfile.TemporaryDirectory() as root:
        for o in objects:
            os.makedirs(os.path.join(root, "grasp_info", o))
            os.makedirs(os.path.join(root, "object_info"), exist_ok=True)
            np.save(os.path.join(root, "object_info", f"{o}_verts.npy"), v)
        write = lambda: data_making.save_touch_info(root, encoder=net, sampler=sampler, batch=a.objects, num_actions=a.actions,  # noqa: E731
                                                    overwrite=True)
        res = ab.alternate({"save": write}, a.bake_calls, a.rounds, 2, clocks=("host",))
        counts = write()
    lines.append(f"#   save_touch_info (overwrite, {counts['written']} files of {a.actions * 4 * 25 * 4 * 4} bytes, temporary directory): "
                 f"median {res['save']['host']['median']:9.2f}  p10 {res['save']['host']['p10']:9.2f}  p90 {res['save']['host']['p90']:9.2f}"
                 f" = {a.objects / (res['save']['host']['median'] * 1e-3):8.1f} objects/s with the file writes; views by code: "
                 f"{counts['touch']} touch, {counts['no_touch']} no_touch, {counts['no_intersection']} no_intersection")
    ab.emit(lines, a.out)


if __name__ == "__main__":
    main()
