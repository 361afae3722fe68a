#!/usr/bin/env python
"""Time ``data_making.extract_points_batch`` (``a3vt_voxel_surface`` + ``a3vt_voxel_points``, csrc/voxel.hip) against the reference's
formulation of the same recipe on one GPU, by ``ab_protocol.py``: the forms alternate, device events and host wall.

    new   one ``extract_points_batch`` call for the M meshes: the clear and seven kernels, one read of M counts, two kernels.
    old   per mesh, what ``utility/data_making.py::extract_points`` does, restated on torch ops on the same GPU with its host work
          kept: a level-by-level subdivision that grows one tensor per level and asks the host whether to go on, a Python loop over
          every occupied voxel for the depth maps, a Python loop over every depth-map pixel for the carving, SciPy's
          ``binary_fill_holes`` on the host, a 3 x 3 x 3 convolution for the surface, the realignment, the doubling and the gather.
Both get the meshes as device tensors and the same injected ``choices``, and both leave the clouds on the device (the host clock
stops after the closing synchronise).  The old form has no kernel of its own, so the result is a recorded number with its p10 / p90,
not a gate; the parent commit cannot make a cloud at all.

Sizes: an icosphere-5 (20 480 faces) at dim 128 with M = 1 and M = 16 (the copies scaled differently), and a mesh of one face across
the whole cube plus 20 000 faces smaller than a voxel.  Launches per ``new`` call are read from the library's counters.

    python tools/points_bench.py --out profiles/points_extract_ab.txt"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ab_protocol as ab  # noqa: E402  (tools/ is this script's directory)
from a3vt_amd import mesh, ops  # noqa: E402
from a3vt_amd.pterotactyl.utility import data_making  # noqa: E402

try:
    from scipy import ndimage
except Exception:   # the fill changes nothing on these grids (DESIGN: the carve argument); without SciPy the old form goes without it
    ndimage = None

p = argparse.ArgumentParser()
ab.add_arguments(p, calls=4, rounds=5, warmup=2)
p.add_argument("--dim", type=int, default=128)
p.add_argument("--num-points", type=int, default=30000)
p.add_argument("--level", type=int, default=5)
p.add_argument("--batch", type=int, default=16)
a = ab.parse(p)
ab.require_gpu("points_bench")
dev = torch.device("cuda", 0)


def old_form(verts, faces, dim, num_points, choices):
    """The reference's recipe for one mesh (see the module docstring), on ``verts``' device."""
    lo, hi = verts.min(), verts.max()
    unit = (verts - lo) / (hi - lo) - 0.5
    a_, b_, c_ = unit[faces[:, 0]], unit[faces[:, 1]], unit[faces[:, 2]]
    points = torch.cat((a_, b_, c_))
    limit = (1.0 / dim) ** 2
    while True:
        longest = torch.stack((((a_ - b_) ** 2).sum(1), ((b_ - c_) ** 2).sum(1), ((c_ - a_) ** 2).sum(1)), 1).max(1)[0]
        big = longest > limit
        if big.sum() == 0:                                       # (the per-level host read)
            break
        a_, b_, c_ = a_[big], b_[big], c_[big]
        ac, ab_, bc = (a_ + c_) / 2.0, (a_ + b_) / 2.0, (b_ + c_) / 2.0
        points = torch.cat((points, ac, ab_, bc))
        a_, b_, c_ = torch.cat((a_, ab_, ab_, ac)), torch.cat((ac, b_, ac, c_)), torch.cat((ab_, bc, bc, bc))
    cell = ((points + 0.5) * (dim - 1)).long()
    grid = torch.zeros((dim, dim, dim), device=verts.device)
    grid[cell[:, 0], cell[:, 1], cell[:, 2]] = 1
    # depth maps: a host loop over the occupied voxels
    g = grid.cpu().numpy()
    last, first = np.full((3, dim, dim), -1), np.full((3, dim, dim), dim)
    for i, j, k in zip(*np.where(g == 1)):
        for axis, (r, s, x) in enumerate(((i, j, k), (i, k, j), (j, k, i))):
            last[axis, r, s] = max(last[axis, r, s], x)
            first[axis, r, s] = min(first[axis, r, s], x)
    # carving: a host loop over the depth-map pixels, then the fill
    kept = np.ones((dim, dim, dim))
    for axis in range(3):
        for r in range(dim):
            for s in range(dim):
                where = (r, s, slice(None)) if axis == 0 else ((r, slice(None), s) if axis == 1 else (slice(None), r, s))
                column = kept[where]
                if last[axis, r, s] < 0:
                    column[:] = 0
                else:
                    column[last[axis, r, s] + 1:] = 0
                    column[:first[axis, r, s]] = 0
    if ndimage is not None:
        kept[ndimage.binary_fill_holes(kept)] = 1
    kept = torch.from_numpy(kept).float().to(verts.device)
    around = torch.nn.functional.conv3d(kept[None, None], torch.ones((1, 1, 3, 3, 3), device=verts.device), padding=1)[0, 0]
    cells = torch.stack(torch.where((around < 27) & (kept != 0))).permute(1, 0).float()
    for axis in range(3):
        cells[:, axis] = cells[:, axis] - (cells[:, axis].max() + cells[:, axis].min()) / 2.0
        extent = cells[:, axis].max() + 1 - cells[:, axis].min()
        cells[:, axis] = cells[:, axis] * (verts[:, axis].max() - verts[:, axis].min()) / extent
    while cells.shape[0] < num_points:
        cells = torch.cat((cells, cells))
    return cells[torch.from_numpy(choices).to(verts.device)]


def workloads():
    v, f = mesh.icosphere(a.level, 0.25)
    rng = np.random.default_rng(0)
    scales = 0.5 + rng.random((a.batch, 1, 3))
    yield f"icosphere-{a.level} ({len(f)} faces), M = 1", [(v, f)]
    yield f"icosphere-{a.level} ({len(f)} faces), M = {a.batch}, the copies scaled per axis by 0.5..1.5", \
        [((v * s).astype(np.float32), f) for s in scales]
    big = np.array([[0, 0, 0], [1, 1, 0.03], [0.02, 1, 1]], dtype=np.float32)
    at = rng.random((20000, 1, 3), dtype=np.float32) * 0.9 + 0.05
    small = (at + rng.random((20000, 3, 3), dtype=np.float32) * (0.5 / a.dim)).reshape(-1, 3)
    yield "one face across the cube + 20000 faces smaller than a voxel, M = 1", \
        [(np.concatenate((big, small)), np.arange(60003, dtype=np.int64).reshape(-1, 3))]


lines = [f"# profiles/points_extract_ab.txt: `python tools/points_bench.py --out profiles/points_extract_ab.txt`, one "
         f"{torch.cuda.get_device_name(0)}",
         f"# dim {a.dim}, {a.num_points} points per cloud; new = extract_points_batch, old = the reference's formulation on torch ops with "
         f"its host loops ({'with' if ndimage is not None else 'WITHOUT'} SciPy's fill), same GPU, alternating; {a.warmup} warm-up, "
         f"{a.rounds} rounds of {a.calls} calls per form; ms",
         "# a recorded number, not a gate: the old form has no kernel of its own, and the parent commit cannot make a cloud at all"]
result = {"device": torch.cuda.get_device_name(0), "dim": a.dim, "num_points": a.num_points, "workloads": {}}
for title, meshes in workloads():
    on_dev = [(torch.from_numpy(np.asarray(v, dtype=np.float32)).to(dev), torch.from_numpy(np.asarray(f, dtype=np.int64)).to(dev))
              for v, f in meshes]
    counts = ops.voxel_surface(*data_making._as_batch(on_dev, dev), a.dim).counts.tolist()
    rng = np.random.default_rng(1)
    choices = []
    for n in counts:
        while n < a.num_points:
            n *= 2
        choices.append(rng.choice(n, a.num_points, replace=False))
    new = lambda: data_making.extract_points_batch(on_dev, a.dim, a.num_points, choices=choices)  # noqa: E731
    old = lambda: [old_form(v, f, a.dim, a.num_points, c) for (v, f), c in zip(on_dev, choices)]  # noqa: E731
    same = all(torch.equal(x, y) for x, y in zip(new(), old()))
    ops.voxel_launches(reset=True)
    new()
    launches = ops.voxel_launches()
    res = ab.alternate({"new": new, "old": old}, a.calls, a.rounds, a.warmup, host_stops="after")
    ab.report(f"{title}: {sum(counts)} surface voxels; clouds identical: {same}; new: {launches['surface']} + {launches['points']} "
              f"operations enqueued per call", res, "new", "old", lines, clock="host")
    result["workloads"][title] = {"surface": counts, "identical": same, "launches": launches, "ms": res}
lines.append(json.dumps(result))
ab.emit(lines, a.out)
