#!/usr/bin/env python
"""Generate ``g24_points.npz``: the REFERENCE's ground-truth point-cloud recipe (``utility/data_making.py::extract_points`` over
``utility/utils.py``'s ``mesh_to_voxel``, ``extract_ODMs``, ``apply_ODMs`` — with its ``binary_fill_holes`` — ``voxel_to_pointcloud``
and ``realign_points``), run on the CPU through ``oracle.ref_shim`` as ``make_golden.py::abc_cloud`` does.

Run in the build container only:  ``python tests/golden/make_golden_points.py``  (a few seconds).  Per case ``<c>`` the file holds the
mesh (``<c>_verts`` fp32, ``<c>_faces`` int32), ``<c>_dim``, and every stage as coordinate lists, not grids:
  ``<c>_occ``      occupied voxels after ``mesh_to_voxel``, int16 (n, 3), sorted lexicographically
  ``<c>_odm``      the six depth maps, int16 (6, dim, dim)
  ``<c>_carved``   the number of voxels ``apply_ODMs`` (with its fill) leaves
  ``<c>_surface``  ``voxel_to_pointcloud`` of the carved grid, int16 (n, 3), in its emission order
  ``<c>_aligned``  ``realign_points`` of them, fp32
  ``<c>_seed``, ``<c>_choices``, ``<c>_cloud``   ``extract_points`` under ``np.random.seed(seed)``: the rows ``np.random.choice``
                   drew from the doubled cloud, and the cloud, fp32 (num_points, 3)
Cases: a seeded random tetrahedron at dim 8 / 16 / 24, the bundled object 1.obj (scaled as ``abc_cloud`` scales 0.obj) at 32 / 128,
two nested icosphere-2 shells (the inner one must vanish) and an open hemisphere (the depth maps see into it through the open
side, so the cloud is the dome alone) at 32.  ``abc`` holds only the mesh of 0.obj: its cloud at 128 is ``g6_chamfer.npz``'s
``abc_cloud``.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from a3vt_amd import mesh as amesh  # noqa: E402
from oracle import mesh as omesh  # noqa: E402
from oracle import ref_shim  # noqa: E402

torch.set_num_threads(8)
ref = ref_shim.load_reference()
assert ref is not None, "needs the reference"
torch.cuda.FloatTensor = torch.FloatTensor
for name in ("pterotactyl.simulator", "pterotactyl.simulator.scene", "pterotactyl.simulator.scene.sampler", "pterotactyl.simulator.physics",
             "pterotactyl.simulator.physics.grasping", "tqdm"):
    if name not in sys.modules:   # data_making.py imports the simulator at its top; extract_points does not use it
        try:
            importlib.import_module(name)
        except Exception:
            ref_shim._stub(name, tqdm=lambda x, **k: x)
ref_making = importlib.import_module("pterotactyl.utility.data_making")


def bundled(name):
    verts, faces = omesh.load_obj(os.path.join(ref.objects_dir, "test_objects", name))
    return ref.utils.scale_points(verts.copy(), 3.1).astype(np.float32), faces


def tetrahedron():
    verts = torch.rand(4, 3, generator=torch.Generator().manual_seed(5)).numpy()
    return verts, np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]])


def shells():
    v, f = amesh.icosphere(level=2, radius=1.0, spatial_order=False)
    return np.concatenate((v, 0.4 * v)).astype(np.float32), np.concatenate((f, f + v.shape[0]))


def hemisphere():
    v, f = amesh.icosphere(level=2, radius=1.0, spatial_order=False)
    return v.astype(np.float32), f[(v[f][:, :, 2] >= -1e-6).all(axis=1)]


def case(out, tag, verts, faces, dim, num_points, seed):
    v, f = torch.FloatTensor(verts), torch.LongTensor(faces)
    voxel = ref.utils.mesh_to_voxel(v, f, dim)
    odms = ref.utils.extract_ODMs(voxel)
    carved = ref.utils.apply_ODMs(odms, dim)
    surface = ref.utils.voxel_to_pointcloud(carved)
    aligned = ref.utils.realign_points(surface.clone(), v.clone())
    n = surface.shape[0]
    while n < num_points:
        n *= 2
    np.random.seed(seed)
    choices = np.random.choice(n, num_points, replace=False)
    np.random.seed(seed)
    cloud = ref_making.extract_points(verts, faces, dim=dim, num_points=num_points)
    out.update({f"{tag}_verts": verts.astype(np.float32), f"{tag}_faces": faces.astype(np.int32), f"{tag}_dim": np.int32(dim),
                f"{tag}_occ": np.argwhere(voxel.numpy() == 1).astype(np.int16), f"{tag}_odm": odms.astype(np.int16),
                f"{tag}_carved": np.int32(carved.sum()), f"{tag}_surface": surface.numpy().astype(np.int16), f"{tag}_aligned": aligned.numpy().astype(np.float32),
                f"{tag}_seed": np.int32(seed), f"{tag}_choices": choices.astype(np.int32), f"{tag}_cloud": cloud.numpy().astype(np.float32)})
    print(f"{tag}: {faces.shape[0]} faces, {int(voxel.sum())} occupied, {int(carved.sum())} carved, {surface.shape[0]} surface")


def main():
    out = {}
    tv, tf = tetrahedron()
    for dim, num in ((8, 700), (16, 300), (24, 1000)):
        case(out, f"tetra{dim}", tv, tf, dim, num, 11 + dim)
    ov, of = bundled("1.obj")
    case(out, "obj1_32", ov, of, 32, 1500, 43)
    case(out, "obj1_128", ov, of, 128, 2000, 44)
    case(out, "shells32", *shells(), 32, 1200, 45)
    case(out, "hemi32", *hemisphere(), 32, 600, 46)
    av, af = bundled("0.obj")
    out.update(abc_verts=av, abc_faces=af.astype(np.int32), abc_dim=np.int32(128))
    path = os.path.join(HERE, "g24_points.npz")
    np.savez_compressed(path, **out)
    print(f"g24_points.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
