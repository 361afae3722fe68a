"""Drop-in for the mesh half of ``pterotactyl/utility/data_making.py``: from object files to the ``_verts.npy`` / ``_faces.npy`` pairs
and the ground-truth clouds ``point_cloud_info/<obj>.npy`` that every loader of ``data_loaders.py`` asks for.

Reference symbols mirrored: ``extract_points`` :50-72, ``save_object_info`` :76-95 (without the URDF), ``save_point_info`` :99-118.
``make_data_split`` and ``save_simulation`` are not here.  This package's own: ``extract_points_batch``, one pass of the kernels
over many meshes.

The cloud of a mesh is the reference's, row for row: voxelise by adaptive subdivision, carve with the six depth maps, take the
surface voxels, realign them to the mesh (``a3vt_voxel_surface`` / ``a3vt_voxel_points``, csrc/voxel.hip, for GPU tensors; the
same contract on NumPy for CPU tensors), double the cloud until it has ``num_points`` rows and draw ``num_points`` of them with
``np.random.choice(n, num_points, replace=False)`` — the reference's own call, so a seeded NumPy gives the reference's cloud.
"""
import os
from glob import glob

import numpy as np
import torch

from ... import ops as _ops
from . import utils


def _as_batch(meshes, device):
    verts = [torch.as_tensor(np.asarray(v, dtype=np.float32) if not isinstance(v, torch.Tensor) else v).detach().to(torch.float32)
             .reshape(-1, 3) for v, _ in meshes]
    faces = [torch.as_tensor(np.asarray(f) if not isinstance(f, torch.Tensor) else f).to(torch.int32).reshape(-1, 3) for _, f in meshes]
    if device is None:
        given = [v.device for v, _ in meshes if isinstance(v, torch.Tensor)]
        device = given[0] if given else utils._default_device()
    offsets = lambda ts: torch.tensor(np.concatenate(([0], np.cumsum([t.shape[0] for t in ts]))), dtype=torch.int32)  # noqa: E731
    return (torch.cat(verts).to(device), torch.cat(faces).to(device), offsets(verts).to(device), offsets(faces).to(device))


def extract_points_batch(meshes, dim=128, num_points=30000, choices=None, device=None):
    """``extract_points`` of every ``(verts, faces)`` pair of ``meshes`` in one pass of the kernels: a list with a (num_points, 3)
    float32 tensor per mesh, or None where the mesh has no surface (no faces).  Identical to the per-mesh calls made in the same
    order: the rows are drawn mesh after mesh from NumPy's global generator.  ``choices``: a list with one index array per mesh
    (into the doubled cloud), replacing the draw.  Arrays go to ``device`` (default: the GPU when there is one); tensors decide it
    themselves.  The one host read is that of the M surface sizes, which the draw and the output's size depend on."""
    if num_points <= 0:
        raise ValueError(f"a3vt: extract_points num_points={num_points} must be positive")
    if len(meshes) == 0:
        return []
    verts, faces, vert_offset, face_offset = _as_batch(meshes, device)
    state = _ops.voxel_surface(verts, faces, vert_offset, face_offset, dim)
    counts = state.counts.tolist()
    index = np.zeros((len(meshes), num_points), dtype=np.int64)
    for m, n in enumerate(counts):
        if n == 0:
            continue
        while n < num_points:
            n *= 2
        index[m] = np.random.choice(n, num_points, replace=False) if choices is None else np.asarray(choices[m], dtype=np.int64)
    cloud = _ops.voxel_points(state, counts=counts, index=torch.from_numpy(index).to(verts.device))["cloud"]
    return [cloud[m] if n else None for m, n in enumerate(counts)]


def extract_points(verts, faces, dim=128, num_points=30000, choices=None):
    """The ground-truth cloud of a mesh, (num_points, 3) float32 on the mesh's device (arrays: the GPU when there is one).  None for
    a mesh without a surface: without faces the reference loops forever."""
    return extract_points_batch([(verts, faces)], dim, num_points, None if choices is None else [choices])[0]


def save_object_info(obj_dir, destination, scale=3.1):
    """``<destination>/<name>_verts.npy`` / ``_faces.npy`` for every ``<obj_dir>/<name>.obj``, scaled by ``utils.get_obj_data``.
    The reference also writes a URDF for pybullet next to them; the physics simulation is out of this package's scope, so no URDF."""
    os.makedirs(destination, exist_ok=True)
    written = []
    for file in sorted(glob(os.path.join(obj_dir, "*.obj"))):
        name = os.path.splitext(os.path.basename(file))[0]
        verts, faces = utils.get_obj_data(file, scale=scale)
        np.save(os.path.join(destination, f"{name}_verts.npy"), verts)
        np.save(os.path.join(destination, f"{name}_faces.npy"), faces)
        written.append(name)
    return written


def save_point_info(object_dir, point_dir, batch=16, dim=128, num_points=30000, device=None):
    """``<point_dir>/<obj>.npy`` — what the loaders read as ``point_cloud_info/<obj>.npy`` — for every ``<obj>_verts.npy`` /
    ``<obj>_faces.npy`` pair of ``object_dir``, ``batch`` meshes per pass of the kernels, in sorted order of the names.  Objects
    without a surface are skipped, as in the reference.  Returns the names written."""
    os.makedirs(point_dir, exist_ok=True)
    names = sorted(os.path.basename(f)[:-len("_verts.npy")] for f in glob(os.path.join(object_dir, "*_verts.npy"))
                   if os.path.exists(f[:-len("_verts.npy")] + "_faces.npy"))
    written = []
    for at in range(0, len(names), max(int(batch), 1)):
        group = names[at:at + max(int(batch), 1)]
        meshes = [(np.load(os.path.join(object_dir, f"{n}_verts.npy")), np.load(os.path.join(object_dir, f"{n}_faces.npy"))) for n in group]
        for name, cloud in zip(group, extract_points_batch(meshes, dim, num_points, device=device)):
            if cloud is not None:
                np.save(os.path.join(point_dir, f"{name}.npy"), cloud.cpu().numpy())
                written.append(name)
    return written
