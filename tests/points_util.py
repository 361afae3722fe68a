"""Shared by the point-cloud tests: the fixture ``g24_points.npz`` case by case, and the meshes no fixture covers."""
import functools

import numpy as np

from golden_util import load

CASES = ("tetra8", "tetra16", "tetra24", "obj1_32", "obj1_128", "shells32", "hemi32")
STAGES = ("occ", "odm", "surface", "aligned")


@functools.lru_cache(maxsize=None)
def fixture():
    z = load("g24_points.npz")
    return {k: z[k] for k in z.files}


def case(tag):
    """dict(verts, faces, dim, occ, odm, carved, surface, aligned, seed, choices, cloud) of one fixture case (read-only)."""
    z = fixture()
    return {k[len(tag) + 1:]: (int(v) if v.ndim == 0 else v) for k, v in z.items() if k.startswith(tag + "_")}


def abc():
    """The bundled object 0.obj as the fixture stores it, and its realigned cloud at dim 128 (``g6_chamfer.npz``)."""
    return dict(case("abc"), aligned=load("g6_chamfer.npz")["abc_cloud"])


def cells_of(grid):
    """Sorted occupied coordinates of a grid (any array type numpy understands)."""
    return np.argwhere(np.asarray(grid) != 0)


def special_meshes():
    """Meshes without a reference fixture -> {name: (verts, faces, dim)}: checked against ``points_ref``."""
    rng = np.random.default_rng(7)
    out = {}
    # one face across the whole cube (the deepest walk) and 200 faces smaller than a voxel (depth 0), dim 64
    big = np.array([[0, 0, 0], [1, 1, 0.03], [0.02, 1, 1]], dtype=np.float32)
    at = rng.random((200, 1, 3), dtype=np.float32) * 0.9 + 0.05
    small = (at + rng.random((200, 3, 3), dtype=np.float32) * 0.004).reshape(-1, 3)
    faces = np.arange(603, dtype=np.int32).reshape(-1, 3)
    out["wide"] = (np.concatenate((big, small)), faces, 64)
    # zero-area (collinear), repeated-vertex and out-of-range faces among ordinary ones, dim 20
    v = rng.random((9, 3), dtype=np.float32)
    v[4] = (v[3] + v[5]) / 2
    out["degenerate"] = (v, np.array([[0, 1, 2], [3, 4, 5], [6, 6, 7], [8, 8, 8], [2, 7, 8], [1, 2, 9], [-1, 0, 3]], dtype=np.int32), 20)
    out["single"] = (rng.random((3, 3), dtype=np.float32), np.array([[2, 0, 1]], dtype=np.int32), 33)
    # a NaN and an infinity in rows no face uses; a face that does use one marks nothing
    v = rng.random((8, 3), dtype=np.float32)
    v[6, 1], v[7, 0] = np.nan, np.inf
    out["nan"] = (v, np.array([[0, 1, 2], [2, 3, 4], [0, 4, 5], [1, 3, 5], [0, 6, 1]], dtype=np.int32), 17)
    return out
