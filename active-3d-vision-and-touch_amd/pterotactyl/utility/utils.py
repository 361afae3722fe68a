"""Drop-in for the hot-path part of ``pterotactyl/utility/utils.py`` (same names, argument meaning, return types).

Reference symbols mirrored (file:line under the reference tree):
``load_mesh_vision`` :30-36, ``set_seeds`` :39-43, ``normalize_adj`` :47-52, ``adj_init`` :56-71,
``adj_fuse_touch`` :75-130, ``calc_adj`` :134-148, ``batch_sample`` :152-187, ``load_mesh_touch`` :194-200,
``chamfer_distance`` :204-217, ``save_config`` :535-544, ``load_model_config`` :547-553; and, for ``utility/data_making.py``,
``save_points`` :220, ``extract_surface`` :228, ``write_obj`` :241, ``scale_points`` :348, ``get_obj_data`` :374, ``mesh_to_voxel``
:382, ``voxel_to_pointcloud`` :453, ``extract_ODMs`` :471, ``apply_ODMs`` :502, ``realign_points`` :523.

Differences that callers can see:
* ``adj_info`` is an :class:`AdjInfo` dict.  It still answers ``['origional']``, ``['adj']`` (dense float tensors,
  materialised lazily — the DDQN graph model reads them, ``policies/DDQN/model.py:68``) and ``['faces']``
  (int64), and additionally carries ``['csr']`` / ``['csr_origional']`` device CSR handles that the HIP GCN uses.
* sampling draws come from Philox4x32-10 seeded from torch's global CPU generator (so ``torch.manual_seed``
  still makes a run reproducible) instead of ``torch.multinomial`` / ``torch.rand`` on the device; pass
  ``samples=`` to inject explicit ``(face_idx, u, v)`` draws (parity tests).

This package's own: ``pretrained_root(args)`` (where the reference's pretrained files are: every engine and trainer asks here) and
``SummaryWriter`` (tensorboard's, or a no-op stub where tensorboard is missing).
"""
import json
import os
import random
from collections import namedtuple

import numpy as np
import torch

from ... import mesh as _mesh
from ... import ops as _ops


try:
    from torch.utils.tensorboard import SummaryWriter
except Exception:  # tensorboard is optional
    class SummaryWriter:
        def __init__(self, *a, **k):
            pass

        def add_scalars(self, *a, **k):
            pass


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("a3vt: no ROCm GPU visible — the MI355X path has no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def pretrained_root(args):
    """The directory the reference's ``download_models.sh`` fills: ``args.pretrained_root``, else ``$PTEROTACTYL_PRETRAINED``."""
    root = getattr(args, "pretrained_root", None) or os.environ.get("PTEROTACTYL_PRETRAINED")
    if not root:
        raise FileNotFoundError("a3vt: set args.pretrained_root or PTEROTACTYL_PRETRAINED to the directory the reference's "
                                "download_models.sh fills (pterotactyl/pretrained/)")
    return root


class AdjInfo(dict):
    """adj_info with lazily materialised dense matrices (reference keys: 'origional', 'adj', 'faces')."""

    _LAZY = {"adj": "csr", "origional": "csr_origional"}

    def __missing__(self, key):
        src = self._LAZY.get(key)
        if src is None or not dict.__contains__(self, src):
            raise KeyError(key)
        csr = dict.__getitem__(self, src)
        dense = torch.from_numpy(csr.host.to_dense()).to(csr.device)
        self[key] = dense
        return dense

    def __contains__(self, key):
        return dict.__contains__(self, key) or (key in self._LAZY and dict.__contains__(self, self._LAZY[key]))


def set_seeds(seed):
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)
    random.seed(seed)


def load_mesh_touch(obj):
    """OBJ -> (verts float32 (V,3), faces int64 (F,3)) on the GPU.  ``obj`` may also be one of the packaged
    asset names 'vision_charts' / 'touch_chart'."""
    if obj in ("vision_charts", "touch_chart"):
        v, f = _mesh.load_asset(obj)
    else:
        v, f = _mesh.load_obj(obj)
    dev = _device()
    return torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)


def calc_adj(faces):
    """Dense binary adjacency with self loops (API compatibility; the hot path uses CSR)."""
    f = faces.detach().cpu().numpy()
    n = int(f.max()) + 1
    r, c = _mesh.vision_pairs(f, n)
    adj = torch.zeros((n, n), dtype=torch.float32)
    adj[torch.from_numpy(r), torch.from_numpy(c)] = 1
    return adj.to(faces.device)


def normalize_adj(mx):
    rowsum = mx.sum(1)
    r_inv = (1.0 / rowsum).view(-1)
    r_inv[r_inv != r_inv] = 0.0
    return r_inv[:, None] * mx


def adj_fuse_touch(verts, faces, adj, args):
    """Dense fused adjacency + faces (API compatibility).  ``adj`` is ignored: the pattern is rebuilt from faces."""
    sv, sf = _mesh.load_asset("touch_chart")
    r, c, n, all_faces = _mesh.fused_pairs(verts.detach().cpu().numpy(), faces.detach().cpu().numpy(), sf,
                                           args.num_grasps, args.finger, sv.shape[0])
    out = torch.zeros((n, n), dtype=torch.float32)
    out[torch.from_numpy(r), torch.from_numpy(c)] = 1
    return out.to(verts.device), torch.from_numpy(all_faces).to(verts.device)


def adj_init(verts, faces, args):
    """CSR adjacency info for a template.  verts (V,3) / faces (F,3) tensors on any device."""
    dev = verts.device if verts.is_cuda else _device()
    v = verts.detach().cpu().numpy().astype(np.float32)
    f = faces.detach().cpu().numpy().astype(np.int64)
    nv = int(f.max()) + 1
    info = AdjInfo()
    orig = _mesh.CSRAdjacency.from_pairs(*_mesh.vision_pairs(f, nv), nv)
    info["csr_origional"] = _ops.DeviceCSR(orig, dev)
    if getattr(args, "use_touch", False):
        sv, sf = _mesh.load_asset("touch_chart")
        r, c, n, all_faces = _mesh.fused_pairs(v, f, sf, args.num_grasps, args.finger, sv.shape[0])
        info["csr"] = _ops.DeviceCSR(_mesh.CSRAdjacency.from_pairs(r, c, n), dev)
        f = all_faces
    else:
        info["csr"] = info["csr_origional"]
    info["faces"] = torch.from_numpy(f).to(dev)
    info["faces_i32"] = info["faces"].to(torch.int32).contiguous()
    return info


def load_mesh_vision(args, obj):
    verts, faces = load_mesh_touch(obj)
    return adj_init(verts, faces, args), verts


def _faces_i32(faces):
    return faces if faces.dtype == torch.int32 else faces.to(torch.int32)


def _philox_seed():
    # one draw from torch's global CPU generator: reproducible under torch.manual_seed, no device sync
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def batch_sample(verts, faces, num=10000, draws=None, samples=None):
    """Area-weighted surface samples.  Returns (B,num,3) like the reference, or (draws,B,num,3) when ``draws`` is given."""
    f32 = _faces_i32(faces).contiguous()
    d = 1 if draws is None else draws
    if samples is not None:
        fi, u, v = samples
        pts = _ops.SamplePointsFn.apply(verts, f32, num, d, 0, 0, fi.to(torch.int32), u, v)
    else:
        pts = _ops.SamplePointsFn.apply(verts, f32, num, d, _philox_seed(), 0, None, None, None)
    return pts[0] if draws is None else pts


def chamfer_distance(verts, faces, gt_points, num=1000, repeat=3, samples=None):
    """(B,) Chamfer distance between ``repeat`` surface samplings of the meshes and ``gt_points`` (B,Q,3).
    ``samples``: optional (face_idx, u, v) tensors shaped (repeat,B,num) to inject the draws."""
    pred = batch_sample(verts, faces, num=num, draws=repeat, samples=samples)
    return _ops.ChamferFn.apply(pred, gt_points.contiguous())


def save_config(location, args):
    abs_path = os.path.abspath(location)
    args = vars(args)
    args["check_point"] = abs_path
    config_location = f"{location}/config.json"
    with open(config_location, "w") as fp:
        json.dump(args, fp, indent=4)
    return config_location


def load_model_config(location):
    config_location = f"{location}/config.json"
    with open(config_location) as json_file:
        data = json.load(json_file)
    weight_location = data["check_point"] + "/model"
    args = namedtuple("ObjectName", data.keys())(*data.values())
    return args, weight_location


# ---- meshes to ground-truth point clouds (reference :220-252, :348-379, :382-532; the pipeline itself is utility/data_making.py) ----
def _default_device():
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


def _one_mesh(verts, faces):
    """(verts float32 (V, 3), faces int32 (F, 3), the two offset tensors) of one mesh, on verts' device (arrays: the default one)."""
    if not isinstance(verts, torch.Tensor):
        verts = torch.as_tensor(np.asarray(verts, dtype=np.float32)).to(_default_device())
    faces = torch.as_tensor(np.asarray(faces) if not isinstance(faces, torch.Tensor) else faces)
    verts = verts.detach().to(torch.float32).reshape(-1, 3)
    faces = faces.to(verts.device).to(torch.int32).reshape(-1, 3)
    offsets = lambda n: torch.tensor([0, n], dtype=torch.int32, device=verts.device)  # noqa: E731
    return verts, faces, offsets(verts.shape[0]), offsets(faces.shape[0])


def mesh_to_voxel(verts, faces, resolution):
    """Occupancy grid (resolution,) * 3, float, of a mesh normalised into the unit cube: every vertex of the reference's adaptive
    1 -> 4 subdivision (sides down to 1 / resolution) marks its voxel.  ``a3vt_voxel_surface`` on GPU tensors, its NumPy form on CPU
    tensors: the same grid, and the reference's bit for bit."""
    v, f, vo, fo = _one_mesh(verts, faces)
    return _ops.voxel_surface(v, f, vo, fo, resolution, want_occupancy=True).occupancy[0].float()


def extract_ODMs(voxels):
    """The six orthographic depth maps of a grid (cells equal to 1 are occupied) as a (6, dim, dim) float64 array, the reference's
    values: [0] / [1] distance of the last / first occupied cell of column (i, j) from the far / near end along k, [2] / [3] along j
    for (i, k), [4] / [5] along i for (j, k); dim for an empty column."""
    voxels = torch.as_tensor(voxels)
    return _ops.voxel_depth_maps((voxels == 1).to(torch.uint8)[None]).cpu().numpy()[0].astype(np.float64)


def apply_ODMs(ODMs, dim, device=None):
    """Space carving: the int64 grid of the cells that no depth map removes (on ``device``; the GPU when there is one).  A cell
    survives iff it lies inside its column's [first, last] interval along all three axes, which is the reference's result including
    its ``binary_fill_holes``: whatever is carved is carved through to the border, so there is no hole to fill."""
    odm = torch.as_tensor(np.asarray(ODMs.cpu() if isinstance(ODMs, torch.Tensor) else ODMs)).to(device or _default_device())
    odm = torch.where(odm > 0, odm, torch.zeros_like(odm)).long()
    x = torch.arange(dim, device=odm.device)
    i, j, k = x[:, None, None], x[None, :, None], x[None, None, :]
    kept = (k >= odm[1][:, :, None]) & (k <= dim - 1 - odm[0][:, :, None])
    kept &= (j >= odm[3][:, None, :]) & (j <= dim - 1 - odm[2][:, None, :])
    kept &= (i >= odm[5][None, :, :]) & (i <= dim - 1 - odm[4][None, :, :])
    return kept.long()


def _box_count(voxel):
    """Occupied cells in every cell's 3 x 3 x 3 neighbourhood (cells outside the grid are empty), int32."""
    box = torch.nn.functional.pad((voxel != 0).to(torch.int32), (1, 1, 1, 1, 1, 1))
    for axis in range(3):
        n = box.shape[axis]
        box = box.narrow(axis, 0, n - 2) + box.narrow(axis, 1, n - 2) + box.narrow(axis, 2, n - 2)
    return box


def voxel_to_pointcloud(voxel):
    """The occupied cells with fewer than 27 occupied cells around them, as float (n, 3) indices in lexicographic order."""
    surface = (voxel != 0) & (_box_count(voxel) < 27)
    return torch.stack(torch.where(surface)).permute(1, 0).float()


def extract_surface(voxel):
    """Every cell, occupied or not, with between 1 and 26 occupied cells in its neighbourhood: float (n, 3) indices."""
    count = _box_count(voxel)
    return torch.stack(torch.where((count < 27) & (count > 0))).permute(1, 0).float()


def realign_points(points, verts):
    """Centre a cloud of cell indices per axis and scale it to the extent of ``verts`` on that axis (a new fp32 tensor)."""
    points = points.float().clone()
    for axis in range(3):
        col = points[:, axis]
        col = col - (col.max() + col.min()) / 2.0
        extent = col.max() + 1 - col.min()                      # (of the centred values)
        points[:, axis] = col * (verts[:, axis].max() - verts[:, axis].min()) / extent
    return points


def scale_points(points, scale=1.0):
    """Move a cloud (array or tensor, changed in place as far as the reference changes it) to the positive octant, scale its largest
    coordinate to 1 / scale and centre every axis on half its extent."""
    for axis in range(3):
        points[:, axis] -= points[:, axis].min()
    points = points / points.max() / scale
    for axis in range(3):
        points[:, axis] -= points[:, axis].max() / 2.0
    return points


def write_obj(filename, verts, faces):
    """A Wavefront OBJ of ``verts`` and ``faces`` (written as given: 1-based indices are the caller's business, as in the reference)."""
    with open(filename, "w") as f:
        f.write("g\n# %d vertex\n" % len(verts))
        f.writelines("v %f %f %f\n" % tuple(v) for v in verts)
        f.write("# %d faces\n" % len(faces))
        f.writelines("f %d %d %d\n" % tuple(face) for face in faces)


def save_points(file, points):
    """``<file>.obj`` holding a point cloud (tensor or array) as vertices."""
    write_obj(f"{file}.obj", points.detach().cpu().numpy() if isinstance(points, torch.Tensor) else points, [])


def get_obj_data(obj_location, scale=1.0):
    """(verts float32 scaled by ``scale_points``, faces int64) of an OBJ file, read by this package's own reader (``mesh.load_obj``)."""
    verts, faces = _mesh.load_obj(obj_location)
    return scale_points(verts, scale), faces
