"""Drop-in for the hot-path part of ``pterotactyl/utility/utils.py`` (same names, argument meaning, return types).

Reference symbols mirrored (file:line under the reference tree):
``load_mesh_vision`` :30-36, ``set_seeds`` :39-43, ``normalize_adj`` :47-52, ``adj_init`` :56-71,
``adj_fuse_touch`` :75-130, ``calc_adj`` :134-148, ``batch_sample`` :152-187, ``load_mesh_touch`` :194-200,
``chamfer_distance`` :204-217, ``save_config`` :535-544, ``load_model_config`` :547-553; and, for ``utility/data_making.py``,
``save_points`` :220, ``extract_surface`` :228, ``write_obj`` :241, ``scale_points`` :348, ``get_obj_data`` :374, ``mesh_to_voxel``
:382, ``voxel_to_pointcloud`` :453, ``extract_ODMs`` :471, ``apply_ODMs`` :502, ``realign_points`` :523; and, for looking at
results, ``get_circle`` :257, ``euler2matrix`` :330, ``add_faces`` :338, ``visualize_actions`` :563, ``visualize_prediction`` :657
(rendered by ``utility/pretty_render.py`` with this library's own ray caster: NOT pyrender's shader, see there).

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
import math
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


# ---- looking at results (reference :257-285, :330-345, :563-668; the renderer itself is utility/pretty_render.py) ----
class get_circle(object):
    """The sphere of actions (reference :257-285): ``points`` (num_points, 3) float32 unit vectors in rings of equal area,
    ``sphere_points`` their [theta, phi].  Where the rings do not add up to ``num_points`` the reference prints and calls ``exit()``;
    this raises ``ValueError`` with the same figures."""

    def __init__(self, num_points, rank=0):
        action_position = []
        a = 4 * np.pi / float(num_points)
        d = math.sqrt(a)
        M_t = round(np.pi / d)
        d_t = np.pi / M_t
        d_phi = a / d_t
        sphere_positions = []
        for i in range(0, M_t):
            theta = np.pi * (i + 0.5) / M_t
            M_phi = round(2 * np.pi * math.sin(theta) / d_phi)
            for j in range(0, M_phi):
                phi = 2 * np.pi * j / M_phi
                sphere_positions.append([theta, phi])
                action_position.append(self.get_point(theta, phi))
        if num_points != len(action_position):
            raise ValueError(f"a3vt: get_circle: we have {len(action_position)} points but want {num_points}")
        self.points = torch.stack(action_position)
        self.sphere_points = sphere_positions

    def get_point(self, a, b):
        return torch.FloatTensor([math.sin(a) * math.cos(b), math.sin(a) * math.sin(b), math.cos(a)])


def euler_matrix(angles, xyz="xyz", degrees=False):
    """SciPy's ``Rotation.from_euler(xyz, angles, degrees).as_matrix()`` for lower-case axis strings, which is all the reference
    passes: extrinsic rotations, applied in the order written about the fixed axes."""
    if len(xyz) != len(angles) or set(xyz) - set("xyz"):
        raise ValueError(f"a3vt: euler_matrix: axes {xyz!r} for {len(angles)} angles (lower-case x, y, z: extrinsic rotations)")
    out = np.eye(3)
    for axis, angle in zip(xyz, np.radians(angles) if degrees else angles):
        c, s = math.cos(angle), math.sin(angle)
        r = {"x": [[1, 0, 0], [0, c, -s], [0, s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]], "z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]
        out = np.array(r, np.float64) @ out
    return out


def euler2matrix(angles=[0, 0, 0], translation=[0, 0, 0], xyz="xyz", degrees=False):
    """A 4 x 4 pose from Euler angles and a translation (reference :330-335)."""
    pose = np.eye(4)
    pose[:3, 3] = translation
    pose[:3, :3] = euler_matrix(angles, xyz, degrees)
    return pose


def add_faces(faces):
    """The faces, then (a, c, b) and (c, b, a) of each (reference :338-345): every triangle three times, once per winding and once
    more, which is how the reference makes its meshes two-sided for pyrender."""
    faces = np.asarray(faces)
    f1, f2, f3 = (np.array(faces[:, k]).reshape(-1, 1) for k in range(3))
    return np.concatenate((faces, np.concatenate((f1, f3, f2), axis=-1), np.concatenate((f3, f2, f1), axis=-1)), axis=0)


# ---- the grasp's vector helpers (reference :289-327), used by simulator/physics/grasping.py ----
def normalize_vector(vector):
    """A (1, 1, 3) array divided by its norm, in place (reference :297-302)."""
    n = np.linalg.norm(vector, axis=2)
    for k in range(3):
        vector[:, :, k] /= n
    return vector


def normal_from_triangle(a, b, c):
    """The unit normal (b - a) x (c - a) of a triangle (reference :289-294)."""
    return normalize_vector(np.cross(b - a, c - a).reshape(1, 1, 3)).reshape(3)


def quats_from_vectors(vec1, vec2):
    """The quaternion (x, y, z, w) of the rotation that turns ``vec1`` onto ``vec2`` about their common normal (reference
    :305-320): I + K + K K (1 - c) / s^2 with K the cross-product matrix of a x b; s = 0 (parallel vectors) is replaced by 1, so
    opposite vectors give what the reference gives, a reflection that SciPy then projects onto a rotation."""
    from scipy.spatial.transform import Rotation
    a, b = np.array(vec1, np.float64), np.array(vec2, np.float64)
    a, b = (a / np.linalg.norm(a)).reshape(3), (b / np.linalg.norm(b)).reshape(3)
    v = np.cross(a, b)
    c, s = np.dot(a, b), np.linalg.norm(v)
    if s == 0:
        s = 1
    kmat = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return Rotation.from_matrix(np.eye(3) + kmat + kmat.dot(kmat) * ((1 - c) / (s ** 2))).as_quat()


def combine_quats(q1, q2):
    """The quaternion of R(q1) R(q2) (reference :323-327)."""
    from scipy.spatial.transform import Rotation
    return Rotation.from_matrix(np.matmul(Rotation.from_quat(q1).as_matrix(), Rotation.from_quat(q2).as_matrix())).as_quat()


def _sphere_cell(point, num_actions):
    """The (row, column) of a unit vector on ``visualize_actions``' (2 num_actions, 4 num_actions) map (reference :573-579)."""
    x, y, z = (float(v) for v in point)
    x = math.atan2(-x, y)
    x = (x + np.pi / 2.0) / (np.pi * 2.0) + np.pi * (28.670 / 360.0)
    y = math.acos(z) / np.pi
    return int(y * num_actions * 12 / (2 * np.pi)), int(x * num_actions * 24 / (2 * np.pi))


def _seen_points(args):
    """The points vision sees, for ``visualize_actions`` with ``use_img``: ``args.visible_points``, an ``.obj`` or ``.npy``.  (The
    reference reads ``objects/visible.obj`` of its own package, which this one does not carry.)"""
    path = getattr(args, "visible_points", None)
    if not path or not os.path.exists(path):
        raise FileNotFoundError(f"a3vt: visualize_actions with use_img needs args.visible_points, the path of an .obj or .npy holding the "
                                f"points vision sees (the reference's pterotactyl/objects/visible.obj); got {path!r}")
    points = np.load(path) if path.endswith(".npy") else _mesh.load_obj(path)[0]
    return np.asarray(points, np.float64).reshape(-1, 3)


def sphere_projection(actions, args):
    """``visualize_actions``' map (reference :571-648) as a (2 num_actions, 4 num_actions, 3) uint8 array: every action's cell, its
    count on top, scaled to 255; with ``args.use_img`` the region vision sees in orange where nothing was marked, and the share of
    the policy's actions inside it printed; the rest teal."""
    n = args.num_actions
    actions = (actions.detach().reshape(-1).long().cpu().numpy() if isinstance(actions, torch.Tensor)
               else np.asarray(actions).reshape(-1).astype(np.int64))
    points = get_circle(n).points.numpy()
    cells = [_sphere_cell(p, n) for p in points]
    array = np.zeros([n * 2, n * 4, 3])
    for x_co, y_co in cells + [cells[a] for a in actions]:
        for i in range(3):
            for j in range(3):
                array[x_co - 1 + i, y_co - 1 + j] += 1.0
    array = array * 255.0 / array.max()
    if args.use_img:
        seen = _seen_points(args)
        seen = seen / np.sqrt((seen ** 2).sum(axis=1)).reshape(-1, 1)
        seen_cells = [_sphere_cell(p, n) for p in seen]
        for x_co, y_co in seen_cells:
            for i in range(5):
                for j in range(5):
                    if array[x_co - 2 + i, y_co - 2 + j].sum() == 0:
                        array[x_co - 2 + i, y_co - 2 + j] = (255, 127, 80)
        array[np.all(array == (0, 0, 0), axis=-1)] = (0, 204, 204)
        check_array = np.zeros([n * 2, n * 4])
        for x_co, y_co in seen_cells:
            for i in range(3):
                for j in range(3):
                    check_array[x_co - 1 + i, y_co - 1 + j] = 100
        on = sum(1.0 for a in actions if check_array[cells[a]] > 0)
        print(f"percentage in vision is {on * 100 / len(actions):.2f} % for policy")
    else:
        array[np.all(array == (0, 0, 0), axis=-1)] = (0, 204, 204)
    return array.astype(np.uint8)


def visualize_actions(location, actions, args):
    """``<location>/histogram.png`` (matplotlib) and ``<location>/sphere_projection.png`` of the actions a policy took (reference
    :563-649), on the host."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from PIL import Image
    flat = actions.detach().reshape(-1).long().cpu().numpy() if isinstance(actions, torch.Tensor) else np.asarray(actions).reshape(-1)
    plt.hist(flat, bins=np.arange(0, args.num_actions + 1))
    plt.title("actions histogram")
    plt.savefig(location + "/histogram.png")
    plt.close()
    Image.fromarray(sphere_projection(actions, args)).save(location + "/sphere_projection.png")


def visualize_prediction(location, meshes, faces, names):
    """``mesh.png``, ``points.png`` and ``ground_truth.png`` of every predicted mesh under ``<location>/<name's last part>/``
    (reference :657-668), all of them rendered by one library call (``pretty_render.render_representations``)."""
    from . import pretty_render
    meshes = meshes.detach().cpu().numpy() if isinstance(meshes, torch.Tensor) else np.asarray(meshes)
    faces = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
    locations = []
    for n in names:
        locations.append(location + "/" + n.split("/")[-1] + "/")
        os.makedirs(locations[-1], exist_ok=True)
    pretty_render.render_representations(locations, names, meshes, faces)
