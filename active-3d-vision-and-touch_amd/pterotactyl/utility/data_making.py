"""Drop-in for the mesh half of ``pterotactyl/utility/data_making.py``: from object files to the ``_verts.npy`` / ``_faces.npy`` pairs
and the ground-truth clouds ``point_cloud_info/<obj>.npy`` that every loader of ``data_loaders.py`` asks for.

Reference symbols mirrored: ``extract_points`` :50-72, ``save_object_info`` :76-95 (without the URDF), ``save_point_info`` :99-118.
``make_data_split`` and ``save_simulation`` are not here.  This package's own: ``extract_points_batch``, one pass of the kernels
over many meshes; ``touch_charts_batch`` / ``save_touch_info``, which write ``touch_charts/<obj>/touch_charts.npy`` from an
object's finger frames (the reference has no writer for that file: it comes with its download).

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


# Whether the bake runs the predictor's head as one launch (ops.touch_chart_head) when the caller does not say: the form that
# measured faster in tools/touch_bake_bench.py (profiles/touch_bake_ab.txt).  scoring.FUSED_HEAD_DEFAULT follows its own, stricter rule.
BAKE_FUSED_HEAD = True


def touch_charts_batch(sampler, encoder, template, names, num_actions=50, truncate=True, encode_chunk=None, fused_head=None):
    """The ``touch_charts.npy`` contents of the objects ``names`` -> (E, A, 4, 25, 4) float32 on the encoder's device: per object,
    action and finger 25 rows of x, y, z, mask.

    One ``sampler.load_objects(names)`` and one ``sampler.sample_table(num_actions, fingers=None, to_host=False)`` call (both
    samplers of ``policies/``); always four fingers (``mesh_loader_vision`` takes finger 1 out of the four-finger file).  The
    images stay channels-last: with ``truncate`` they pass through uint8 first (the data set stores ``_touch.npy`` as uint8, and
    the predictor is trained on those), then ``/ 255`` in fp32, then ``encoder.predict_features_nhwc`` under ``no_grad``, in
    chunks of ``encode_chunk`` views (None: all at once); then the head over all E * A * 4 views: ``ops.touch_chart_head`` with
    ``fused_head`` (None: ``BAKE_FUSED_HEAD``; one launch on the GPU), otherwise the torch lines of ``Encoder.forward`` and
    ``scoring.touch_slots``.

    The mask column holds the environment's codes — 2 for "touch" (the predicted chart), 1 for "no_touch" (the finger's
    position 25 times), 0 otherwise (zeros) — because the reference evaluates, on exactly those codes (``policies/environment.py:
    304-353``), the model it trained on the data set's files.  That the downloaded files hold the same codes is an inference from
    that; the files are not on hand to check."""
    dev = next(encoder.parameters()).device
    sampler.load_objects(names)
    table = sampler.sample_table(num_actions, fingers=None, to_host=False)
    signal = table["touch_signal"]
    E, A, F = signal.shape[:3]
    n = E * A * F
    signal = signal.reshape(n, *signal.shape[3:])
    chunk = n if not encode_chunk else max(int(encode_chunk), 1)
    features = []
    with torch.no_grad():
        for at in range(0, n, chunk):
            part = signal[at:at + chunk].to(dev)
            if truncate:
                part = part.to(torch.uint8)
            features.append(encoder.predict_features_nhwc(part.to(torch.float32) / 255.0))
        features = features[0] if len(features) == 1 else torch.cat(features)
        head = (_ops.touch_chart_head if (BAKE_FUSED_HEAD if fused_head is None else fused_head)
                else lambda *a: torch.cat(_ops._chart_head_torch(*a), dim=-1))
        rows = head(features, encoder.fc, torch.as_tensor(template, dtype=torch.float32).to(dev).reshape(25, 3),
                    table["finger_transform_rot_M"].to(dev).float().reshape(n, 3, 3),
                    table["finger_transfrom_pos"].to(dev).float().reshape(n, 3), table["touch_code"].to(dev).reshape(n))
    return rows.reshape(E, A, F, 25, 4)


def _load_touch_encoder(touch_location, device):
    """The touch ``Encoder`` of a checkpoint directory, in ``eval`` mode on ``device``; ``touch_location=None``: the directory
    ``ActiveTouch.pretrained_recon_models`` resolves (``<pretrained root>/reconstruction/touch/best``)."""
    from types import SimpleNamespace

    from ..reconstruction.touch import model as touch_model
    if touch_location is None:
        touch_location = os.path.join(utils.pretrained_root(SimpleNamespace()), "reconstruction", "touch", "best") + "/"
    encoder = touch_model.Encoder().to(device)
    encoder.load_state_dict(torch.load(os.path.join(touch_location, "model"), map_location=device))
    return encoder.eval()


def save_touch_info(data_root, encoder=None, touch_location=None, sampler="rendered", batch=8, num_actions=50, overwrite=False,
                    device=None):
    """``<data_root>/touch_charts/<id>/touch_charts.npy`` — what ``mesh_loader_vision.get_touch_info`` reads, (num_actions, 4, 25, 4)
    float32 (``touch_charts_batch`` states the columns) — for every ``<data_root>/object_info/<id>_verts.npy`` that has a
    ``<data_root>/grasp_info/<id>/`` directory, ``batch`` objects per pass, in sorted order of the ids.  The last step of the
    data generation: ``save_object_info`` -> ``save_point_info`` -> grasps (``<action>/<finger>_ref_frame.npy``, from a simulator)
    -> this.  Nothing in the reference writes the file: there it comes with the downloaded data set.

    ``encoder``: a touch ``Encoder`` (used as it is, on its device); None loads ``touch_location``'s checkpoint, or with that None
    too the pretrained one, by the rule of ``ActiveTouch.pretrained_recon_models``, onto ``device`` (default: the GPU when there
    is one).  ``sampler``: "rendered" (a ``RenderedSampler`` on the tree: the images are rendered from the triangles and the
    frames), "recorded" (a ``RecordedSampler``: the tree's ``<finger>_touch.npy`` are replayed) or a sampler object with
    ``load_objects`` and ``sample_table``.  Existing files are kept unless ``overwrite``.  A file is written under a temporary
    name in its directory and renamed, so an interrupted run leaves no half-written ``touch_charts.npy``.

    Returns the counts ``written``, ``skipped_existing``, ``skipped_no_grasps`` (objects) and ``views``, ``touch``, ``no_touch``,
    ``no_intersection`` (the views of the written files by their code)."""
    from ..policies import recorded, rendered
    batch, num_actions = max(int(batch), 1), int(num_actions)
    if batch * num_actions * recorded.FINGERS > rendered.MAX_VIEWS:
        raise ValueError(f"a3vt: save_touch_info batch={batch} x num_actions={num_actions} x {recorded.FINGERS} fingers is "
                         f"{batch * num_actions * recorded.FINGERS} views, more than the {rendered.MAX_VIEWS} of one pass")
    object_dir = os.path.join(data_root, "object_info")
    counts = dict(written=0, skipped_existing=0, skipped_no_grasps=0, views=0, touch=0, no_touch=0, no_intersection=0)
    todo = []
    for obj in sorted(os.path.basename(f)[:-len("_verts.npy")] for f in glob(os.path.join(object_dir, "*_verts.npy"))):
        if not os.path.isdir(os.path.join(data_root, "grasp_info", obj)):
            counts["skipped_no_grasps"] += 1
        elif not overwrite and os.path.exists(os.path.join(data_root, "touch_charts", obj, "touch_charts.npy")):
            counts["skipped_existing"] += 1
        else:
            todo.append(obj)
    if not todo:
        return counts
    if encoder is None:
        encoder = _load_touch_encoder(touch_location, utils._default_device() if device is None else torch.device(device))
    dev = next(encoder.parameters()).device
    if sampler == "rendered":
        sampler = rendered.RenderedSampler(data_root, to_host=False, device=dev)
    elif sampler == "recorded":
        sampler = recorded.RecordedSampler(data_root)
    elif not callable(getattr(sampler, "sample_table", None)) or not callable(getattr(sampler, "load_objects", None)):
        raise ValueError(f'a3vt: save_touch_info sampler is "rendered", "recorded" or an object with load_objects and sample_table, '
                         f"got {sampler!r}")
    from ... import mesh as _mesh
    template = torch.from_numpy(np.asarray(_mesh.load_asset("touch_chart")[0], dtype=np.float32))
    for at in range(0, len(todo), batch):
        group = todo[at:at + batch]
        rows = touch_charts_batch(sampler, encoder, template, [os.path.join(object_dir, obj) for obj in group], num_actions).cpu().numpy()
        for obj, charts in zip(group, rows):
            directory = os.path.join(data_root, "touch_charts", obj)
            os.makedirs(directory, exist_ok=True)
            temporary = os.path.join(directory, f".touch_charts.{os.getpid()}.tmp")
            try:
                with open(temporary, "wb") as f:
                    np.save(f, np.ascontiguousarray(charts, dtype=np.float32))
                os.replace(temporary, os.path.join(directory, "touch_charts.npy"))
            finally:
                if os.path.exists(temporary):
                    os.remove(temporary)
            code = charts[:, :, 0, 3]
            counts["written"] += 1
            counts["views"] += code.size
            for name, value in (("touch", 2), ("no_touch", 1), ("no_intersection", 0)):
                counts[name] += int((code == value).sum())
    return counts


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
