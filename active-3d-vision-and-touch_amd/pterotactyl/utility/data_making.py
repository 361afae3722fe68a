"""Drop-in for the mesh half of ``pterotactyl/utility/data_making.py``: from object files to the ``_verts.npy`` / ``_faces.npy`` pairs
and the ground-truth clouds ``point_cloud_info/<obj>.npy`` that every loader of ``data_loaders.py`` asks for.

Reference symbols mirrored: ``make_data_split`` :22-46, ``extract_points`` :50-72, ``save_object_info`` :76-95 (without the URDF),
``save_point_info`` :99-118, and of ``save_simulation`` :122-209 what follows the grasp: ``save_image_info`` (the vision image,
:157-166) and ``save_touch_signals`` (the touch records, :186-199).  Bullet's grasp physics is not here: for those two the finger
frames ``<action>/<finger>_ref_frame.npy`` are an input, and ``save_simulation`` writes them with a KINEMATIC grasp
(``simulator/physics/grasping.py``: not pybullet, never compared with pybullet's frames) before it calls them.  This package's own: ``extract_points_batch``, one pass of the kernels over many
meshes; ``touch_charts_batch`` / ``save_touch_info``, which write ``touch_charts/<obj>/touch_charts.npy`` from an object's finger
frames (the reference has no writer for that file: it comes with its download).

The chain from object files to a tree that ``data_loaders.py``'s three loaders and the trainers read: ``save_object_info`` ->
``save_point_info`` -> ``save_image_info`` -> frames from a simulator -> ``save_touch_signals`` -> ``save_touch_info`` ->
``make_data_split``; ``save_simulation`` is the three middle steps with the kinematic grasp as the simulator.

The cloud of a mesh is the reference's, row for row: voxelise by adaptive subdivision, carve with the six depth maps, take the
surface voxels, realign them to the mesh (``a3vt_voxel_surface`` / ``a3vt_voxel_points``, csrc/voxel.hip, for GPU tensors; the
same contract on NumPy for CPU tensors), double the cloud until it has ``num_points`` rows and draw ``num_points`` of them with
``np.random.choice(n, num_points, replace=False)`` — the reference's own call, so a seeded NumPy gives the reference's cloud.
"""
import os
import random
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


def _save_atomic(directory, name, array):
    """``<directory>/<name>`` under a temporary name in the same directory, then renamed: no reader ever sees half a file."""
    temporary = os.path.join(directory, f".{name}.{os.getpid()}.tmp")
    try:
        with open(temporary, "wb") as f:
            np.save(f, array)
        os.replace(temporary, os.path.join(directory, name))
    finally:
        if os.path.exists(temporary):
            os.remove(temporary)


def _object_ids(data_root):
    return sorted(os.path.basename(f)[:-len("_verts.npy")] for f in glob(os.path.join(data_root, "object_info", "*_verts.npy")))


def save_image_info(data_root, batch=16, overwrite=False, resolution=(256, 256), colour=_ops.VISION_DEFAULTS["colour"], device=None,
                    sampler=None):
    """``<data_root>/images_colourful/<id>.npy`` — the (height, width, 3) uint8 image ``mesh_loader_vision`` / ``_active`` read and
    whose presence all three loaders take as "this object exists" — for every ``_verts.npy`` / ``_faces.npy`` pair of
    ``<data_root>/object_info/``, in sorted order of the ids, ``batch`` objects per ``ops.scene_render`` call (at most 128: that
    call's images per launch) and one host read per batch.  The image is ``RenderedSampler``'s ``"vision"``: the object alone under
    the reference's vision scene (``ops.VISION_DEFAULTS``), with ``scene_render``'s Lambert shading, NOT pyrender's — a model
    trained on the reference's images has not been evaluated on these.  ``sampler``: an object with ``load_objects`` and
    ``vision_images`` in place of the ``RenderedSampler`` made here.  Existing files are kept unless ``overwrite``; each file is
    written under a temporary name and renamed.

    Returns the counts ``written``, ``skipped_existing`` and ``skipped_no_surface`` (objects without faces)."""
    from ..policies import rendered
    batch = max(int(batch), 1)
    if batch > 128:
        raise ValueError(f"a3vt: save_image_info batch={batch} is more than the 128 images of one scene_render launch")
    object_dir, image_dir = os.path.join(data_root, "object_info"), os.path.join(data_root, "images_colourful")
    counts = dict(written=0, skipped_existing=0, skipped_no_surface=0)
    todo = []
    for obj in _object_ids(data_root):
        faces = os.path.join(object_dir, f"{obj}_faces.npy")
        if not os.path.exists(faces):
            continue
        if np.load(faces, mmap_mode="r").size == 0:
            counts["skipped_no_surface"] += 1
        elif not overwrite and os.path.exists(os.path.join(image_dir, f"{obj}.npy")):
            counts["skipped_existing"] += 1
        else:
            todo.append(obj)
    if not todo:
        return counts
    os.makedirs(image_dir, exist_ok=True)
    if sampler is None:
        sampler = rendered.RenderedSampler({}, to_host=True, resolution=list(resolution), object_colours=colour,
                                           device=utils._device() if device is None else torch.device(device))
    for at in range(0, len(todo), batch):
        group = todo[at:at + batch]
        sampler.load_objects([os.path.join(object_dir, obj) for obj in group])
        for obj, image in zip(group, sampler.vision_images()):
            _save_atomic(image_dir, f"{obj}.npy", np.ascontiguousarray(image, dtype=np.uint8))
            counts["written"] += 1
    return counts


# Whether save_touch_signals reads the batch's clouds and images back packed (ops.touch_pack) when the caller does not say: the
# rule and the measurement of rendered.PACK_POINTS_DEFAULT (profiles/touch_signals_ab.txt), which is not met.  (The same file has
# the bake itself at 8 objects: 68 ms packed against 303 ms padded before the file writes, 291 against 540 with them.)
BAKE_PACK_POINTS = False
BAKING_MARKER = ".baking"


def _touch_records(sampler, names, num_actions, pack_points):
    """One batch of ``save_touch_signals`` -> ``(codes (E, A, 4) int array, {(e, a, finger): (image uint8 (121, 121, 3), points
    float32 (n, 3))})`` for the views whose code is 2.  Packed: one table call and two host reads — the codes with the offsets,
    then ONE buffer holding the clouds' rows and the "touch" views' uint8 images.  Otherwise the calls the package had before
    ``ops.touch_pack``: the float table, truncated here, and ``sample_many`` with the padded points buffer."""
    sampler.load_objects(names)
    E, A, F = len(names), num_actions, 4
    if not pack_points:
        table = sampler.sample_table(A, fingers=None, to_host=True)
        codes = table["touch_code"].numpy()
        images = table["touch_signal"].numpy().astype(np.uint8)
        clouds = sampler.sample_many([[a] * E for a in range(A)], touch=True, touch_point_cloud=True, pack_points=False)
        return codes, {(e, a, j): (images[e, a, j], np.asarray(torch.as_tensor(clouds[a]["touch_point_cloud"][e][j]).cpu().numpy(), np.float32))
                       for e, a, j in zip(*np.nonzero(codes == 2))}
    table = sampler.sample_table(A, fingers=None, to_host=False, touch_point_cloud=True, as_uint8=True)
    n = E * A * F
    small = torch.cat((table["touch_code"].reshape(-1).to(torch.int32), table["cloud_offsets"].to(torch.int32))).cpu().numpy()   # read 1
    codes, offsets = small[:n].reshape(E, A, F), small[n:]
    views = np.flatnonzero(small[:n] == 2)
    total = int(offsets[-1])
    pick = torch.from_numpy(views).to(table["touch_u8"].device)
    payload = torch.cat((table["cloud"][:total].reshape(-1).view(torch.uint8),
                         table["touch_u8"].reshape(n, -1)[pick].reshape(-1))).cpu().numpy()                                       # read 2
    cloud = payload[:total * 12].view(np.float32).reshape(total, 3)
    images = payload[total * 12:].reshape(len(views), 121, 121, 3)
    return codes, {(v // (A * F), v // F % A, v % F): (images[k], cloud[offsets[v]:offsets[v + 1]]) for k, v in enumerate(views)}


def save_touch_signals(data_root, batch=8, num_actions=50, overwrite=False, device=None, sampler=None, pack_points=None, write=True):
    """The touch records of a data set — the part of the reference's ``save_simulation`` that follows the grasp (:186-199): for every
    object of ``<data_root>/object_info/`` with a ``<data_root>/grasp_info/<id>/`` directory, ``<action>/<finger>_touch.npy``
    (121, 121, 3) uint8 and ``<action>/<finger>_points.npy`` (n, 3) for the fingers whose status is "touch", and for no other
    finger — what ``mesh_loader_touch`` reads.  The signals are rendered from the object's triangles and the frames
    ``<action>/<finger>_ref_frame.npy`` (``RenderedSampler``), which are read and never written.  ``batch`` objects per pass, in
    sorted order of the ids: one ``load_objects``, one ``sample_table`` call (two render launches and one ``ops.touch_pack``
    launch) and two host reads.

    Deviation: the points are stored as float32, the renderer's own values.  The reference stores NumPy's float64, and the loader
    converts to float32 at once (``standerdize_point_size``).

    A downloaded data set's files are never silently replaced: without ``overwrite``, an object that already holds any
    ``*_touch.npy`` or ``*_points.npy`` is skipped whole (``skipped_existing``).  While an object's files are being written a
    marker ``grasp_info/<id>/.baking`` exists; it is removed after the last rename.  An object found with the marker counts as not
    yet written: its records are removed and written again.  (So are, under ``overwrite``, those of any object.)  An object
    none of whose fingers touches leaves no file, and a later run renders it again.

    ``sampler``: an object with ``load_objects``, ``sample_table`` and ``sample_many`` in place of the ``RenderedSampler`` made
    here.  ``pack_points`` None: ``BAKE_PACK_POINTS``; the files are the same bytes either way.  ``write=False`` does everything
    but touch the tree (for measuring).

    Returns the counts ``written``, ``skipped_existing``, ``skipped_no_grasps`` (objects) and ``views``, ``touch``, ``no_touch``,
    ``no_intersection`` (the views of the written objects by their status)."""
    from ..policies import recorded, rendered
    batch, num_actions = max(int(batch), 1), int(num_actions)
    if batch * num_actions * recorded.FINGERS > rendered.MAX_VIEWS:
        raise ValueError(f"a3vt: save_touch_signals batch={batch} x num_actions={num_actions} x {recorded.FINGERS} fingers is "
                         f"{batch * num_actions * recorded.FINGERS} views, more than the {rendered.MAX_VIEWS} of one pass")
    object_dir, grasp_dir = os.path.join(data_root, "object_info"), os.path.join(data_root, "grasp_info")
    counts = dict(written=0, skipped_existing=0, skipped_no_grasps=0, views=0, touch=0, no_touch=0, no_intersection=0)
    records = lambda obj: [f for kind in ("touch", "points") for f in glob(os.path.join(grasp_dir, obj, "*", f"*_{kind}.npy"))]  # noqa: E731
    todo = []
    for obj in _object_ids(data_root):
        if not os.path.isdir(os.path.join(grasp_dir, obj)):
            counts["skipped_no_grasps"] += 1
        elif not overwrite and not os.path.exists(os.path.join(grasp_dir, obj, BAKING_MARKER)) and records(obj):
            counts["skipped_existing"] += 1
        else:
            todo.append(obj)
    if not todo:
        return counts
    pack_points = BAKE_PACK_POINTS if pack_points is None else bool(pack_points)
    if sampler is None:                                 # (padded: the sampler copies the buffers whole and slices them on the host)
        sampler = rendered.RenderedSampler(data_root, to_host=not pack_points,
                                           device=utils._device() if device is None else torch.device(device))
    for at in range(0, len(todo), batch):
        group = todo[at:at + batch]
        codes, found = _touch_records(sampler, [os.path.join(object_dir, obj) for obj in group], num_actions, pack_points)
        for e, obj in enumerate(group):
            if write:
                with open(os.path.join(grasp_dir, obj, BAKING_MARKER), "w"):
                    pass
                for stale in records(obj):
                    os.remove(stale)
                for (_, a, j), (image, points) in sorted((kv for kv in found.items() if kv[0][0] == e), key=lambda kv: kv[0]):
                    directory = os.path.join(grasp_dir, obj, str(a))
                    os.makedirs(directory, exist_ok=True)
                    _save_atomic(directory, f"{j}_touch.npy", np.ascontiguousarray(image, dtype=np.uint8))
                    _save_atomic(directory, f"{j}_points.npy", np.ascontiguousarray(points, dtype=np.float32))
                os.remove(os.path.join(grasp_dir, obj, BAKING_MARKER))
            counts["written"] += 1
            counts["views"] += codes[e].size
            for name, value in (("touch", 2), ("no_touch", 1), ("no_intersection", 0)):
                counts[name] += int((codes[e] == value).sum())
    return counts


def save_simulation(data_root, hand, batch=8, num_actions=50, overwrite=False, steps=64, device=None, signals=True, placement=None):
    """The reference's ``save_simulation`` (:122-209) on a tree: the grasp of every action of every object of
    ``<data_root>/object_info/``, then the vision image and the touch records.  **The grasp is ``KinematicGrasp``'s
    (``simulator/physics/grasping.py``): the reference's hand placement, and a kinematic closing rule that is a stand-in for five
    ``stepSimulation`` calls under position control.  No frame of it has been compared with one of pybullet's.**

    Writes ``grasp_info/<id>/<action>/<finger>_ref_frame.npy`` — the reference's pickled ``{"pos": (3,), "rot": (3, 3)}`` float32
    dict, which ``recorded.tree_frames`` reads — one file for every finger of a placed grasp and none for a grasp that could not
    be placed ("no_intersection"; the action's directory is made either way, as the reference makes it).  ``batch`` objects per
    ``KinematicGrasp.grasp_table`` call (one ``ops.grasp_close`` call each), in sorted order of the ids.  ``hand``: a ``HandModel``
    or a path ``HandModel.load`` takes (None: ``PTEROTACTYL_HAND``).  ``placement``: ``KinematicGrasp``'s — "host", "device"
    (``ops.hull_place``: all actions of a batch's objects in one launch) or None for its default.

    Frames are never silently replaced: without ``overwrite`` an object that already holds any ``*_ref_frame.npy`` is skipped
    (``skipped_existing``) unless it carries the marker ``grasp_info/<id>/.baking`` of an interrupted run; such an object's frames,
    and under ``overwrite`` any object's, are removed and written again.  Each file is written under a temporary name and renamed.

    Then, with ``signals``, the existing ``save_image_info`` and ``save_touch_signals`` run on the tree with the same ``batch``
    (capped at ``save_image_info``'s 128), ``overwrite`` and ``device``.  With ``save_object_info``, ``save_point_info``,
    ``save_touch_info`` and ``make_data_split`` a folder of ``.obj`` files is then enough for every file the loaders read.

    Returns the counts ``written``, ``skipped_existing`` (objects), ``grasps``, ``placed`` and, with ``signals``, ``images`` and
    ``touch``: the two calls' own counts."""
    from ..simulator.hand import HandModel
    from ..simulator.physics.grasping import KinematicGrasp
    batch, num_actions = max(int(batch), 1), int(num_actions)
    if not isinstance(hand, HandModel):
        hand = HandModel.load(hand)
    object_dir, grasp_dir = os.path.join(data_root, "object_info"), os.path.join(data_root, "grasp_info")
    counts = dict(written=0, skipped_existing=0, grasps=0, placed=0)
    frames = lambda obj: glob(os.path.join(grasp_dir, obj, "*", "*_ref_frame.npy"))  # noqa: E731
    todo = []
    for obj in _object_ids(data_root):
        if not os.path.exists(os.path.join(object_dir, f"{obj}_faces.npy")):
            continue
        if not overwrite and not os.path.exists(os.path.join(grasp_dir, obj, BAKING_MARKER)) and frames(obj):
            counts["skipped_existing"] += 1
        else:
            todo.append(obj)
    grasper = KinematicGrasp(hand, steps=steps, device=utils._default_device() if device is None else torch.device(device),
                             placement=placement) if todo else None
    for at in range(0, len(todo), batch):
        group = todo[at:at + batch]
        geometry = {obj: (np.load(os.path.join(object_dir, f"{obj}_verts.npy")), np.load(os.path.join(object_dir, f"{obj}_faces.npy")))
                    for obj in group}
        table = grasper.grasp_table(geometry, group, num_actions)
        for e, obj in enumerate(group):
            os.makedirs(os.path.join(grasp_dir, obj), exist_ok=True)
            with open(os.path.join(grasp_dir, obj, BAKING_MARKER), "w"):
                pass
            for stale in frames(obj):
                os.remove(stale)
            for a in range(num_actions):
                directory = os.path.join(grasp_dir, obj, str(a))
                os.makedirs(directory, exist_ok=True)
                for j in np.flatnonzero(table["present"][e, a]):
                    _save_atomic(directory, f"{j}_ref_frame.npy", np.array({"pos": table["pos"][e, a, j].copy(),
                                                                           "rot": table["rot"][e, a, j].copy()}, dtype=object))
                counts["placed"] += int(table["present"][e, a].any())
            os.remove(os.path.join(grasp_dir, obj, BAKING_MARKER))
            counts["written"] += 1
            counts["grasps"] += num_actions
    if signals:
        counts["images"] = save_image_info(data_root, batch=min(batch, 128), overwrite=overwrite, device=device)
        counts["touch"] = save_touch_signals(data_root, batch=batch, num_actions=num_actions, overwrite=overwrite, device=device)
    return counts


SPLIT_SETS = ("recon_train", "auto_train", "RL_train", "valid", "test")
SPLIT_SIZES = (7700, 7700, 7700, 2000, 1000)            # the reference's (:34-38)


def make_data_split(data_root, sizes=None, destination=None):
    """The reference's split rule (:22-46) over a tree's own objects: the ids of ``<data_root>/object_info/*_verts.npy`` (the
    reference takes them from ``initial_objects/*``), sorted as strings, shuffled by ``random.Random(0).shuffle`` and cut
    consecutively into ``recon_train``, ``auto_train``, ``RL_train``, ``valid`` and ``test`` of ``sizes`` objects (None: the
    reference's 7700 / 7700 / 7700 / 2000 / 1000).  A tree with fewer ids than the sizes sum to raises ``ValueError`` — the
    reference's slices would silently come out short or empty.  Writes the dict, pickled, to ``destination`` (None:
    ``<data_root>/data_split.npy``, the file ``data_loaders.load_split`` reads) and returns it."""
    sizes = SPLIT_SIZES if sizes is None else tuple(int(s) for s in sizes)
    if len(sizes) != len(SPLIT_SETS) or min(sizes) < 0:
        raise ValueError(f"a3vt: make_data_split wants {len(SPLIT_SETS)} sizes >= 0 for {SPLIT_SETS}, got {sizes}")
    ids = _object_ids(data_root)
    if len(ids) < sum(sizes):
        raise ValueError(f"a3vt: make_data_split: {data_root!r} holds {len(ids)} objects, fewer than the {sum(sizes)} that the sets "
                         f"{dict(zip(SPLIT_SETS, sizes))} take: pass `sizes` that fit the tree")
    ids.sort()
    random.Random(0).shuffle(ids)
    cuts = np.concatenate(([0], np.cumsum(sizes)))
    split = {name: ids[cuts[k]:cuts[k + 1]] for k, name in enumerate(SPLIT_SETS)}
    destination = os.path.join(data_root, "data_split.npy") if destination is None else destination
    with open(destination, "wb") as f:
        np.save(f, split, allow_pickle=True)
    return split


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
