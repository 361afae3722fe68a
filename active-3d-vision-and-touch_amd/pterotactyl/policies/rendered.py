"""``RenderedSampler``: the sampler interface of ``ActiveTouch`` (``policies/environment.py``) answered by RENDERING the touch
signals on the GPU from the object's triangles and the grasp's finger frames.

Of the reference's simulator (``simulator/scene/sampler.py:62-175``, ``instance.py``) only the grasp physics needs pybullet, and its
result — the finger frame ``{"pos", "rot"}`` — is what the dataset stores per finger and action in ``*_ref_frame.npy``.  Everything
after the frame is arithmetic on the triangles the dataset stores too (``<obj>_verts.npy``, ``<obj>_faces.npy``): the 121 x 121 depth
camera at the finger, the status, ``depth_to_touch`` and ``depth_to_points``.  That is ``ops.touch_render`` (``a3vt_touch_render``,
csrc/touch_render.hip: two launches for any number of views).  Beside ``RecordedSampler`` (``recorded.py``), which replays images,
this class needs no image on disk, serves ``touch_point_cloud=True`` and returns ``depths``.

The result dict has the reference's keys (its spellings included):

    touch_status             E x 4 strings: "touch", "no_touch" or "no_intersection"
    touch_signal             (E, 4, 121, 121, 3) float32, values 0..255
    depths                   (E, 4, 121, 121) float32
    finger_transfrom_pos     (E, 4, 3) float32
    finger_transform_rot_M   (E, 4, 3, 3) float32
    touch_point_cloud        on request: per element four float32 arrays (n, 3), empty (0, 3) for a finger that is not "touch"
    vision                   on request: E arrays (H, W, 3) uint8, the object alone under the reference's vision scene
    vision_occluded          on request (needs ``hand_visual``): E arrays (H, W, 3) uint8, the object with the posed hand in front

Sources:
* frames: a mapping ``{(object_id, action): (pos (4, 3), rot (4, 3, 3), present (4,) bool)}`` or a dataset root holding
  ``grasp_info/<id>/<action>/<finger>_ref_frame.npy`` — read by ``recorded.tree_frames``, with ``recorded.py``'s id convention (the
  basename of the ``names`` entry).  A finger without a frame, and every finger of an unknown ``(id, action)``, is
  "no_intersection" and all zeros, like a grasp that failed (``sampler.py:115-121``);
* geometry: ``<name>_verts.npy`` / ``<name>_faces.npy`` next to the ``names`` entries (``sampler.py:69-70``), or a mapping
  ``{object_id: (verts (V, 3), faces (F, 3))}``.  Faces are taken as stored: the caster is two-sided, so the reference's
  ``add_faces`` duplicates are not needed.

``sample_table(num_actions, fingers=None, to_host=None)`` answers for every action of the loaded objects at once, rendering only the
fingers asked for, in one call: the table ``ActiveTouch`` builds once per episode under ``args.touch_table``.  With
``touch_point_cloud`` or ``as_uint8`` it also carries what a data set stores per view — the uint8 images and the contact clouds packed
end to end (``ops.touch_pack``, one more launch) — which is what ``data_making.save_touch_signals`` writes.

``vision=True`` adds the reference's ``"vision"`` images (``sampler.py:162-173``): all E from one ``ops.scene_render`` call under
``ops.VISION_DEFAULTS`` (``simulator/rendering/vision_renderer.py:35-77``).  THE SHADING IS NOT PYRENDER'S: it is ``scene_render``'s
Lambert model on ray-cast hits at pixel centres, and no image of it has been compared with one of pyrender's.

``vision_occluded=True`` adds the reference's occluded view (``sampler.py:166-173``: the same scene after ``update_hand``): the
object and the 21 nodes of a ``simulator/hand.py::HandVisual`` posed by the grasp's links (``frames.hand_links``), all K * E images of
a ``sample_many`` from ONE ``ops.scene_render_posed`` call (``a3vt_scene_render_posed``, csrc/posed_render.hip), which draws rigid
instances of shared parts without writing the posed triangles out.  Stated deviations: Lambert shading, not pyrender's, and no
image compared with one of pyrender's; the digit is drawn OPAQUE (pyrender blends its alpha of 175; ``object_colours``' alpha is
ignored likewise); faces are taken as stored, no ``add_faces``; the poses are the kinematic grasp's, not Bullet's; the parts sit in the
URDF link frames (the reference's ``getLinkState(...)[:2]`` is the inertial frame: no link of the URDF gives its ``<inertial>`` an
origin, so the two coincide); an UNPLACED grasp shows the object alone (the reference leaves the hand wherever Bullet has it).

Frames are an input here.  ``simulator/physics/grasping.py::GraspFrames`` makes them from the meshes by a KINEMATIC grasp (not
pybullet's dynamics, never compared with pybullet's frames) and is passed as ``frames`` unchanged.  Out of scope: Bullet's grasp
physics and the TACTO renderer."""
import os
from collections.abc import Mapping

import numpy as np
import torch

from .recorded import FINGERS, NO_CONTACT, object_id, table_fingers, tree_frames

RES = 121
PIXELS = RES * RES
STATUS = ("no_touch", "touch")          # the library's status codes
MAX_VIEWS = 1 << 16                     # views of one a3vt_touch_render call (csrc/kernels.h's kTouchMaxImages)
# Whether ``touch_point_cloud=True`` reads the clouds back packed (``ops.touch_pack``: offsets, then the rows that exist) when the
# caller does not say: on only where tools/touch_signals_bench.py measured the packed read's p90 below the padded read's p10 at both
# sizes (profiles/touch_signals_ab.txt).  Measured: 1.49 x at 1 600 views with a fifth of the pixels in contact, no difference at 12
# views or with every pixel in contact — the rule is not met, the packed read is an option.
PACK_POINTS_DEFAULT = False
# Whether ``vision_occluded`` images come from the posed kernel (``ops.scene_render_posed``) or from the materialised form
# (``ops.pose_parts``, then ``ops.scene_render``) when the caller does not say; the bits are the same.  The project's rule for a
# default: True only where tools/occluded_bench.py measured the posed kernel's p90 below the materialised form's p10 at both sizes
# (profiles/occluded_vision_ab.txt).  Measured, host wall: 0.68 ms against 0.78 at I = 3 and 5.07 against 6.60 at I = 150 (1.16 x and
# 1.30 x), p90 below p10 at both, with 66 MiB against 152 MiB of allocator peak at I = 150: the rule is met.
POSED_RENDER_DEFAULT = True


def pack_host(out, want_touch=True, want_points=True, capacity=None):
    """``ops.touch_pack``'s contract on CPU tensors, for a sampler whose ``render`` is a host callable."""
    result = {}
    if want_touch:
        result["touch_u8"] = torch.nan_to_num(out["touch"], nan=0.0).clamp(0, 255).to(torch.uint8)
    if want_points:
        rows = torch.where(out["status"] == 1, out["count"].clamp(0, PIXELS), torch.zeros_like(out["count"])).to(torch.int64)
        result["offsets"] = torch.cat((rows.new_zeros(1), rows.cumsum(0))).to(torch.int32)
        parts = [out["points"][i, :int(n)] for i, n in enumerate(rows)]
        result["cloud"] = torch.cat(parts) if parts else out["points"].new_zeros((0, 3))
    return result


def camera_matrix(orientation):
    """A camera orientation as ``Renderer.update_camera_pose`` takes it (``vision_renderer.py:180-186``): a 3 x 3 matrix, or three
    xyz Euler angles in degrees."""
    from ..utility import utils
    orientation = np.asarray(orientation, np.float64)
    if orientation.shape == (3,):
        return utils.euler_matrix(orientation, "xyz", degrees=True)
    if orientation.shape != (3, 3):
        raise ValueError(f"RenderedSampler: a camera orientation is a 3 x 3 matrix or three Euler angles, got shape {orientation.shape}")
    return orientation


class RenderedSampler:
    def __init__(self, frames, geometry=None, bs=None, vision=False, render=None, to_host=True, device=None, max_depth=0.025,
                 yfov=40.0 / 180.0 * np.pi, znear=1e-4, zfar=10.0, resolution=[256, 256], object_colours=None, render_scene=None,
                 pack=None, pack_points=None, hand_visual=None, render_posed=None):
        """``frames`` / ``geometry``: the sources described above (``geometry=None``: the ``.npy`` files beside the names).  ``bs``
        and ``vision`` are accepted for the reference's constructor shape and not needed.  ``render``: a callable with the
        signature and result of ``ops.touch_render`` that replaces it — it then gets CPU tensors unless ``device`` says otherwise
        (tests run this class's host logic so).  ``to_host=True`` returns CPU tensors, as ``ActiveTouch`` expects of a sampler;
        ``to_host=False`` leaves them where the renderer put them.

        ``resolution`` (width, height) and ``object_colours`` — one RGB(A) colour or one per loaded object, None: the reference's
        (228, 217, 111); alpha is ignored — are the reference's, for ``vision=True``.  ``render_scene`` / ``pack``: callables that
        replace ``ops.scene_render`` / ``ops.touch_pack`` (with a ``render`` given, ``pack`` defaults to ``pack_host``).
        ``pack_points``: whether contact clouds are read back packed; None: ``PACK_POINTS_DEFAULT``.  The results are the same bits.

        ``hand_visual``: a ``simulator/hand.py::HandVisual``, for ``vision_occluded=True``; ``frames`` must then offer
        ``hand_links(object_id, action)`` (``GraspFrames`` does; a data-set tree stores no link poses).  ``render_posed``: a callable
        that replaces ``ops.scene_render_posed``."""
        if not isinstance(frames, Mapping) and not os.path.isdir(os.path.join(str(frames), "grasp_info")):
            raise ValueError(f"RenderedSampler: {frames!r} is neither a mapping of frames nor a directory holding grasp_info/")
        if geometry is not None and not isinstance(geometry, Mapping):
            raise ValueError("RenderedSampler: geometry is a mapping {id: (verts, faces)} or None (read <name>_verts.npy / _faces.npy)")
        self.frames, self.geometry, self.bs, self.to_host = frames, geometry, bs, to_host
        self.camera = dict(max_depth=max_depth, yfov=yfov, znear=znear, zfar=zfar)
        if render is None:
            from ... import ops
            render = ops.touch_render
            device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
            if pack is None:
                pack = ops.touch_pack
        self.render, self.render_scene = render, render_scene
        self.pack = pack_host if pack is None else pack
        self.pack_points = PACK_POINTS_DEFAULT if pack_points is None else bool(pack_points)
        self.device = torch.device("cpu") if device is None else torch.device(device)
        self.resolution, self.object_colours = (int(resolution[0]), int(resolution[1])), object_colours
        self.hand_visual, self.render_posed, self.parts = hand_visual, render_posed, None
        self.ids, self.table, self.face_offset = [], None, [0]

    def load_objects(self, batch, from_dataset=True, scale=3.1):
        """The batch's meshes as ONE table on the renderer's device (``scale`` is accepted and unused: the stored vertices are
        scaled already)."""
        self.ids = [object_id(name) for name in batch]
        verts, faces, offsets, base = [], [], [0], 0
        for name, obj in zip(batch, self.ids):
            if self.geometry is not None:
                if obj not in self.geometry:
                    raise KeyError(f"RenderedSampler: no geometry for object {obj!r}")
                v, f = self.geometry[obj]
            else:
                v, f = np.load(str(name) + "_verts.npy"), np.load(str(name) + "_faces.npy")
            v, f = np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)
            if len(f) and (f.min() < 0 or f.max() >= len(v)):
                raise ValueError(f"RenderedSampler: object {obj!r} has face indices outside its {len(v)} vertices")
            verts.append(v)
            faces.append(f + base)
            base += len(v)
            offsets.append(offsets[-1] + len(f))
        up = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a, dtype)).to(self.device)  # noqa: E731
        self.table = (up(np.concatenate(verts) if verts else np.zeros((0, 3)), np.float32),
                      up(np.concatenate(faces) if faces else np.zeros((0, 3)), np.int32), up(np.array(offsets), np.int32))
        self.face_offset = offsets
        self.parts = None
        if self.hand_visual is not None:                       # the hand's parts, then one part per object: one table for the call
            from ... import ops
            local = [(v, f - b) for v, f, b in zip(verts, faces, np.cumsum([0] + [len(v) for v in verts]))]
            self.parts = ops.PartTable(list(self.hand_visual.parts) + local, device=self.device)

    def frames_of(self, obj, action):
        if isinstance(self.frames, Mapping):
            return self.frames.get((obj, int(action)))
        return tree_frames(str(self.frames), obj, int(action))

    def vision_images(self, parameters=None):
        """The ``"vision"`` entry: the loaded objects, each alone under the reference's vision scene, as E images (H, W, 3) uint8
        from ONE ``ops.scene_render`` call without the primitive image — arrays with ``to_host``, else device tensors.
        ``parameters``: None, or per element None or a ``(position, orientation)`` pair that moves that element's camera
        (``camera_matrix`` states the orientation's forms).  Faces are taken as stored: the caster is two-sided.  Lambert shading,
        not pyrender's."""
        from ... import ops
        D, E = ops.VISION_DEFAULTS, len(self.ids)
        if self.table is None:
            raise RuntimeError("RenderedSampler: load_objects has not been called")
        if parameters is not None and len(parameters) != E:
            raise ValueError(f"RenderedSampler: {len(parameters)} camera parameters for {E} loaded objects")
        if E == 0:
            return []
        cam_pos, cam_rot = self._vision_cameras(parameters)
        per_face = np.repeat(self._object_rgb(), np.diff(self.face_offset), axis=0)
        verts, faces, _ = self.table
        dev = verts.device
        render_scene = ops.scene_render if self.render_scene is None else self.render_scene
        rgb = render_scene(verts, faces, torch.from_numpy(per_face).to(dev), torch.zeros((0, 3), device=dev), torch.zeros(0, device=dev),
                           torch.zeros((0, 3), dtype=torch.uint8, device=dev), list(self.face_offset), [0] * (E + 1), list(range(E)),
                           torch.from_numpy(cam_pos).to(dev), torch.from_numpy(cam_rot).to(dev), yfov=D["yfov"], znear=D["znear"],
                           zfar=D["zfar"], width=self.resolution[0], height=self.resolution[1], lights=D["lights"],
                           ambient=D["ambient"], background=D["background"], want_prim=False)["rgb"]
        return list(rgb.cpu().numpy()) if self.to_host else list(rgb)

    def _vision_cameras(self, parameters):
        """The E elements' vision cameras ``(cam_pos (E, 3), cam_rot (E, 3, 3))`` float32: the reference's, moved per element by
        ``parameters``."""
        from ... import ops
        D, E = ops.VISION_DEFAULTS, len(self.ids)
        cam_pos, cam_rot = np.tile(np.asarray(D["cam_pos"], np.float32), (E, 1)), np.zeros((E, 3, 3), np.float32)
        cam_rot[:] = camera_matrix(D["cam_euler_xyz_deg"])
        for e, pair in enumerate(parameters or ()):
            if pair is not None:
                cam_pos[e], cam_rot[e] = np.asarray(pair[0], np.float32).reshape(3), camera_matrix(pair[1])
        return cam_pos, cam_rot

    def _object_rgb(self):
        """``object_colours`` as (E, 3) uint8, alpha dropped."""
        from ... import ops
        E = len(self.ids)
        colours = np.asarray(ops.VISION_DEFAULTS["colour"] if self.object_colours is None else self.object_colours)
        if colours.ndim == 1:
            colours = np.tile(colours, (E, 1))
        if colours.shape not in ((E, 3), (E, 4)):
            raise ValueError(f"RenderedSampler: object_colours is one RGB(A) colour or one per object ({E}), got shape {colours.shape}")
        return np.ascontiguousarray(colours[:, :3], np.uint8)

    def occluded_instances(self, action_lists, parameters=None):
        """The instance tables of the K * E occluded images, image (k, e) at row k * E + e, as host arrays: ``inst_part``,
        ``inst_pos``, ``inst_rot``, ``inst_rgb``, ``inst_offset`` (K * E + 1,), ``cam_pos``, ``cam_rot``.  Per image: the element's
        object (part ``len(hand_visual.parts) + e``) under the identity in its ``object_colours`` colour, then — unless the grasp
        could not be placed — the hand's 21 nodes in ``HandVisual``'s order, each under its link's pose (the base's for link -1)."""
        hv, E = self.hand_visual, len(self.ids)
        if not hasattr(self.frames, "hand_links"):
            raise ValueError("RenderedSampler: vision_occluded needs the grasp's link poses, and this `frames` source has no "
                             "hand_links(object_id, action) (a data-set tree stores finger frames only): pass a GraspFrames")
        if self.parts is None:
            raise RuntimeError("RenderedSampler: load_objects has not been called")
        if parameters is not None and len(parameters) != E:
            raise ValueError(f"RenderedSampler: {len(parameters)} camera parameters for {E} loaded objects")
        for actions in action_lists:
            if len(actions) != E:
                raise ValueError(f"RenderedSampler: {len(actions)} actions for {E} loaded objects")
        K = len(action_lists)
        colours, (cam_pos, cam_rot) = self._object_rgb(), self._vision_cameras(parameters)
        node_part = np.array([n[0] for n in hv.nodes], np.int32)
        node_link = np.array([n[1] for n in hv.nodes], np.int64)
        node_rgb = np.array([n[2] for n in hv.nodes], np.uint8).reshape(-1, 3)
        part, pos, rot, rgb, offset = [], [], [], [], [0]
        eye = np.eye(3, dtype=np.float32)
        for actions in action_lists:
            for e, (obj, action) in enumerate(zip(self.ids, actions)):
                part.append(np.array([len(hv.parts) + e], np.int32))
                pos.append(np.zeros((1, 3), np.float32))
                rot.append(eye[None])
                rgb.append(colours[e:e + 1])
                links = self.frames.hand_links(obj, int(action))
                if links is not None:
                    base_pos, base_rot, link_pos, link_rot = (np.asarray(a, np.float32) for a in links)
                    if node_link.max(initial=-1) >= len(link_pos):
                        raise ValueError(f"RenderedSampler: hand_visual names link {int(node_link.max())}, the grasp has {len(link_pos)} links")
                    base = (node_link < 0)
                    at = np.where(base, 0, node_link)
                    part.append(node_part)
                    pos.append(np.where(base[:, None], base_pos.reshape(1, 3), link_pos[at]))
                    rot.append(np.where(base[:, None, None], base_rot.reshape(1, 3, 3), link_rot[at]))
                    rgb.append(node_rgb)
                offset.append(offset[-1] + 1 + (len(node_part) if links is not None else 0))
        cat = lambda rows, shape, dtype: np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros(shape), dtype)  # noqa: E731
        return dict(inst_part=cat(part, (0,), np.int32), inst_pos=cat(pos, (0, 3), np.float32), inst_rot=cat(rot, (0, 3, 3), np.float32),
                    inst_rgb=cat(rgb, (0, 3), np.uint8), inst_offset=np.array(offset, np.int32),
                    cam_pos=np.tile(cam_pos, (K, 1)), cam_rot=np.tile(cam_rot, (K, 1, 1)))

    def occluded_images(self, action_lists, parameters=None, posed=None):
        """The ``"vision_occluded"`` entries of K action lists: K lists of E images (H, W, 3) uint8 — arrays with ``to_host``, else
        device tensors —, the object with the posed hand under the reference's vision scene (``occluded_instances`` states what
        is drawn; the module's docstring states the deviations).  All K * E images come from ONE ``ops.scene_render_posed`` call
        without the primitive images; ``posed=False`` (None: ``POSED_RENDER_DEFAULT``) writes the posed triangles out with
        ``ops.pose_parts`` and renders them with ``ops.scene_render`` instead — the same bits.  Every image is rendered on its
        own, so K lists give what K single calls give bit for bit."""
        from ... import ops
        if self.hand_visual is None:
            raise ValueError("RenderedSampler: occluded_images needs a hand_visual")
        K, E, D = len(action_lists), len(self.ids), ops.VISION_DEFAULTS
        t = self.occluded_instances(action_lists, parameters)
        if K * E == 0:
            return [[] for _ in range(K)]
        dev = self.parts.verts.device
        up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
        scene = dict(yfov=D["yfov"], znear=D["znear"], zfar=D["zfar"], width=self.resolution[0], height=self.resolution[1],
                     lights=D["lights"], ambient=D["ambient"], background=D["background"], want_prim=False)
        inst = [up(t[name]) for name in ("inst_part", "inst_pos", "inst_rot", "inst_rgb")]
        if POSED_RENDER_DEFAULT if posed is None else posed:
            render_posed = ops.scene_render_posed if self.render_posed is None else self.render_posed
            rgb = render_posed(self.parts, *inst, t["inst_offset"], up(t["cam_pos"]), up(t["cam_rot"]), **scene)["rgb"]
        else:
            render_scene = ops.scene_render if self.render_scene is None else self.render_scene
            m = ops.pose_parts(self.parts, *inst, inst_offset=t["inst_offset"])
            rgb = render_scene(m["verts"], m["faces"], m["face_rgb"], torch.zeros((0, 3), device=dev), torch.zeros(0, device=dev),
                               torch.zeros((0, 3), dtype=torch.uint8, device=dev), list(m["face_offset"]), [0] * (K * E + 1),
                               list(range(K * E)), up(t["cam_pos"]), up(t["cam_rot"]), **scene)["rgb"]
        images = list(rgb.cpu().numpy()) if self.to_host else list(rgb)
        return [images[k * E:(k + 1) * E] for k in range(K)]

    def sample(self, actions, touch=True, touch_point_cloud=False, vision=False, vision_occluded=False, parameters=None,
               pack_points=None, **unused):
        return self.sample_many([actions], touch=touch, touch_point_cloud=touch_point_cloud, vision=vision,
                                vision_occluded=vision_occluded, parameters=parameters, pack_points=pack_points)[0]

    def sample_many(self, action_lists, touch=True, touch_point_cloud=False, vision=False, vision_occluded=False, parameters=None,
                    pack_points=None, **unused):
        """``[sample(actions) for actions in action_lists]`` with all K * E * 4 views rendered in ONE call — what a greedy step's
        candidate loop asks for.  Every view is rendered on its own, so the results are those of the single calls bit for bit.
        ``vision_occluded`` (with a ``hand_visual``): result k carries ``occluded_images(action_lists)[k]`` under
        ``"vision_occluded"``, all K * E images from one more call.  ``vision``: every result carries the same ``"vision"`` list (``vision_images(parameters)``: the images do not depend on the
        actions, so they are rendered once).  ``pack_points`` (None: the instance's): the clouds reach the host as the offsets
        table, one small read, and the rows that exist; the padded buffer is not copied."""
        if vision_occluded and self.hand_visual is None:
            raise NotImplementedError("RenderedSampler: vision_occluded needs the hand model (the reference's objects/hand meshes "
                                      "posed by the grasp), which this package does not carry")
        K, E = len(action_lists), len(self.ids)
        for actions in action_lists:
            if len(actions) != E:
                raise ValueError(f"RenderedSampler: {len(actions)} actions for {E} loaded objects")
        if vision_occluded:
            occluded = self.occluded_images(action_lists, parameters)
            return [dict(result, vision_occluded=images) for result, images in
                    zip(self.sample_many(action_lists, touch, touch_point_cloud, vision=vision, parameters=parameters,
                                         pack_points=pack_points), occluded)]
        if vision:
            images = self.vision_images(parameters)
            return [dict(result, vision=images) for result in self.sample_many(action_lists, touch, touch_point_cloud,
                                                                               pack_points=pack_points)]
        if not touch:
            return [{} for _ in range(K)]
        if self.table is None:
            raise RuntimeError("RenderedSampler: load_objects has not been called")
        n = K * E * FINGERS
        pos, rot, live = np.zeros((n, 3), np.float32), np.zeros((n, 3, 3), np.float32), np.zeros(n, bool)
        mesh_of = np.tile(np.repeat(np.arange(E, dtype=np.int32), FINGERS), K)
        for k, actions in enumerate(action_lists):
            for e, (obj, action) in enumerate(zip(self.ids, actions)):
                found = self.frames_of(obj, action)
                if found is None:
                    continue
                at = slice((k * E + e) * FINGERS, (k * E + e + 1) * FINGERS)
                p, r, present = found
                present = np.asarray(present, bool).reshape(FINGERS)
                pos[at] = np.asarray(p, np.float32).reshape(FINGERS, 3) * present[:, None]
                rot[at] = np.asarray(r, np.float32).reshape(FINGERS, 3, 3) * present[:, None, None]
                live[at] = present
        index = np.flatnonzero(live)
        out = None
        if len(index):
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)  # noqa: E731
            out = self.render(*self.table, up(mesh_of[index]), up(pos[index]), up(rot[index]), want_touch=True,
                              want_points=touch_point_cloud, **self.camera)
        where = torch.device("cpu") if self.to_host or out is None else out["depth"].device
        index_t = torch.from_numpy(index).to(where)

        def spread(name, shape):
            """A rendered array -> (K, E, 4, *shape) with zeros at the views that were not rendered: one copy."""
            if out is None:
                return torch.zeros((K, E, FINGERS) + shape, device=where)
            got = out[name].to(where)
            if len(index) == n:
                return got.reshape((K, E, FINGERS) + shape)
            full = torch.zeros((n,) + shape, dtype=got.dtype, device=where)
            full[index_t] = got
            return full.reshape((K, E, FINGERS) + shape)

        signal, depths = spread("touch", (RES, RES, 3)), spread("depth", (RES, RES))
        status = np.full(n, -1, np.int64)
        if out is not None:
            status[index] = out["status"].cpu().numpy()
        words = [NO_CONTACT if s < 0 else STATUS[s] for s in status]
        clouds = None
        if touch_point_cloud:
            clouds = [np.zeros((0, 3), np.float32) if self.to_host else torch.zeros((0, 3), device=where) for _ in range(n)]
            if out is not None and (self.pack_points if pack_points is None else pack_points):
                packed = self.pack(out, want_touch=False, want_points=True)
                offsets = packed["offsets"].cpu().numpy()
                rows = packed["cloud"][:int(offsets[-1])].to(where)
                for j, i in enumerate(index):
                    if status[i] == 1:
                        cloud = rows[int(offsets[j]):int(offsets[j + 1])]
                        clouds[i] = cloud.numpy().copy() if self.to_host else cloud
            elif out is not None:
                points, count = out["points"].to(where), out["count"].cpu().numpy()
                for j, i in enumerate(index):
                    if status[i] == 1:
                        cloud = points[j, :int(count[j])]
                        clouds[i] = cloud.numpy().copy() if self.to_host else cloud
        pos_t, rot_t = torch.from_numpy(pos).to(where), torch.from_numpy(rot).to(where)
        results = []
        for k in range(K):
            rows = slice(k * E * FINGERS, (k + 1) * E * FINGERS)
            result = {"touch_status": [words[(k * E + e) * FINGERS:(k * E + e + 1) * FINGERS] for e in range(E)],
                      "touch_signal": signal[k], "depths": depths[k],
                      "finger_transfrom_pos": pos_t[rows].reshape(E, FINGERS, 3), "finger_transform_rot_M": rot_t[rows].reshape(E, FINGERS, 3, 3)}
            if touch_point_cloud:
                result["touch_point_cloud"] = [clouds[(k * E + e) * FINGERS:(k * E + e + 1) * FINGERS] for e in range(E)]
            results.append(result)
        return results

    def sample_table(self, num_actions, fingers=None, to_host=None, touch_point_cloud=False, as_uint8=False):
        """What ``sample`` answers for EVERY action of the loaded objects, as one table (``ActiveTouch`` builds its per-episode touch
        table from it): ``touch_signal`` (E, A, Fs, 121, 121, 3), ``touch_code`` (E, A, Fs) int32 (2 = "touch", 1 = "no_touch", 0 =
        "no_intersection"), ``finger_transfrom_pos`` (E, A, Fs, 3) and ``finger_transform_rot_M`` (E, A, Fs, 3, 3).  Entry [e, a, j]
        is bit for bit what ``sample(actions)`` with ``actions[e] = a`` returns for element e and finger ``fingers[j]`` (indices
        into 0..3; None: all four).  Every grasp's frames are read once, and the live views of the fingers asked for — no others —
        are rendered in ONE call, without contact points.  ``to_host`` None: the instance's setting; False leaves the table on the
        renderer's device.

        With ``touch_point_cloud`` or ``as_uint8`` the render also makes the contact points and ONE ``ops.touch_pack`` launch
        follows it; the table then carries as well ``touch_u8`` (E, A, Fs, 121, 121, 3) uint8 — ``touch_signal`` truncated, as a data
        set stores it —, ``cloud_offsets`` (E * A * Fs + 1,) int32 and ``cloud`` (total, 3) float32: view v = (e * A + a) * Fs + j
        owns the rows ``[cloud_offsets[v], cloud_offsets[v + 1])``, ``sample``'s ``touch_point_cloud`` of that finger bit for bit
        (no rows unless its code is 2).  On the device ``cloud`` keeps its worst-case rows; only the first ``cloud_offsets[-1]``
        are written.  On the host it is cut to them."""
        fingers = table_fingers(fingers)
        E, A, Fs = len(self.ids), int(num_actions), len(fingers)
        if self.table is None:
            raise RuntimeError("RenderedSampler: load_objects has not been called")
        n = E * A * Fs
        if n > MAX_VIEWS:
            raise ValueError(f"RenderedSampler: sample_table of {E} objects x {A} actions x {Fs} fingers is {n} views, more than the "
                             f"{MAX_VIEWS} of one render call")
        to_host = self.to_host if to_host is None else to_host
        pos, rot, live = np.zeros((n, 3), np.float32), np.zeros((n, 3, 3), np.float32), np.zeros(n, bool)
        mesh_of = np.repeat(np.arange(E, dtype=np.int32), A * Fs)
        for e, obj in enumerate(self.ids):
            for a in range(A):
                found = self.frames_of(obj, a)
                if found is None:
                    continue
                at = slice((e * A + a) * Fs, (e * A + a + 1) * Fs)
                p, r, present = found
                present = np.asarray(present, bool).reshape(FINGERS)
                pos[at] = (np.asarray(p, np.float32).reshape(FINGERS, 3) * present[:, None])[fingers]
                rot[at] = (np.asarray(r, np.float32).reshape(FINGERS, 3, 3) * present[:, None, None])[fingers]
                live[at] = present[fingers]
        index = np.flatnonzero(live)
        out = None
        if len(index):
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)  # noqa: E731
            out = self.render(*self.table, up(mesh_of[index]), up(pos[index]), up(rot[index]), want_touch=True,
                              want_points=bool(touch_point_cloud or as_uint8), **self.camera)
        where = torch.device("cpu") if to_host or out is None else out["touch"].device
        extra = {}
        if touch_point_cloud or as_uint8:
            if out is None:
                extra = {"touch_u8": torch.zeros((E, A, Fs, RES, RES, 3), dtype=torch.uint8, device=where),
                         "cloud_offsets": torch.zeros(n + 1, dtype=torch.int32, device=where), "cloud": torch.zeros((0, 3), device=where)}
            else:
                packed = self.pack(out, want_touch=True, want_points=True)
                offsets, small, cloud = packed["offsets"], packed["touch_u8"], packed["cloud"]
                if len(index) != n:                                  # a view that was not rendered owns no rows and a zero image
                    live_before = torch.searchsorted(torch.from_numpy(index).to(offsets.device),
                                                     torch.arange(n + 1, device=offsets.device))
                    offsets = offsets[live_before]
                    small = torch.zeros((n, RES, RES, 3), dtype=torch.uint8, device=small.device)
                    small[torch.from_numpy(index).to(small.device)] = packed["touch_u8"]
                if to_host:
                    offsets = offsets.cpu()
                    cloud = cloud[:int(offsets[-1])].cpu()
                    small = small.cpu()
                extra = {"touch_u8": small.reshape(E, A, Fs, RES, RES, 3), "cloud_offsets": offsets, "cloud": cloud}
        if len(index) == n:
            signal, code = out["touch"].to(where), out["status"].to(where).to(torch.int32) + 1
        else:                                                        # zeros and code 0 at the views that were not rendered
            signal = torch.zeros((n, RES, RES, 3), device=where)
            code = torch.zeros(n, dtype=torch.int32, device=where)
            if out is not None:
                index_t = torch.from_numpy(index).to(where)
                signal[index_t] = out["touch"].to(where)
                code[index_t] = out["status"].to(where).to(torch.int32) + 1  # the library's 0 / 1 -> "no_touch" 1 / "touch" 2
        return {"touch_signal": signal.reshape(E, A, Fs, RES, RES, 3), "touch_code": code.reshape(E, A, Fs),
                "finger_transfrom_pos": torch.from_numpy(pos).to(where).reshape(E, A, Fs, 3),
                "finger_transform_rot_M": torch.from_numpy(rot).to(where).reshape(E, A, Fs, 3, 3), **extra}

    def disconnect(self):
        pass
