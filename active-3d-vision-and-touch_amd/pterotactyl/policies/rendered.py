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

Sources:
* frames: a mapping ``{(object_id, action): (pos (4, 3), rot (4, 3, 3), present (4,) bool)}`` or a dataset root holding
  ``grasp_info/<id>/<action>/<finger>_ref_frame.npy`` — read by ``recorded.tree_frames``, with ``recorded.py``'s id convention (the
  basename of the ``names`` entry).  A finger without a frame, and every finger of an unknown ``(id, action)``, is
  "no_intersection" and all zeros, like a grasp that failed (``sampler.py:115-121``);
* geometry: ``<name>_verts.npy`` / ``<name>_faces.npy`` next to the ``names`` entries (``sampler.py:69-70``), or a mapping
  ``{object_id: (verts (V, 3), faces (F, 3))}``.  Faces are taken as stored: the caster is two-sided, so the reference's
  ``add_faces`` duplicates are not needed.

``sample_table(num_actions, fingers=None, to_host=None)`` answers for every action of the loaded objects at once, rendering only the
fingers asked for, in one call: the table ``ActiveTouch`` builds once per episode under ``args.touch_table``.

Out of scope: the grasp physics (frames are an input), the TACTO renderer and vision images."""
import os
from collections.abc import Mapping

import numpy as np
import torch

from .recorded import FINGERS, NO_CONTACT, object_id, table_fingers, tree_frames

RES = 121
STATUS = ("no_touch", "touch")          # the library's status codes
MAX_VIEWS = 1 << 16                     # views of one a3vt_touch_render call (csrc/kernels.h's kTouchMaxImages)


class RenderedSampler:
    def __init__(self, frames, geometry=None, bs=None, vision=False, render=None, to_host=True, device=None, max_depth=0.025,
                 yfov=40.0 / 180.0 * np.pi, znear=1e-4, zfar=10.0):
        """``frames`` / ``geometry``: the sources described above (``geometry=None``: the ``.npy`` files beside the names).  ``bs``
        and ``vision`` are accepted for the reference's constructor shape and not needed.  ``render``: a callable with the
        signature and result of ``ops.touch_render`` that replaces it — it then gets CPU tensors unless ``device`` says otherwise
        (tests run this class's host logic so).  ``to_host=True`` returns CPU tensors, as ``ActiveTouch`` expects of a sampler;
        ``to_host=False`` leaves them where the renderer put them."""
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
        self.render = render
        self.device = torch.device("cpu") if device is None else torch.device(device)
        self.ids, self.table = [], None

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

    def frames_of(self, obj, action):
        if isinstance(self.frames, Mapping):
            return self.frames.get((obj, int(action)))
        return tree_frames(str(self.frames), obj, int(action))

    def sample(self, actions, touch=True, touch_point_cloud=False, **unused):
        return self.sample_many([actions], touch=touch, touch_point_cloud=touch_point_cloud)[0]

    def sample_many(self, action_lists, touch=True, touch_point_cloud=False, **unused):
        """``[sample(actions) for actions in action_lists]`` with all K * E * 4 views rendered in ONE call — what a greedy step's
        candidate loop asks for.  Every view is rendered on its own, so the results are those of the single calls bit for bit."""
        K, E = len(action_lists), len(self.ids)
        for actions in action_lists:
            if len(actions) != E:
                raise ValueError(f"RenderedSampler: {len(actions)} actions for {E} loaded objects")
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
            if out is not None:
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

    def sample_table(self, num_actions, fingers=None, to_host=None):
        """What ``sample`` answers for EVERY action of the loaded objects, as one table (``ActiveTouch`` builds its per-episode touch
        table from it): ``touch_signal`` (E, A, Fs, 121, 121, 3), ``touch_code`` (E, A, Fs) int32 (2 = "touch", 1 = "no_touch", 0 =
        "no_intersection"), ``finger_transfrom_pos`` (E, A, Fs, 3) and ``finger_transform_rot_M`` (E, A, Fs, 3, 3).  Entry [e, a, j]
        is bit for bit what ``sample(actions)`` with ``actions[e] = a`` returns for element e and finger ``fingers[j]`` (indices
        into 0..3; None: all four).  Every grasp's frames are read once, and the live views of the fingers asked for — no others —
        are rendered in ONE call, without contact points.  ``to_host`` None: the instance's setting; False leaves the table on the
        renderer's device."""
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
            out = self.render(*self.table, up(mesh_of[index]), up(pos[index]), up(rot[index]), want_touch=True, want_points=False,
                              **self.camera)
        where = torch.device("cpu") if to_host or out is None else out["touch"].device
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
                "finger_transform_rot_M": torch.from_numpy(rot).to(where).reshape(E, A, Fs, 3, 3)}

    def disconnect(self):
        pass
