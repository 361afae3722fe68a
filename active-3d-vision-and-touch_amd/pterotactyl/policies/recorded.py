"""``RecordedSampler``: the sampler interface of ``ActiveTouch`` (``policies/environment.py``) answered from recorded signals.

The reference's environment drives its simulator through two calls, ``sampler.load_objects(names, from_dataset=True)`` and
``sampler.sample(actions, touch_point_cloud=True)`` (``simulator/scene/sampler.py:62-175``).  The simulator needs pybullet and
pyrender; this class replays what it recorded instead, with the same signatures and the same result dict (the reference's key
spellings included):

    touch_status             E x 4 strings: "touch", "no_touch" or "no_intersection"
    touch_signal             (E, 4, 121, 121, 3) float32, values 0..255
    finger_transfrom_pos     (E, 4, 3) float32
    finger_transform_rot_M   (E, 4, 3, 3) float32

Sources:
* a mapping ``{(object_id, action): record}``; a record holds ``touch`` (4, 121, 121, 3), ``pos`` (4, 3), ``rot`` (4, 3, 3) and
  ``status`` (4 strings);
* a dataset root laid out as ``mesh_loader_touch`` reads it: ``grasp_info/<id>/<action>/<finger>_touch.npy`` and
  ``<finger>_ref_frame.npy`` (pickled ``{"rot", "pos"}``).

Conventions of THIS package (the reference never replays, so none of this restates it): in a dataset tree a finger with a touch
image is "touch", a finger with only a frame file is "no_touch", a finger with neither is "no_intersection" and all zeros; the
object id is the basename of the ``names`` entry given to ``load_objects``; an unknown ``(id, action)`` is "no_intersection" for
all four fingers, like a grasp that failed (``sampler.py:115-121``).

``sample_table(num_actions, fingers=None)`` answers for every action of the loaded objects at once — the table ``ActiveTouch`` builds
once per episode under ``args.touch_table`` — with status codes (``STATUS_CODES``) in place of the strings."""
import os
from collections.abc import Mapping

import numpy as np
import torch

FINGERS = 4
NO_CONTACT = "no_intersection"
STATUS_CODES = {"touch": 2, "no_touch": 1}     # ``sample_table``'s ``touch_code`` (``scoring.touch_slots``' codes); anything else is 0


def table_fingers(fingers):
    """The ``fingers`` argument of ``sample_table`` as a list of indices into 0..3 (None: all four).  (Shared with ``rendered.py``.)"""
    fingers = list(range(FINGERS)) if fingers is None else [int(f) for f in fingers]
    if not fingers or any(not 0 <= f < FINGERS for f in fingers):
        raise ValueError(f"sample_table: fingers must be indices into 0..{FINGERS - 1}, got {fingers}")
    return fingers


def object_id(name):
    """The id of a ``names`` entry of ``load_objects``: its basename."""
    return os.path.basename(os.path.normpath(str(name)))


def tree_frames(root, obj, action):
    """The finger frames of one grasp in a dataset tree -> ``(pos (4, 3), rot (4, 3, 3), present (4,) bool)`` float32, zeros for
    a finger without ``<finger>_ref_frame.npy``; None without the grasp's directory.  (Shared with ``rendered.py``.)"""
    d = os.path.join(root, "grasp_info", obj, str(action))
    if not os.path.isdir(d):
        return None
    pos, rot, present = np.zeros((FINGERS, 3), np.float32), np.zeros((FINGERS, 3, 3), np.float32), np.zeros(FINGERS, bool)
    for f in range(FINGERS):
        frame = os.path.join(d, f"{f}_ref_frame.npy")
        if not os.path.exists(frame):
            continue
        ref = np.load(frame, allow_pickle=True).item()
        pos[f], rot[f], present[f] = np.asarray(ref["pos"]).reshape(3), np.asarray(ref["rot"]).reshape(3, 3), True
    return pos, rot, present


def _tree_record(root, obj, action):
    frames = tree_frames(root, obj, action)
    if frames is None:
        return None
    pos, rot, present = frames
    rec = {"touch": np.zeros((FINGERS, 121, 121, 3), np.float32), "pos": pos, "rot": rot, "status": [NO_CONTACT] * FINGERS}
    for f in np.flatnonzero(present):
        touch = os.path.join(root, "grasp_info", obj, str(action), f"{f}_touch.npy")
        if os.path.exists(touch):
            rec["touch"][f] = np.load(touch)
            rec["status"][f] = "touch"
        else:
            rec["status"][f] = "no_touch"
    return rec


class RecordedSampler:
    def __init__(self, source, bs=None, vision=False):
        """``source``: the mapping or the dataset root described above; ``bs`` and ``vision`` are accepted for the reference's
        constructor shape (``Sampler(grasp, bs=, vision=)``) and not needed: the batch is whatever ``load_objects`` was given."""
        if not isinstance(source, Mapping) and not os.path.isdir(os.path.join(str(source), "grasp_info")):
            raise ValueError(f"RecordedSampler: {source!r} is neither a mapping of records nor a directory holding grasp_info/")
        self.source = source
        self.bs = bs
        self.ids = []

    def load_objects(self, batch, from_dataset=True, scale=3.1):
        self.ids = [object_id(name) for name in batch]

    def record(self, obj, action):
        if isinstance(self.source, Mapping):
            return self.source.get((obj, int(action)))
        return _tree_record(str(self.source), obj, int(action))

    def sample(self, actions, touch_point_cloud=False, **unused):
        if len(actions) != len(self.ids):
            raise ValueError(f"RecordedSampler: {len(actions)} actions for {len(self.ids)} loaded objects")
        E = len(self.ids)
        status = [[NO_CONTACT] * FINGERS for _ in range(E)]
        touch = torch.zeros((E, FINGERS, 121, 121, 3))
        pos = torch.zeros((E, FINGERS, 3))
        rot = torch.zeros((E, FINGERS, 3, 3))
        for e, (obj, action) in enumerate(zip(self.ids, actions)):
            rec = self.record(obj, action)
            if rec is None:
                continue
            status[e] = [str(s) for s in rec["status"]]
            touch[e] = torch.as_tensor(np.asarray(rec["touch"]), dtype=torch.float32)
            pos[e] = torch.as_tensor(np.asarray(rec["pos"]), dtype=torch.float32)
            rot[e] = torch.as_tensor(np.asarray(rec["rot"]), dtype=torch.float32)
        return {"touch_status": status, "touch_signal": touch, "finger_transfrom_pos": pos, "finger_transform_rot_M": rot}

    def sample_table(self, num_actions, fingers=None, to_host=None):
        """What ``sample`` answers for EVERY action of the loaded objects, as one table (``ActiveTouch`` builds its per-episode touch
        table from it): ``touch_signal`` (E, A, Fs, 121, 121, 3), ``touch_code`` (E, A, Fs) int32 (``STATUS_CODES``; 0 for anything
        else), ``finger_transfrom_pos`` (E, A, Fs, 3) and ``finger_transform_rot_M`` (E, A, Fs, 3, 3), CPU tensors.  Entry [e, a, j]
        is bit for bit what ``sample(actions)`` with ``actions[e] = a`` returns for element e and finger ``fingers[j]`` (None: all
        four); zeros and code 0 where it says "no_intersection".  ``to_host`` is accepted for ``RenderedSampler``'s signature."""
        fingers = table_fingers(fingers)
        E, A, Fs = len(self.ids), int(num_actions), len(fingers)
        touch = torch.zeros((E, A, Fs, 121, 121, 3))
        code = torch.zeros((E, A, Fs), dtype=torch.int32)
        pos = torch.zeros((E, A, Fs, 3))
        rot = torch.zeros((E, A, Fs, 3, 3))
        for e, obj in enumerate(self.ids):
            for a in range(A):
                rec = self.record(obj, a)
                if rec is None:
                    continue
                code[e, a] = torch.tensor([STATUS_CODES.get(str(rec["status"][f]), 0) for f in fingers], dtype=torch.int32)
                touch[e, a] = torch.as_tensor(np.asarray(rec["touch"]), dtype=torch.float32)[fingers]
                pos[e, a] = torch.as_tensor(np.asarray(rec["pos"]), dtype=torch.float32)[fingers]
                rot[e, a] = torch.as_tensor(np.asarray(rec["rot"]), dtype=torch.float32)[fingers]
        return {"touch_signal": touch, "touch_code": code, "finger_transfrom_pos": pos, "finger_transform_rot_M": rot}

    def disconnect(self):
        pass
