"""A kinematic Allegro grasp: the reference's hand placement restated, and the finger closing by a kinematic rule on the GPU.

**The closing rule is a kinematic stand-in for five ``stepSimulation`` calls under position control.  No frame of it has been
compared with one of pybullet's.**  The reference's ``Agnostic_Grasp.grasp`` (``simulator/physics/grasping.py:41-65``) sets every
joint's target far past its limit and lets Bullet's contact dynamics decide where the links stop; pybullet is not a dependency of this
package.  Here every finger chain closes on its own in ``steps`` equal steps towards its upper limits, joint by joint from the palm
outwards, and a joint stops for good at the first step whose tentative pose would make one of its distal collision BOXES overlap a
triangle of the object (``ops.grasp_close`` / ``a3vt_grasp_close``, csrc/grasp_close.hip; ``include/a3vt.h`` states the rule in full).
Fingers do not see each other, the palm is not tested, there are no forces, no friction and no object motion.

``place_hand`` is ``Agnostic_Grasp.set_hand_hull`` / ``get_position_on_hull`` (:67-128) with SciPy's ``ConvexHull`` and a ray cast of
its own in place of trimesh.  Difference: the reference takes the face of ``index_tri[0]`` — whatever trimesh returns first — for the
normal while taking the FARTHEST hit for the position; here the normal is the farthest hit's own facet's.  On a convex hull that
contains the origin the ray has one hit and the two agree.

``KinematicGrasp(placement="device")`` places the hand with ``ops.hull_place`` instead (``a3vt_hull_place``, csrc/hull_place.hip): the
same farthest hit and facet plane from a linear programme over the vertices, all actions of all objects in one launch and no hull;
the pairs it leaves undecided (status 2) go to ``place_hand``.  An option: ``DEVICE_PLACEMENT_DEFAULT`` is False.

``KinematicGrasp`` closes all placed grasps of all objects in one ``ops.grasp_close`` call; ``GraspFrames`` serves the result as the
``frames`` mapping of ``RenderedSampler``."""
from collections.abc import Mapping

import numpy as np
import torch

from .... import ops as _ops
from ...utility import utils
from ..hand import poses_as_reference

HAND_DISTANCE = 0.013                 # the reference's hand_distance
FINGERTIP_OFFSET = (0.0, 0.0, 0.133)  # "displacement of the fingertip from the center of the hand" (:100-104)
# Where KinematicGrasp places the hand when it is not told: False = place_hand on the host, True = ops.hull_place.  The device form
# is an option until a change of its own turns it on: its base poses may differ from the host's by one float32 ulp, and with them
# everything downstream (profiles/grasp_place_ab.txt records whether the project's rule for a default is met).
DEVICE_PLACEMENT_DEFAULT = False
_DIRECTIONS = {}


def directions(num_actions):
    """``-get_circle(num_actions).points`` as float64 (the reference's ``self.directions``, :18)."""
    if num_actions not in _DIRECTIONS:
        _DIRECTIONS[num_actions] = -utils.get_circle(num_actions).points.numpy().astype(np.float64)
    return _DIRECTIONS[num_actions]


def hull_facets(verts):
    """The facets (n, 3) of the convex hull of ``verts`` as vertex indices, or None for a hull SciPy refuses (fewer than four
    points, coplanar points, a non-finite coordinate)."""
    from scipy.spatial import ConvexHull, QhullError
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    if len(verts) < 4 or not np.isfinite(verts).all():
        return None
    try:
        return ConvexHull(verts).simplices
    except (QhullError, ValueError):
        return None


def hull_hit(verts, direction, facets=None):
    """The farthest hit of the ray from the origin along ``direction`` with the convex hull of ``verts`` -> ``(point, simplex)``
    (the facet's three vertex indices), or None: no hit, or no hull.  ``facets``: ``hull_facets(verts)`` made ahead (one hull
    serves every action of an object)."""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    facets = hull_facets(verts) if facets is None else facets
    if facets is None:
        return None
    d = np.asarray(direction, np.float64).reshape(3)
    tri = verts[facets]                                           # (n, 3, 3)
    # Moeller-Trumbore for a ray from the origin, all facets at once; hits on an edge count (eps below)
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    h = np.cross(d, e2)
    det = (e1 * h).sum(-1)
    ok = np.abs(det) > 1e-300
    inv = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)
    s = -tri[:, 0]
    u = (s * h).sum(-1) * inv
    qv = np.cross(s, e1)
    v = (qv * d).sum(-1) * inv
    t = (e2 * qv).sum(-1) * inv
    eps = 1e-9
    hit = ok & (u >= -eps) & (v >= -eps) & (u + v <= 1 + eps) & (t > 0)
    if not hit.any():
        return None
    best = np.flatnonzero(hit)[np.argmax(t[hit])]
    return d * t[best], facets[best]


def place_hand(verts, action, num_actions=50, hand_distance=HAND_DISTANCE, facets=None):
    """The hand's base pose ``(pos (3,), rot (3, 3))`` float64 for ``action`` on the object ``verts``, or None for a grasp the
    reference calls "no_intersection" (no hit; also a hull SciPy refuses).  The reference's steps: the ray from the origin along
    ``directions(num_actions)[action]`` against the convex hull, the farthest hit; the facet's normal, flipped to point away from
    the origin; the point ``hand_distance`` along it; ``normal -= 0.001``; the rotation that turns (-1, 0, 0) onto it; the
    position moved back by R (0, 0, 0.133) so that the middle finger's tip, not the palm, sits over the point.  ``facets``:
    ``hull_facets(verts)`` made ahead."""
    from scipy.spatial.transform import Rotation
    verts = np.asarray(verts.detach().cpu().numpy() if isinstance(verts, torch.Tensor) else verts, np.float64).reshape(-1, 3)
    found = hull_hit(verts, directions(num_actions)[action], facets)
    if found is None:
        return None
    point, simplex = found
    normal = utils.normal_from_triangle(verts[simplex[0]], verts[simplex[1]], verts[simplex[2]])
    if (point ** 2).sum() > ((point + normal * 0.0001) ** 2).sum():
        normal = normal * -1
    position = point + normal * hand_distance
    normal = normal - 0.001
    orientation = utils.combine_quats(utils.quats_from_vectors([-1, 0, 0], normal), Rotation.from_euler("xyz", [0, 0, 0]).as_quat())
    rot = Rotation.from_quat(orientation).as_matrix()
    return position - rot.dot(np.array(FINGERTIP_OFFSET)), rot


class KinematicGrasp:
    """``grasp_table``: the finger frames of every action of a list of objects — placement, then ONE ``ops.grasp_close``
    call for all placed grasps of all objects.  ``hand``: a ``HandModel``.  ``device``: where the closing runs (None: the GPU
    when there is one; "cpu" takes the float64 NumPy form of the rule).  ``placement``: "host" — ``place_hand`` per action on
    SciPy's hull — or "device" — ONE ``ops.hull_place`` call for all actions of all objects, ``place_hand`` only for the pairs it
    leaves undecided (status 2); None: ``DEVICE_PLACEMENT_DEFAULT``.  **Not pybullet: see the module's docstring.**"""

    def __init__(self, hand, steps=64, device=None, placement=None):
        if placement is None:
            placement = "device" if DEVICE_PLACEMENT_DEFAULT else "host"
        if placement not in ("host", "device"):
            raise ValueError(f"a3vt: KinematicGrasp: placement={placement!r} must be None, 'host' or 'device'")
        self.placement = placement
        self.hand, self.steps = hand, int(steps)
        self.device = utils._default_device() if device is None else torch.device(device)
        self.table = hand.table()
        self.placement_seconds = 0.0          # host time of the last grasp_table call up to its grasp_close call (tools/grasp_bench.py)
        self.undecided = 0                    # pairs of the last grasp_table call that ops.hull_place left to place_hand

    def _place_on_device(self, verts, verts_t, A):
        """All (object, action) pairs in one ``ops.hull_place`` call and one read of its status -> ``placed`` (the (e, a) pairs
        in row order), ``base_pos`` (G, 3) and ``base_rot`` (G, 3, 3) float32 on the device.  Pairs of status 2 go to
        ``place_hand``, on a hull made when an object's first such pair comes up."""
        found = _ops.hull_place(verts_t, np.cumsum([0] + [len(v) for v in verts]), directions(A), HAND_DISTANCE, FINGERTIP_OFFSET)
        status = found["status"].cpu().numpy()
        pos, rot = found["base_pos"].to(torch.float32).reshape(-1, 3), found["base_rot"].to(torch.float32).reshape(-1, 3, 3)
        present = status == 0
        hulls, rows, poses = {}, [], []
        for e, a in np.argwhere(status == 2).tolist():
            if e not in hulls:
                hulls[e] = hull_facets(verts[e])
            pose = place_hand(verts[e], a, A, facets=hulls[e]) if hulls[e] is not None else None
            if pose is not None:
                present[e, a] = True
                rows.append(e * A + a)
                poses.append(pose)
        self.undecided = int((status == 2).sum())
        if rows:
            at = torch.tensor(rows, dtype=torch.int64, device=pos.device)
            pos[at] = torch.from_numpy(np.array([p for p, _ in poses], np.float32)).to(pos.device)
            rot[at] = torch.from_numpy(np.array([r for _, r in poses], np.float32)).to(pos.device)
        placed = [tuple(pair) for pair in np.argwhere(present).tolist()]
        at = torch.tensor([e * A + a for e, a in placed], dtype=torch.int64, device=pos.device)
        return placed, pos[at], rot[at]

    def grasp_table(self, geometry, ids, num_actions=50, want_q=False, want_blocked_step=False, want_hand_pose=False, want_base=False,
                    want_links=False):
        """``geometry``: a mapping ``{id: (verts, faces)}``.  Returns a dict with ``pos`` (E, A, 4, 3) and ``rot`` (E, A, 4, 3, 3)
        float32 and ``present`` (E, A, 4) bool arrays — ``present`` is false, and the frames zero, for all four fingers of a grasp
        that could not be placed — and on request ``q`` (E, A, 16), ``blocked_step`` (E, A, 16) and ``hand_pose`` (E lists of A
        entries: the reference's list of 28 ``(position, xyz-Euler)`` pairs, None for an unplaced grasp) and ``base_pos``
        (E, A, 3) / ``base_rot`` (E, A, 3, 3) float32, the hand's base poses as ``ops.grasp_close`` got them (``want_base``).
        ``want_links``: also ``link_pos`` (E, A, L, 3) and ``link_rot`` (E, A, L, 3, 3) float32, the world poses of all L links as
        ``ops.grasp_close`` returns them (zero for an unplaced grasp), and the base poses."""
        want_base = want_base or want_links
        import time
        E, A = len(ids), int(num_actions)
        verts, faces, offsets, base = [], [], [0], 0
        placed, base_pos, base_rot = [], [], []
        self.undecided = 0
        start = time.perf_counter()
        for e, obj in enumerate(ids):
            v, f = geometry[obj]
            v, f = np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)
            verts.append(v)
            faces.append(f + base)
            base += len(v)
            offsets.append(offsets[-1] + len(f))
            if self.placement == "device":
                continue
            facets = hull_facets(v)
            for a in range(A if facets is not None else 0):
                pose = place_hand(v, a, A, facets=facets)
                if pose is not None:
                    placed.append((e, a))
                    base_pos.append(pose[0])
                    base_rot.append(pose[1])
        up = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a, dtype)).to(self.device)  # noqa: E731
        verts_t = None
        if self.placement == "device" and E:
            verts_t = up(np.concatenate(verts), np.float32)
            placed, base_pos, base_rot = self._place_on_device(verts, verts_t, A)
        self.placement_seconds = time.perf_counter() - start
        out = dict(pos=np.zeros((E, A, 4, 3), np.float32), rot=np.zeros((E, A, 4, 3, 3), np.float32), present=np.zeros((E, A, 4), bool))
        if want_q:
            out["q"] = np.zeros((E, A, 16), np.float32)
        if want_blocked_step:
            out["blocked_step"] = np.zeros((E, A, 16), np.int32)
        if want_hand_pose:
            out["hand_pose"] = [[None] * A for _ in range(E)]
        if want_base:
            out["base_pos"], out["base_rot"] = np.zeros((E, A, 3), np.float32), np.zeros((E, A, 3, 3), np.float32)
        if want_links:
            L = self.hand.num_links
            out["link_pos"], out["link_rot"] = np.zeros((E, A, L, 3), np.float32), np.zeros((E, A, L, 3, 3), np.float32)
        if not placed:
            return out
        G = len(placed)
        if verts_t is None:
            verts_t = up(np.concatenate(verts), np.float32)
            base_pos_t, base_rot_t = up(np.array(base_pos).reshape(G, 3), np.float32), up(np.array(base_rot).reshape(G, 3, 3), np.float32)
        else:
            base_pos_t, base_rot_t = base_pos, base_rot
            if want_base or want_hand_pose:
                base_pos, base_rot = base_pos_t.cpu().numpy(), base_rot_t.cpu().numpy()
        closed = _ops.grasp_close(verts_t, up(np.concatenate(faces), np.int32), offsets, [e for e, _ in placed], base_pos_t, base_rot_t,
                                  self.table, self.hand.q0, self.steps)
        host = {name: t.cpu().numpy() for name, t in closed.items()
                if name in ("frame_pos", "frame_rot") or (name == "q" and want_q) or (name == "blocked_step" and want_blocked_step)
                or (name in ("link_pos", "link_rot") and (want_hand_pose or want_links))}
        index = tuple(np.array(placed).T)
        out["pos"][index], out["rot"][index], out["present"][index] = host["frame_pos"], host["frame_rot"], True
        if want_q:
            out["q"][index] = host["q"]
        if want_blocked_step:
            out["blocked_step"][index] = host["blocked_step"]
        if want_base:
            out["base_pos"][index], out["base_rot"][index] = np.array(base_pos).reshape(G, 3), np.array(base_rot).reshape(G, 3, 3)
        if want_links:
            out["link_pos"][index], out["link_rot"][index] = host["link_pos"], host["link_rot"]
        if want_hand_pose:
            for g, (e, a) in enumerate(placed):
                out["hand_pose"][e][a] = poses_as_reference(base_pos[g], base_rot[g], host["link_pos"][g], host["link_rot"][g])
        return out


class GraspFrames(Mapping):
    """The ``frames`` mapping of ``RenderedSampler``: keys ``(object_id, action)``, values ``(pos (4, 3), rot (4, 3, 3), present
    (4,))``.  One object's whole action table is made on first touch (one ``grasp_table`` call) and kept.  ``geometry``: the
    mapping ``{id: (verts, faces)}`` the sampler gets too."""

    def __init__(self, grasper, geometry, num_actions=50):
        self.grasper, self.geometry, self.num_actions = grasper, geometry, int(num_actions)
        self._tables, self._link_tables = {}, {}

    def link_table(self, obj):
        """``grasp_table(..., want_links=True)`` of one object, made on first touch and kept, as ``table`` keeps its own; it also
        serves ``table`` (the same call gives the same frames)."""
        if obj not in self._link_tables:
            full = self.grasper.grasp_table(self.geometry, [obj], self.num_actions, want_links=True)
            self._link_tables[obj] = full
            self._tables.setdefault(obj, {name: full[name] for name in ("pos", "rot", "present")})
        return self._link_tables[obj]

    def hand_links(self, obj, action):
        """``(base_pos (3,), base_rot (3, 3), link_pos (L, 3), link_rot (L, 3, 3))`` float32 of a grasp — the hand's base pose and
        the world poses of all its links after closing, what ``HandVisual``'s nodes are posed by —, or None for a grasp that could
        not be placed."""
        if obj not in self.geometry or not 0 <= int(action) < self.num_actions:
            raise KeyError((obj, action))
        t, a = self.link_table(obj), int(action)
        if not t["present"][0, a].any():
            return None
        return t["base_pos"][0, a], t["base_rot"][0, a], t["link_pos"][0, a], t["link_rot"][0, a]

    def table(self, obj):
        if obj not in self._tables:
            self._tables[obj] = self.grasper.grasp_table(self.geometry, [obj], self.num_actions)
        return self._tables[obj]

    def __getitem__(self, key):
        obj, action = key
        if obj not in self.geometry or not 0 <= int(action) < self.num_actions:
            raise KeyError(key)
        t = self.table(obj)
        return t["pos"][0, int(action)], t["rot"][0, int(action)], t["present"][0, int(action)]

    def __iter__(self):
        return ((obj, a) for obj in self.geometry for a in range(self.num_actions))

    def __len__(self):
        return len(self.geometry) * self.num_actions
