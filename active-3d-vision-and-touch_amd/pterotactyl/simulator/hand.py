"""``HandModel``: the numbers of the reference's Allegro hand (``objects/hand/allegro_hand.urdf``) that a kinematic grasp needs — the
link tree, the joint origins, axes and limits, and ONE collision box per link — with forward kinematics on the host in float64.

The package commits no hand data and carries no default asset: ``HandModel.load(path)`` reads a URDF (parsed with ``xml.etree``; its
collision meshes are binary STL files beside it) or a ``.npz`` holding the same numbers (``HandModel.save``), and with ``path=None`` the
file that the environment variable ``PTEROTACTYL_HAND`` names.

Link numbering.  The table has the URDF's links without the base, in depth-first order from the base, the children of a link in the
order of their joints in the file.  For the Allegro URDF that is 28 links in four chains ``0-6``, ``7-13``, ``14-20``, ``21-27``, each
chain four revolute joints, then ``tip``, ``end`` and ``end_cam``; ``TOUCH_CAMERAS = [6, 13, 20, 27]`` are then the ``end_cam_*``
links.  **This numbering is inferred from the reference's camera indices (``touch_cameras`` of ``simulator/scene/instance.py``); it has
not been checked against pybullet's own link indices.**

Rest pose ``q0``: literally ``Agnostic_Grasp.reset_hand`` (``simulator/physics/grasping.py:130-139``): all zero, ``q[20] = 1.2``,
``q[22] = 0.7``.  Under the numbering above index 20 is a FIXED joint (``end_cam`` of the third chain), so that entry has no effect:
an angle of a fixed joint is ignored everywhere here.  It is kept as the reference writes it.

Collision boxes.  The URDF's ``<box>`` where a link's collision gives one, otherwise the axis-aligned bounds of the collision mesh's
vertices under the collision origin: centre and half-extents in the link frame.  A box whose largest extent is below 1 mm (the
``end_*`` markers) is dropped: that link carries no box.  This is a simplification of the collision geometry, part of the kinematic
stand-in (``physics/grasping.py``); pybullet collides with the meshes' convex hulls.

``HandVisual``: the hand's VISUAL meshes as the reference's vision scene draws them (``simulator/rendering/vision_renderer.py``):
ten distinct parts and the 21 nodes that place them on the base and on 20 links.  It carries no data either: see ``HandVisual.load``."""
import math
import os
import struct
import xml.etree.ElementTree as ET

import numpy as np

TOUCH_CAMERAS = [6, 13, 20, 27]
# The columns of ``HandModel.table()`` (float64, one row per link): what ``ops.grasp_close`` and ``a3vt_grasp_close`` take.
COL_PARENT, COL_TYPE, COL_XYZ, COL_ROT, COL_AXIS, COL_LOWER, COL_UPPER, COL_HAS_BOX, COL_BOX_CENTRE, COL_BOX_HALF, TABLE_COLS = \
    0, 1, 2, 5, 14, 17, 18, 19, 20, 23, 26
MIN_BOX_EXTENT = 1e-3
# The vision scene's hand (vision_renderer.py:17-18, :94-123, :140-161).  The digit's alpha (175) is not used: it is drawn opaque.
HAND_COLOUR, DIGIT_COLOUR = (119, 136, 153), (119, 225, 153)
VISUAL_PARTS = ("0_base", "1_finger", "2_finger", "3_finger", "4_finger", "5_digit", "6_thumb", "7_thumb", "8_thumb", "9_thumb")
# init_hand's nodes in order, as part indices: the base, three fingers of four segments and a digit, the thumb's four and a digit
VISUAL_NODE_PARTS = (0,) + (1, 2, 3, 4, 5) * 3 + (6, 7, 8, 9, 5)
# update_hand's index list: the link whose pose each node after the base takes, as rows of HandModel's table
VISUAL_NODE_LINKS = (-1, 0, 1, 2, 3, 4, 7, 8, 9, 10, 11, 14, 15, 16, 17, 18, 21, 22, 23, 24, 25)
_FIELDS = ("names", "parent", "origin_xyz", "origin_rpy", "axis", "revolute", "lower", "upper", "has_box", "box_centre", "box_half", "q0")


def rpy_matrix(rpy):
    """A URDF ``rpy`` triple as a matrix: fixed-axis roll, pitch, yaw, R = Rz(yaw) Ry(pitch) Rx(roll)."""
    (cr, sr), (cp, sp), (cy, sy) = ((math.cos(a), math.sin(a)) for a in rpy)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]], np.float64)


def axis_angle_matrix(axis, angle):
    """Rodrigues' formula about the normalised ``axis``."""
    x, y, z = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    c, s = math.cos(angle), math.sin(angle)
    t = 1.0 - c
    return np.array([[t * x * x + c, t * x * y - s * z, t * x * z + s * y],
                     [t * x * y + s * z, t * y * y + c, t * y * z - s * x],
                     [t * x * z - s * y, t * y * z + s * x, t * z * z + c]], np.float64)


def matrix_euler_xyz(R):
    """The fixed-axis xyz angles (roll, pitch, yaw) of a rotation matrix, R = Rz(yaw) Ry(pitch) Rx(roll): what
    ``getEulerFromQuaternion`` returns and ``utils.euler_matrix(angles, "xyz")`` turns back into R."""
    return (math.atan2(R[2, 1], R[2, 2]), -math.asin(min(1.0, max(-1.0, R[2, 0]))), math.atan2(R[1, 0], R[0, 0]))


def read_stl_vertices(path):
    """The (3 n, 3) float64 vertices of a binary STL file."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 84:
        raise ValueError(f"a3vt: {path!r} is too short for a binary STL file")
    n = struct.unpack("<I", data[80:84])[0]
    if len(data) < 84 + 50 * n:
        raise ValueError(f"a3vt: {path!r} announces {n} triangles and holds {len(data)} bytes (an ASCII STL file is not read)")
    rows = np.frombuffer(data, dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]), count=n, offset=84)
    return rows["v"].reshape(-1, 3).astype(np.float64)


def _floats(text, n, default):
    if text is None:
        return np.array(default, np.float64)
    values = np.array([float(w) for w in text.split()], np.float64)
    if values.shape != (n,):
        raise ValueError(f"a3vt: hand URDF: {text!r} is not {n} numbers")
    return values


def _origin(element):
    o = None if element is None else element.find("origin")
    return (_floats(None if o is None else o.get("xyz"), 3, [0, 0, 0]), _floats(None if o is None else o.get("rpy"), 3, [0, 0, 0]))


def _collision_box(link, directory):
    """``(centre, half)`` of a ``<link>``'s first collision in the link frame, or None."""
    collision = link.find("collision")
    geometry = None if collision is None else collision.find("geometry")
    if geometry is None:
        return None
    xyz, rpy = _origin(collision)
    R = rpy_matrix(rpy)
    box, mesh = geometry.find("box"), geometry.find("mesh")
    if box is not None:
        half = _floats(box.get("size"), 3, None) / 2.0
        corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * half
    elif mesh is not None:
        corners = read_stl_vertices(os.path.join(directory, mesh.get("filename"))) * _floats(mesh.get("scale"), 3, [1, 1, 1])
    else:
        return None
    points = corners @ R.T + xyz
    lo, hi = points.min(axis=0), points.max(axis=0)
    if (hi - lo).max() < MIN_BOX_EXTENT:
        return None
    return (lo + hi) / 2.0, (hi - lo) / 2.0


class HandModel:
    """The link table described in the module's docstring.  Arrays, one row per link: ``names``, ``parent`` (-1: the base),
    ``origin_xyz`` / ``origin_rpy`` (the joint's origin in the parent's frame), ``axis``, ``revolute`` (bool; every other joint is
    treated as fixed), ``lower`` / ``upper``, ``has_box``, ``box_centre`` / ``box_half``; and ``q0``."""

    def __init__(self, **fields):
        for name in _FIELDS:
            setattr(self, name, np.asarray(fields[name]))
        n = len(self.parent)
        self.num_links = n
        if n % 4 or any(self.parent[i] >= i for i in range(n)):
            raise ValueError("a3vt: hand: the links are not four chains in depth-first order")
        self.chain = n // 4
        self.origin_rot = np.stack([rpy_matrix(r) for r in self.origin_rpy]) if n else np.zeros((0, 3, 3))
        self.touch_cameras = [c * self.chain + self.chain - 1 for c in range(4)]

    @classmethod
    def load(cls, path=None):
        """A ``HandModel`` from a URDF or a ``.npz``; ``path=None``: the file the environment variable ``PTEROTACTYL_HAND`` names."""
        if path is None:
            path = os.environ.get("PTEROTACTYL_HAND")
            if not path:
                raise ValueError("a3vt: HandModel.load: no path given and PTEROTACTYL_HAND is not set (the package carries no hand "
                                 "data: pass the reference's objects/hand/allegro_hand.urdf or an .npz made by HandModel.save)")
        path = str(path)
        if path.endswith(".npz"):
            with np.load(path, allow_pickle=False) as z:
                return cls(**{name: z[name] for name in _FIELDS})
        return cls._from_urdf(path)

    def save(self, path):
        """The numbers as a ``.npz`` (no program text, no mesh): what ``load`` reads back array by array."""
        np.savez(path, **{name: getattr(self, name) for name in _FIELDS})

    @classmethod
    def _from_urdf(cls, path):
        root = ET.parse(path).getroot()
        directory = os.path.dirname(os.path.abspath(path))
        links = {link.get("name"): link for link in root.findall("link")}
        joints = root.findall("joint")                                    # in file order
        children = {joint.find("child").get("link") for joint in joints}
        roots = [name for name in links if name not in children]
        if len(roots) != 1:
            raise ValueError(f"a3vt: hand URDF {path!r}: expected one base link, found {roots}")
        rows = []

        def visit(parent_name, parent_index):
            for joint in joints:
                if joint.find("parent").get("link") != parent_name:
                    continue
                child = joint.find("child").get("link")
                xyz, rpy = _origin(joint)
                axis = joint.find("axis")
                limit = joint.find("limit")
                revolute = joint.get("type") == "revolute"
                rows.append(dict(name=child, parent=parent_index, xyz=xyz, rpy=rpy,
                                 axis=_floats(None if axis is None else axis.get("xyz"), 3, [1, 0, 0]), revolute=revolute,
                                 lower=float(limit.get("lower", 0.0)) if revolute and limit is not None else 0.0,
                                 upper=float(limit.get("upper", 0.0)) if revolute and limit is not None else 0.0,
                                 box=_collision_box(links[child], directory)))
                visit(child, len(rows) - 1)
        visit(roots[0], -1)
        n = len(rows)
        q0 = np.zeros(n, np.float64)
        if n > 22:                                                        # reset_hand, literally (index 20 is a fixed joint here)
            q0[20], q0[22] = 1.2, 0.7
        zero = np.zeros(3)
        return cls(names=np.array([r["name"] for r in rows]), parent=np.array([r["parent"] for r in rows], np.int32),
                   origin_xyz=np.array([r["xyz"] for r in rows]), origin_rpy=np.array([r["rpy"] for r in rows]),
                   axis=np.array([r["axis"] for r in rows]), revolute=np.array([r["revolute"] for r in rows], bool),
                   lower=np.array([r["lower"] for r in rows]), upper=np.array([r["upper"] for r in rows]),
                   has_box=np.array([r["box"] is not None for r in rows], bool),
                   box_centre=np.array([zero if r["box"] is None else r["box"][0] for r in rows]),
                   box_half=np.array([zero if r["box"] is None else r["box"][1] for r in rows]), q0=q0)

    def table(self):
        """The (num_links, TABLE_COLS) float64 table of ``ops.grasp_close``: parent, type (1 revolute, 0 fixed), origin xyz, origin
        rotation (row-major), axis (normalised), lower, upper, has_box, box centre, box half-extents."""
        t = np.zeros((self.num_links, TABLE_COLS), np.float64)
        t[:, COL_PARENT], t[:, COL_TYPE] = self.parent, self.revolute
        t[:, COL_XYZ:COL_XYZ + 3], t[:, COL_ROT:COL_ROT + 9] = self.origin_xyz, self.origin_rot.reshape(-1, 9)
        t[:, COL_AXIS:COL_AXIS + 3] = self.axis / np.linalg.norm(self.axis, axis=1, keepdims=True)
        t[:, COL_LOWER], t[:, COL_UPPER], t[:, COL_HAS_BOX] = self.lower, self.upper, self.has_box
        t[:, COL_BOX_CENTRE:COL_BOX_CENTRE + 3], t[:, COL_BOX_HALF:COL_BOX_HALF + 3] = self.box_centre, self.box_half
        return t

    def forward(self, base_pos, base_rot, q):
        """The links' world poses ``(pos (n, 3), rot (n, 3, 3))`` in float64 for the base pose and the joint angles ``q`` (n,); the
        entry of a fixed joint is ignored."""
        base_pos, base_rot, q = np.asarray(base_pos, np.float64).reshape(3), np.asarray(base_rot, np.float64).reshape(3, 3), \
            np.asarray(q, np.float64).reshape(self.num_links)
        pos, rot = np.zeros((self.num_links, 3)), np.zeros((self.num_links, 3, 3))
        for i in range(self.num_links):
            p, R = (base_pos, base_rot) if self.parent[i] < 0 else (pos[self.parent[i]], rot[self.parent[i]])
            pos[i] = p + R @ self.origin_xyz[i]
            rot[i] = R @ self.origin_rot[i]
            if self.revolute[i]:
                rot[i] = rot[i] @ axis_angle_matrix(self.axis[i], q[i])
        return pos, rot

    def frames(self, base_pos, base_rot, q):
        """The finger frames: the rows of the ``touch_cameras`` links, ``(pos (4, 3), rot (4, 3, 3))``."""
        pos, rot = self.forward(base_pos, base_rot, q)
        return pos[self.touch_cameras], rot[self.touch_cameras]

    def hand_pose(self, base_pos, base_rot, q):
        """The reference's ``get_hand_pose`` (``instance.py:70-84``): a list of ``num_links`` ``(position, xyz-Euler)`` pairs.  Entry
        0 is the BASE's, as the reference's ``get_pose`` answers for ``linkID <= 0``; entry i > 0 is link i's."""
        pos, rot = self.forward(base_pos, base_rot, q)
        return poses_as_reference(np.asarray(base_pos, np.float64).reshape(3), np.asarray(base_rot, np.float64).reshape(3, 3), pos, rot)


def poses_as_reference(base_pos, base_rot, link_pos, link_rot):
    """Link poses in ``hand_pose``'s form: entry 0 the base's, entry i > 0 link i's, each ``(position tuple, xyz-Euler tuple)``."""
    out = [(tuple(float(x) for x in base_pos), matrix_euler_xyz(np.asarray(base_rot, np.float64)))]
    for i in range(1, len(link_pos)):
        out.append((tuple(float(x) for x in link_pos[i]), matrix_euler_xyz(np.asarray(link_rot[i], np.float64))))
    return out


class HandVisual:
    """The hand of the reference's vision scene: ``parts``, a list of ``(verts (n, 3) float32, faces (m, 3) int32)`` — the distinct
    meshes, each once —, and ``nodes``, a list of ``(part, link, rgb)``: ``init_hand``'s 21 nodes in its order, ``link`` the row of
    ``HandModel``'s table whose pose ``update_hand`` gives the node (-1: the base), ``rgb`` ``HAND_COLOUR`` or, for the four
    ``5_digit`` nodes, ``DIGIT_COLOUR``.

    The parts are drawn in the link frames ``ops.grasp_close`` returns.  The reference poses them by ``getLinkState(...)[:2]``, the
    INERTIAL frame; none of the URDF's 29 links gives its ``<inertial>`` an ``<origin>``, so the two frames coincide and no
    correction is applied.  Faces are taken as stored (no ``add_faces``; the caster is two-sided).  Seen on the reference's files:
    every finger part's bounds equal its link's collision box in the link frame, except ``6_thumb`` on link 21, whose bounds are the
    box's turned half a turn about x (it is drawn as the file has it), and ``5_digit``, whose collision mesh is another file."""

    def __init__(self, parts, nodes=None):
        self.parts = [(np.ascontiguousarray(v, np.float32).reshape(-1, 3), np.ascontiguousarray(f, np.int32).reshape(-1, 3)) for v, f in parts]
        if nodes is None:
            nodes = [(part, link, DIGIT_COLOUR if VISUAL_PARTS[part] == "5_digit" else HAND_COLOUR)
                     for part, link in zip(VISUAL_NODE_PARTS, VISUAL_NODE_LINKS)]
        self.nodes = [(int(part), int(link), tuple(int(c) for c in rgb)) for part, link, rgb in nodes]
        for p, (v, f) in enumerate(self.parts):
            if len(f) and (f.min() < 0 or f.max() >= len(v)):
                raise ValueError(f"a3vt: HandVisual: part {p} has face indices outside its {len(v)} vertices")
        if any(not 0 <= part < len(self.parts) or link < -1 or len(rgb) != 3 for part, link, rgb in self.nodes):
            raise ValueError("a3vt: HandVisual: a node names a part that is not there, a link below -1 or a colour that is not RGB")

    @property
    def links(self):
        """The nodes' link rows, in node order (-1: the base)."""
        return [link for _, link, _ in self.nodes]

    @property
    def num_faces(self):
        return sum(len(self.parts[part][1]) for part, _, _ in self.nodes)

    @classmethod
    def load(cls, path=None):
        """A ``HandVisual`` from a directory laid out as the reference's ``objects/hand/meshes_obj`` (``<part>.obj`` for the ten
        names of ``VISUAL_PARTS``, read with ``mesh.load_obj``) or from a ``.npz`` made by ``save``; ``path=None``: what the
        environment variable ``PTEROTACTYL_HAND_MESHES`` names."""
        if path is None:
            path = os.environ.get("PTEROTACTYL_HAND_MESHES")
            if not path:
                raise ValueError("a3vt: HandVisual.load: no path given and PTEROTACTYL_HAND_MESHES is not set (the package carries no "
                                 "hand data: pass the reference's objects/hand/meshes_obj or an .npz made by HandVisual.save)")
        path = str(path)
        if path.endswith(".npz"):
            with np.load(path, allow_pickle=False) as z:
                names = [str(n) for n in z["part_names"]]
                parts = [(z[f"verts_{n}"], z[f"faces_{n}"]) for n in names]
                nodes = list(zip(z["node_part"].tolist(), z["node_link"].tolist(), z["node_rgb"].tolist()))
            return cls(parts, nodes)
        from ... import mesh
        return cls([mesh.load_obj(os.path.join(path, name + ".obj")) for name in VISUAL_PARTS])

    def save(self, path):
        """The parts and nodes as a ``.npz``: arrays only (float32 vertices, int32 faces, the node table)."""
        names = [VISUAL_PARTS[p] if len(self.parts) == len(VISUAL_PARTS) else f"part{p}" for p in range(len(self.parts))]
        arrays = {"part_names": np.array(names), "node_part": np.array([n[0] for n in self.nodes], np.int32),
                  "node_link": np.array([n[1] for n in self.nodes], np.int32), "node_rgb": np.array([n[2] for n in self.nodes], np.uint8)}
        for name, (v, f) in zip(names, self.parts):
            arrays[f"verts_{name}"], arrays[f"faces_{name}"] = v, f
        np.savez_compressed(path, **arrays)
