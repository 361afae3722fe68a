"""What the posed-render tests build alike: synthetic parts, poses, scenes of instances, the materialised numbering, and the two
views held against the fp64 yardstick of ``scene_render_util``.

A part is ``(verts (n, 3) float32, faces (m, 3) int)`` with local indices; an instance is ``(part index, pos (3,), rot (3, 3), rgb)``;
an image is a list of instances.  ``tables(images)`` flattens them into ``scene_render_posed``'s arrays.  The cameras are
``scene_render_util``'s: NARROW sees +-0.05 around the origin from 1.98 away, so ``fan(n)`` (radius 0.3, in the plane z = 0) fills the
view under any small pose, and a ray that sees the background has leaked through an edge."""
import os

import numpy as np

import scene_render_util as su

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EYE = np.eye(3)
FORWARD = -su.CAM_ROT[:, 2]                       # the NARROW camera's viewing direction, in the world


def fan(n):
    s = su.fan(n)
    return s["verts"], s["faces"]


def tetra(size=0.004):
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) * size
    return v.astype(np.float32), np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])


def box(half=(0.006, 0.004, 0.009)):
    v = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * np.asarray(half)
    f = [[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]]
    return v.astype(np.float32), np.array(f)


def ico(level, radius):
    s = su.ico(level, radius)
    return s["verts"], s["faces"]


def rotation(angles):
    """A generic rotation from three xyz Euler angles in radians (``scene_render_ref.camera_rotation`` takes degrees)."""
    return su.sr.camera_rotation(tuple(np.degrees(angles)))


QUARTER = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])       # 90 degrees about z: exact in any format
GENERIC = rotation((0.3, -0.7, 1.1))


def scatter(n, part=0, seed=3, spread=0.04, rgb=None):
    """n instances of one part at random places of the NARROW view under random rotations."""
    g = np.random.default_rng(seed)
    return [(part, np.append(g.uniform(-spread, spread, 2), g.uniform(-0.01, 0.02)), rotation(g.uniform(-3, 3, 3)),
             su.PALETTE[i % len(su.PALETTE)] if rgb is None else rgb) for i in range(n)]


def tables(images):
    """A list of images -> ``inst_part, inst_pos, inst_rot, inst_rgb, inst_offset`` as arrays of the kernel's types."""
    flat = [inst for image in images for inst in image]
    n = len(flat)
    return dict(inst_part=np.array([i[0] for i in flat], np.int32).reshape(n),
                inst_pos=np.array([i[1] for i in flat], np.float32).reshape(n, 3),
                inst_rot=np.array([i[2] for i in flat], np.float32).reshape(n, 3, 3),
                inst_rgb=np.array([i[3] for i in flat], np.uint8).reshape(n, 3),
                inst_offset=np.cumsum([0] + [len(image) for image in images]).astype(np.int32))


def materialised_index(face_offset, inst_part, face_base, prim_inst, prim_face):
    """(instance, face into the part table) -> the face's row in ``pose_parts``' output: ``face_base[instance] + face -
    face_offset[part]``; -1 stays -1."""
    inst = np.where(prim_inst < 0, 0, prim_inst)
    row = np.asarray(face_base)[inst] + prim_face - np.asarray(face_offset)[np.asarray(inst_part)[inst]]
    return np.where(prim_inst < 0, -1, row).astype(np.int32)


def posed_scene(parts, image):
    """One image's instances as a ``scene_render_util`` scene with the posed triangles formed in FLOAT64 (not rounded to float32:
    the yardstick sees the exact poses of the float32 inputs), and the (instance, part-local face) of every row."""
    verts, faces, rgb, owner, base = [], [], [], [], 0
    for k, (part, pos, rot, colour) in enumerate(image):
        v, f = parts[part]
        R, p = np.asarray(rot, np.float32).astype(np.float64), np.asarray(pos, np.float32).astype(np.float64)
        verts.append(np.asarray(v, np.float32).astype(np.float64) @ R.T + p)
        faces.append(np.asarray(f) + base)
        rgb.append(np.tile(np.asarray(colour, np.uint8), (len(f), 1)))
        owner.append(np.stack([np.full(len(f), k), np.arange(len(f))], 1))
        base += len(v)
    empty = su.make()
    scene = dict(empty, verts=np.concatenate(verts), faces=np.concatenate(faces).astype(np.int32), face_rgb=np.concatenate(rgb))
    return scene, np.concatenate(owner)


# ---- the two yardstick views ---------------------------------------------------------------------------------------------------
YARD_SIZE = (40, 24)


def synthetic_hand():
    """Parts and one image: an icosphere-2 at the origin and, in front of it as the NARROW camera sees it, a "hand" of a box palm
    and five boxes and tetrahedra as fingers, each under a generic pose.  -> (parts, image, camera position, yfov)."""
    parts = [ico(2, 0.03), box((0.012, 0.016, 0.004)), box((0.003, 0.003, 0.012)), tetra(0.006)]
    lift = -FORWARD * 0.06                                                   # towards the camera
    image = [(0, np.zeros(3), EYE, su.PALETTE[0]), (1, lift, rotation((0.5, 0.2, -0.4)), (119, 136, 153))]
    for k in range(4):
        at = lift + su.CAM_ROT @ np.array([0.012 * (k - 1.5), 0.02, 0.004])
        image.append((2, at, rotation((0.4 + 0.1 * k, -0.2, 0.3 * k)), (119, 136, 153)))
        image.append((3, at + su.CAM_ROT @ np.array([0.0, 0.014, 0.006]), rotation((0.2 * k, 1.0, -0.3)), (119, 225, 153)))
    return parts, image, su.NARROW_POS, su.NARROW_YFOV


def golden_hand():
    from a3vt_amd.pterotactyl.simulator.hand import HandModel, HandVisual
    return HandModel.load(os.path.join(GOLDEN, "allegro_hand.npz")), HandVisual.load(os.path.join(GOLDEN, "allegro_hand_visual.npz"))


GRASP_OBJECT = "ball"
GRASP_ACTION = 7


def grasp_geometry():
    from a3vt_amd import mesh
    v, f = mesh.icosphere(2, 0.05)
    return {GRASP_OBJECT: (v.astype(np.float32), f.astype(np.int64))}


def hand_image(visual, links, object_part, colour=su.PALETTE[0]):
    """The instances ``RenderedSampler`` draws for one element: the object at the identity, then the 21 nodes under their links."""
    base_pos, base_rot, link_pos, link_rot = links
    image = [(object_part, np.zeros(3), EYE, colour)]
    for part, link, rgb in visual.nodes:
        image.append((part, base_pos if link < 0 else link_pos[link], base_rot if link < 0 else link_rot[link], rgb))
    return image


def golden_grasp():
    """The golden hand closed on an icosphere by the kinematic grasp's HOST path (float64 NumPy: the same on every machine), seen by
    the reference's vision camera.  -> (parts, image, camera position, camera rotation, yfov)."""
    from a3vt_amd import ops
    from a3vt_amd.pterotactyl.policies.rendered import camera_matrix
    from a3vt_amd.pterotactyl.simulator.physics.grasping import GraspFrames, KinematicGrasp
    hand, visual = golden_hand()
    geometry = grasp_geometry()
    frames = GraspFrames(KinematicGrasp(hand, steps=16, device="cpu"), geometry, num_actions=50)
    links = frames.hand_links(GRASP_OBJECT, GRASP_ACTION)
    assert links is not None
    parts = list(visual.parts) + [geometry[GRASP_OBJECT]]
    D = ops.VISION_DEFAULTS
    return parts, hand_image(visual, links, len(visual.parts)), np.asarray(D["cam_pos"]), camera_matrix(D["cam_euler_xyz_deg"]), D["yfov"]


_YARD = {}


def yard_view(name):
    """``(parts, image, pos, rot, yfov, scene, owner, reference)`` of "synthetic" or "golden": computed once, shared, never changed."""
    if name not in _YARD:
        if name == "synthetic":
            parts, image, pos, yfov = synthetic_hand()
            rot = su.CAM_ROT
        else:
            parts, image, pos, rot, yfov = golden_grasp()
        scene, owner = posed_scene(parts, image)
        D = vision_scene()
        want = su.reference(scene, *YARD_SIZE, pos=pos, rot=rot, yfov=yfov, lights=D["lights"], ambient=D["ambient"],
                            background=D["background"], znear=D["znear"], zfar=D["zfar"])
        _YARD[name] = (parts, image, pos, rot, yfov, scene, owner, want)
    return _YARD[name]


def vision_scene():
    from a3vt_amd import ops
    D = ops.VISION_DEFAULTS
    return dict(lights=np.asarray(D["lights"]), ambient=D["ambient"], background=D["background"], znear=D["znear"], zfar=D["zfar"])
