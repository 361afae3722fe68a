"""CPU tests of the kinematic grasp's host side: the hand description (``simulator/hand.py``), the placement
(``simulator/physics/grasping.py::place_hand``), the closing rule (``ops.grasp_close`` on CPU tensors, the vectorised float64 NumPy
path, against ``grasp_ref``'s loop-by-loop statement), ``GraspFrames`` and ``data_making.save_simulation``.

**The closing rule is a kinematic stand-in for pybullet's five ``stepSimulation`` calls; nothing here compares a frame with
pybullet's.**"""
import os

import numpy as np
import pytest
import torch

import grasp_ref as gr

# Both sides of these comparisons work in float64, where the chain's arithmetic errs by about 1e-15 m: a query whose |separation| is
# at least this is decided for both with a margin of 1e6.
HOST_DECIDED = 1e-9


@pytest.fixture(scope="module")
def hand():
    return gr.hand()


def close_host(hand, meshes, which, base_pos, base_rot, steps):
    from a3vt_amd import ops
    verts, faces, offsets = gr.batch(meshes)
    out = ops.grasp_close(torch.from_numpy(verts), torch.from_numpy(faces.astype(np.int32)), offsets, which,
                          torch.from_numpy(np.asarray(base_pos, np.float32)), torch.from_numpy(np.asarray(base_rot, np.float32)),
                          hand.table(), hand.q0, steps)
    ref = gr.close(verts, faces, offsets, which, np.asarray(base_pos, np.float32), np.asarray(base_rot, np.float32), hand, steps)
    return {k: v.numpy() for k, v in out.items()}, ref


def upper16(hand):
    return np.array([hand.upper[7 * c + j] for c in range(4) for j in range(4)])


# ---- the hand ------------------------------------------------------------------------------------------------------------------
def test_parser_against_the_fixture(hand):
    from oracle.ref_shim import REFERENCE_ROOT
    from a3vt_amd.pterotactyl.simulator.hand import _FIELDS, HandModel
    urdf = os.path.join(REFERENCE_ROOT, "pterotactyl", "objects", "hand", "allegro_hand.urdf")
    if not os.path.exists(urdf):
        pytest.skip("the reference's hand files are not on this machine")
    live = HandModel.load(urdf)
    for name in _FIELDS:
        assert np.array_equal(getattr(live, name), getattr(hand, name)), name


def test_link_table(hand):
    assert hand.num_links == 28 and hand.chain == 7 and hand.touch_cameras == [6, 13, 20, 27]
    assert [str(hand.names[i]) for i in hand.touch_cameras] == ["end_cam_0", "end_cam_1", "end_cam_2", "end_cam_3"]
    assert [str(hand.names[7 * c]) for c in range(4)] == ["link_8.0", "link_4.0", "link_0.0", "link_12.0"]
    for c in range(4):
        assert hand.revolute[7 * c:7 * c + 7].tolist() == [True] * 4 + [False] * 3
        assert hand.parent[7 * c:7 * c + 7].tolist() == [-1] + [7 * c + k for k in (0, 1, 2, 3, 4, 4)]
    # the revolute limits as in the file
    assert (hand.lower[0], hand.upper[0]) == (-0.47, 0.47) and (hand.lower[1], hand.upper[1]) == (-0.196, 1.61)
    assert (hand.lower[9], hand.upper[9]) == (-0.174, 1.709) and (hand.lower[17], hand.upper[17]) == (-0.227, 1.618)
    assert (hand.lower[21], hand.upper[21]) == (0.263, 1.396) and (hand.lower[24], hand.upper[24]) == (-0.162, 1.719)
    for tip in (4, 11, 18, 25):          # link_11.0_tip, link_7.0_tip, link_3.0_tip, link_15.0_tip: the URDF's own boxes
        assert hand.has_box[tip] and np.allclose(2 * hand.box_half[tip], [0.028, 0.028, 0.034], atol=1e-15)
        assert np.allclose(hand.box_centre[tip], [-0.0023, 0, 0], atol=1e-15)
    for c in range(4):                   # the end_* markers carry none; every other link has one from its mesh
        assert not hand.has_box[7 * c + 5] and not hand.has_box[7 * c + 6] and hand.has_box[7 * c:7 * c + 5].all()
    q0 = np.zeros(28)
    q0[20], q0[22] = 1.2, 0.7
    assert np.array_equal(hand.q0, q0) and not hand.revolute[20] and hand.revolute[22]
    table = hand.table()
    assert table.shape == (28, 26) and np.allclose(np.linalg.norm(table[:, 14:17], axis=1), 1.0)


def test_load_needs_a_path(monkeypatch, tmp_path, hand):
    from a3vt_amd.pterotactyl.simulator.hand import HandModel
    monkeypatch.delenv("PTEROTACTYL_HAND", raising=False)
    with pytest.raises(ValueError, match="PTEROTACTYL_HAND"):
        HandModel.load()
    path = str(tmp_path / "hand.npz")
    hand.save(path)
    monkeypatch.setenv("PTEROTACTYL_HAND", path)
    assert np.array_equal(HandModel.load().table(), hand.table())


def test_forward_kinematics(hand):
    from a3vt_amd.pterotactyl.utility import utils
    pos, rot = hand.forward(np.zeros(3), np.eye(3), np.zeros(28))
    for c, cam in enumerate(hand.touch_cameras):
        # at q = 0 the chain's frames differ from the base's by the joint origins alone: summed by hand along base -> 0 1 2 3 tip cam
        R, p = np.eye(3), np.zeros(3)
        for i in [7 * c + k for k in (0, 1, 2, 3, 4, 6)]:
            r, pt, y = hand.origin_rpy[i]
            p = p + R @ hand.origin_xyz[i]
            R = R @ utils.euler_matrix([r, pt, y], "xyz")
        assert np.allclose(pos[cam], p, atol=1e-15) and np.allclose(rot[cam], R, atol=1e-15)
    fp, fr = hand.frames(np.zeros(3), np.eye(3), np.zeros(28))
    assert np.array_equal(fp, pos[[6, 13, 20, 27]]) and np.array_equal(fr, rot[[6, 13, 20, 27]])
    q = np.zeros(28)
    q[9] = 0.5                           # the third joint of the second chain: only links 9..13 move
    pos2, rot2 = hand.forward(np.zeros(3), np.eye(3), q)
    moved = np.array([not (np.array_equal(pos[i], pos2[i]) and np.array_equal(rot[i], rot2[i])) for i in range(28)])
    assert moved.tolist() == [9 <= i <= 13 for i in range(28)]
    assert np.array_equal(pos[9], pos2[9]) and not np.array_equal(pos[10], pos2[10])
    q[20] = 3.0                          # a fixed joint's entry has no effect
    assert np.array_equal(hand.forward(np.zeros(3), np.eye(3), q)[0], pos2)
    # a moved base, and hand_pose's angles back through utils.euler_matrix
    base_rot = utils.euler_matrix([0.3, -0.7, 1.9], "xyz")
    base_pos = np.array([0.1, -0.2, 0.05])
    q = hand.q0 + 0.3 * (hand.upper - hand.q0)
    pos, rot = hand.forward(base_pos, base_rot, q)
    pose = hand.hand_pose(base_pos, base_rot, q)
    assert len(pose) == 28 and np.allclose(pose[0][0], base_pos) and np.allclose(utils.euler_matrix(pose[0][1], "xyz"), base_rot, atol=1e-12)
    for i in range(1, 28):
        assert np.allclose(pose[i][0], pos[i]) and np.allclose(utils.euler_matrix(pose[i][1], "xyz"), rot[i], atol=1e-12), i


def test_vector_helpers():
    from a3vt_amd.pterotactyl.utility import utils
    from scipy.spatial.transform import Rotation
    n = utils.normal_from_triangle(np.array([0.0, 0, 0]), np.array([2.0, 0, 0]), np.array([0.0, 3, 0]))
    assert np.allclose(n, [0, 0, 1])
    target = np.array([0.2, -0.5, 0.7])
    R = Rotation.from_quat(utils.quats_from_vectors([-1, 0, 0], target)).as_matrix()
    assert np.allclose(R @ np.array([-1.0, 0, 0]), target / np.linalg.norm(target)) and np.allclose(R @ R.T, np.eye(3))
    a, b = Rotation.from_euler("xyz", [0.1, 0.2, 0.3]), Rotation.from_euler("xyz", [-0.4, 0.5, 0.6])
    assert np.allclose(Rotation.from_quat(utils.combine_quats(a.as_quat(), b.as_quat())).as_matrix(), a.as_matrix() @ b.as_matrix())


# ---- placement -----------------------------------------------------------------------------------------------------------------
def hull_distance(verts, point):
    """max over the hull's facets of the signed distance of ``point`` to the facet's plane: 0 on the hull, negative inside."""
    from scipy.spatial import ConvexHull
    eq = ConvexHull(np.asarray(verts, np.float64)).equations
    return (eq[:, :3] @ point + eq[:, 3]).max()


@pytest.mark.parametrize("shape", ["sphere", "cube", "ellipsoid"])
def test_placement(shape):
    from a3vt_amd.pterotactyl.simulator.physics import grasping
    verts = {"sphere": gr.icosphere(2, 0.08)[0], "cube": gr.box_mesh((0.05, 0.05, 0.05))[0],
             "ellipsoid": gr.icosphere(2, 0.1, (1.0, 0.6, 0.4))[0]}[shape].astype(np.float64)
    for action in range(0, 50, 7):
        d = grasping.directions(50)[action]
        point, simplex = grasping.hull_hit(verts, d)
        assert abs(hull_distance(verts, point)) < 1e-12 and np.linalg.norm(np.cross(point, d)) < 1e-12 and point @ d > 0
        pos, rot = grasping.place_hand(verts, action)
        assert np.allclose(rot @ rot.T, np.eye(3), atol=1e-12) and np.linalg.det(rot) > 0
        normal = np.cross(verts[simplex[1]] - verts[simplex[0]], verts[simplex[2]] - verts[simplex[0]])
        normal /= np.linalg.norm(normal)
        normal = normal if normal @ point > 0 else -normal        # outward: the origin is inside
        assert np.allclose(pos + rot @ np.array([0, 0, 0.133]), point + 0.013 * normal, atol=1e-12)
        aim = normal - 0.001
        assert np.allclose(rot @ np.array([-1.0, 0, 0]), aim / np.linalg.norm(aim), atol=1e-9)


def test_placement_without_a_grasp():
    from a3vt_amd.pterotactyl.simulator.physics import grasping
    flat = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 0]], np.float64) - [0.5, 0.5, 0]
    assert grasping.place_hand(flat, 0) is None and grasping.place_hand(flat[:3], 3) is None
    # an object that does not contain the origin: the ray misses it (no grasp) or passes through it (two hits: the farther one)
    away = gr.icosphere(2, 0.08, centre=(0.1, 0.0, 0.0))[0].astype(np.float64)
    hits = 0
    for action in range(50):
        found = grasping.hull_hit(away, grasping.directions(50)[action])
        if found is None:
            assert grasping.place_hand(away, action) is None
            continue
        hits += 1
        point, _ = found
        d = grasping.directions(50)[action]
        assert abs(hull_distance(away, point)) < 1e-12 and (point - [0.1, 0.0, 0.0]) @ d > 0      # where the ray LEAVES the sphere
        assert grasping.place_hand(away, action) is not None
    assert 0 < hits < 50


# ---- the rule ------------------------------------------------------------------------------------------------------------------
def test_nothing_to_touch(hand):
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))
    far = gr.icosphere(1, 0.05, centre=(2.0, 0.0, 0.0))
    pos, rot = np.zeros((2, 3)), np.stack([np.eye(3), np.eye(3)])
    got, ref = close_host(hand, [empty, far], [0, 1], pos, rot, 8)
    assert (got["blocked_step"] == 8).all() and np.array_equal(got["q"], np.tile(upper16(hand), (2, 1)))
    assert (ref[1] == 8).all() and np.allclose(ref[0], got["q"], atol=1e-12)
    q = hand.q0.copy()
    for c in range(4):
        q[7 * c:7 * c + 4] = hand.upper[7 * c:7 * c + 4]
    lp, lr = hand.forward(np.zeros(3), np.eye(3), q)
    assert np.allclose(got["link_pos"][0], lp, atol=1e-15) and np.allclose(got["link_rot"][1], lr, atol=1e-15)
    assert np.array_equal(got["frame_pos"], got["link_pos"][:, [6, 13, 20, 27]])


def test_overlap_at_the_rest_pose(hand):
    """A triangle through link 1 of finger 0 at q0.  Joint 1 cannot take a step, and neither can joint 0, whose tested links
    (itself and everything distal) include link 1; joints 2 and 3 test only links beyond it and move; no other finger is touched."""
    pos, rot = gr.chain_poses(hand, 0, np.zeros(3), np.eye(3), hand.q0[:7])
    centre = pos[1] + rot[1] @ hand.box_centre[1]
    tri = (centre + np.array([[0.03, 0.001, 0.0], [-0.03, 0.002, 0.004], [0.0, -0.001, -0.005]])).astype(np.float32)
    got, ref = close_host(hand, [(tri, np.array([[0, 1, 2]]))], [0], np.zeros((1, 3)), np.eye(3)[None], 16)
    assert np.array_equal(got["blocked_step"], ref[1]) and ref[2].min() >= HOST_DECIDED
    assert (got["blocked_step"][0, :2] == 0).all() and (got["blocked_step"][0, 2:4] > 0).all() and (got["blocked_step"][0, 4:] == 16).all()
    assert np.array_equal(got["q"][0, :2], hand.q0[:2])


@pytest.mark.parametrize("finger", [0, 1, 2, 3])
def test_one_triangle_in_one_fingers_path(hand, finger):
    tri = gr.blocking_triangle(hand, finger, 0.4)
    got, ref = close_host(hand, [tri], [0], np.zeros((1, 3)), np.eye(3)[None], 32)
    assert ref[2].min() >= HOST_DECIDED
    assert np.array_equal(got["blocked_step"], ref[1]) and np.allclose(got["q"], ref[0], atol=1e-12)
    mine = got["blocked_step"][0, 4 * finger:4 * finger + 4]
    assert (mine < 32).any() and (np.delete(got["blocked_step"][0], range(4 * finger, 4 * finger + 4)) == 32).all()
    # the tip box reaches a triangle through its centre at 40 % of the way before step 0.4 * 32, and after the first step
    assert 0 < mine.min() < 0.4 * 32
    assert np.allclose(got["link_pos"][0], ref[3][0], atol=1e-12) and np.allclose(got["link_rot"][0], ref[4][0], atol=1e-12)


@pytest.mark.parametrize("steps", [1, 5])
def test_against_the_loop_reference_on_meshes(hand, steps):
    meshes = [gr.icosphere(2, 0.08), gr.box_mesh()]
    which, pos, rot = gr.placements(meshes, [(0, 9), (1, 6), (0, 30), (1, 27)])
    got, ref = close_host(hand, meshes, which, pos, rot, steps)
    decided = np.repeat(ref[2] >= HOST_DECIDED, 4, axis=1)
    assert decided.mean() >= 0.9
    assert np.array_equal(got["blocked_step"][decided], ref[1][decided]) and np.allclose(got["q"][decided], ref[0][decided], atol=1e-12)
    assert (got["blocked_step"] < steps).any() and (got["blocked_step"] == steps).any()
    if steps == 1:                       # one step: a joint is at q0 or at its upper limit
        up, rest = np.tile(upper16(hand), (4, 1)), np.tile([hand.q0[7 * c + j] for c in range(4) for j in range(4)], (4, 1))
        assert np.array_equal(got["q"], np.where(got["blocked_step"] == 1, up, rest))


def test_host_path_refuses_bad_tables(hand):
    from a3vt_amd import ops
    v, f = gr.icosphere(1)
    args = lambda off, which: (torch.from_numpy(v), torch.from_numpy(f.astype(np.int32)), off, which, torch.zeros(1, 3),  # noqa: E731
                               torch.eye(3)[None], hand.table(), hand.q0)
    for off, which, steps in (([0, 90], [0], 4), ([5, 2], [0], 4), ([0, 80], [1], 4), ([0, 80], [0], 0)):
        with pytest.raises(ValueError, match="grasp_close"):
            ops.grasp_close(*args(off, which), steps)
    with pytest.raises(ValueError, match="hand_table"):
        ops.grasp_close(*args([0, 80], [0])[:6], hand.table()[:, :20], hand.q0, 4)


# ---- GraspFrames and save_simulation ----------------------------------------------------------------------------------------------
def two_objects():
    flat = (np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32) * 0.1 - np.float32(0.05), np.array([[0, 1, 2], [0, 2, 3]]))
    return {"ball": gr.icosphere(1, 0.08), "flat": flat}


def test_grasp_frames_feed_the_rendered_sampler(hand):
    from a3vt_amd.pterotactyl.policies.rendered import RenderedSampler
    from a3vt_amd.pterotactyl.simulator.physics.grasping import GraspFrames, KinematicGrasp
    geometry = two_objects()
    grasper = KinematicGrasp(hand, steps=2, device="cpu")
    calls = []
    table_of = grasper.grasp_table
    grasper.grasp_table = lambda *a, **k: calls.append(a[1]) or table_of(*a, **k)
    frames = GraspFrames(grasper, geometry)
    assert len(frames) == 100 and ("ball", 49) in frames and ("ball", 50) not in frames and ("cup", 0) not in frames
    pos, rot, present = frames[("ball", 3)]
    assert pos.shape == (4, 3) and rot.shape == (4, 3, 3) and present.all()
    assert not frames[("flat", 0)][2].any() and not frames[("flat", 0)][0].any()      # a coplanar object: no grasp, zeros
    frames[("ball", 4)]
    assert calls == [["ball"], ["flat"]]                                              # one table per object, on first touch
    full = grasper.grasp_table(geometry, ["ball", "flat"], 50, want_q=True, want_blocked_step=True, want_hand_pose=True)
    assert np.array_equal(full["pos"][0, 3], pos) and full["present"][0].all() and not full["present"][1].any()
    assert full["q"].shape == (2, 50, 16) and full["blocked_step"].max() <= 2 and full["hand_pose"][1][0] is None
    pose = full["hand_pose"][0][3]
    assert len(pose) == 28 and np.allclose(pose[6][0], pos[0], atol=1e-6)

    seen = []

    def render(verts, faces, face_offset, image_mesh, cam_pos, cam_rot, want_touch=True, want_points=True, **camera):
        seen.append((cam_pos.numpy().copy(), cam_rot.numpy().copy(), image_mesh.numpy().copy()))
        n = cam_pos.shape[0]
        return {"depth": torch.zeros(n, 121, 121), "status": torch.zeros(n, dtype=torch.int32), "touch": torch.zeros(n, 121, 121, 3)}
    sampler = RenderedSampler(frames, geometry=geometry, render=render)
    sampler.load_objects(["ball", "flat"])
    out = sampler.sample([3, 0])
    assert out["touch_status"][0] == ["no_touch"] * 4 and out["touch_status"][1] == ["no_intersection"] * 4
    cam_pos, cam_rot, mesh = seen[0]
    assert np.array_equal(cam_pos, pos) and np.array_equal(cam_rot, rot) and mesh.tolist() == [0] * 4
    assert np.array_equal(np.asarray(out["finger_transfrom_pos"])[0], pos)


def write_tree(root, geometry):
    os.makedirs(os.path.join(root, "object_info"))
    for name, (v, f) in geometry.items():
        np.save(os.path.join(root, "object_info", f"{name}_verts.npy"), v)
        np.save(os.path.join(root, "object_info", f"{name}_faces.npy"), f)


def test_save_simulation_on_the_host(hand, tmp_path):
    from a3vt_amd.pterotactyl.policies import recorded
    from a3vt_amd.pterotactyl.simulator.physics.grasping import KinematicGrasp
    from a3vt_amd.pterotactyl.utility import data_making
    root = str(tmp_path)
    geometry = two_objects()
    write_tree(root, geometry)
    counts = data_making.save_simulation(root, hand, batch=2, num_actions=50, steps=2, device="cpu", signals=False)
    assert counts == dict(written=2, skipped_existing=0, grasps=100, placed=50)
    table = KinematicGrasp(hand, steps=2, device="cpu").grasp_table(geometry, ["ball", "flat"], 50)
    for a in (0, 17, 49):
        pos, rot, present = recorded.tree_frames(root, "ball", a)
        assert present.all() and np.array_equal(pos, table["pos"][0, a]) and np.array_equal(rot, table["rot"][0, a])
        frames = recorded.tree_frames(root, "flat", a)                                # the directory exists, no finger has a file
        assert frames is not None and not frames[2].any()
    ref = np.load(os.path.join(root, "grasp_info", "ball", "0", "2_ref_frame.npy"), allow_pickle=True).item()
    assert set(ref) == {"pos", "rot"} and ref["pos"].shape == (3,) and ref["rot"].shape == (3, 3) and ref["pos"].dtype == np.float32
    assert not os.path.exists(os.path.join(root, "grasp_info", "ball", data_making.BAKING_MARKER))
    assert not [f for _, _, files in os.walk(root) for f in files if f.endswith(".tmp")]
    # never silently replaced: a frame changed by hand survives a second run, and "flat" (no frames) is done again
    target = os.path.join(root, "grasp_info", "ball", "0", "2_ref_frame.npy")
    np.save(target, np.array({"pos": np.ones(3, np.float32), "rot": np.eye(3, dtype=np.float32)}, dtype=object))
    counts = data_making.save_simulation(root, hand, batch=2, num_actions=50, steps=2, device="cpu", signals=False)
    assert counts["skipped_existing"] == 1 and counts["written"] == 1
    assert np.array_equal(np.load(target, allow_pickle=True).item()["pos"], np.ones(3, np.float32))
    # an interrupted run's marker: the object is written again
    with open(os.path.join(root, "grasp_info", "ball", data_making.BAKING_MARKER), "w"):
        pass
    stray = os.path.join(root, "grasp_info", "ball", "7", "9_ref_frame.npy")
    np.save(stray, np.array({"pos": np.ones(3, np.float32), "rot": np.eye(3, dtype=np.float32)}, dtype=object))
    counts = data_making.save_simulation(root, hand, batch=1, num_actions=50, steps=2, device="cpu", signals=False)
    assert counts["written"] == 2 and not os.path.exists(stray)
    assert np.array_equal(np.load(target, allow_pickle=True).item()["pos"], table["pos"][0, 0, 2])
    assert not os.path.exists(os.path.join(root, "grasp_info", "ball", data_making.BAKING_MARKER))
    # overwrite replaces
    np.save(target, np.array({"pos": np.ones(3, np.float32), "rot": np.eye(3, dtype=np.float32)}, dtype=object))
    counts = data_making.save_simulation(root, hand, batch=2, num_actions=50, steps=2, device="cpu", signals=False, overwrite=True)
    assert counts["written"] == 2 and np.array_equal(np.load(target, allow_pickle=True).item()["pos"], table["pos"][0, 0, 2])
