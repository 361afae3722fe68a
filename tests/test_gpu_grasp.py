"""``a3vt_grasp_close`` (csrc/grasp_close.hip) on the GPU against ``grasp_ref``, the tests' loop-by-loop float64 statement of the
closing rule, and the layers above it (``KinematicGrasp``, ``GraspFrames``, ``data_making.save_simulation``).

**The rule is a kinematic stand-in for pybullet's five ``stepSimulation`` calls; nothing here compares a frame with pybullet's.**

Decided cases.  ``grasp_ref`` also returns every query's signed separation.  A (grasp, finger) is *decided* when every query on its
path has |separation| >= 1e-5 m: float32 on coordinates <= 0.5 m through <= 6 chained transforms errs by about 2e-7 m, which leaves a
50 x margin.  On decided pairs ``blocked_step`` equals the reference's integer for integer and ``q`` lies within 1e-6 of it (one
multiply and one add in float32 at |q| <= 1.8).  Every test asserts that at most 10 % of its pairs are undecided; the meshes, scales
and actions below were chosen on the CPU so that the float64 reference alone shows that.

Link poses and frames are compared with ``HandModel.forward`` in float64 on the kernel's own ``q``.  The tolerance is not fixed in
advance: it is 8 x the error that a float32 NumPy emulation of the same chain (``fk32`` below) shows against float64 on the same
angles, case by case.  Measured on an MI355X over the cases of this file: emulation 3.0e-8 m (positions) and 1.3e-7 (rotation
entries) at most, kernel 2.8e-8 m and 1.6e-7 at most (the smallest case: emulation 5.3e-9 m / 6.1e-8, kernel 5.3e-9 m / 6.8e-8);
``q`` on decided pairs within 5.3e-8 of the reference; undecided pairs 3 of 200 in the 50-action case, none elsewhere.

Shapes: a single triangle; two meshes of 320 and 12 faces behind ``grasp_mesh``; all 50 actions on an icosphere-3 (1280 faces, 5
chunks of the cull) and 10 of them on the same sphere without its last three faces (1277: the last chunk is partial and F is no
multiple of 64); an icosphere-5 whose in-reach faces exceed the LDS capacity, against the same mesh cut to the faces that ever come
within 1 mm of a box; a mesh out of reach; a mesh overlapping a link at the rest pose; ``steps`` 1 and 64."""
import functools
import os

import numpy as np
import pytest
import torch

import grasp_ref as gr

pytestmark = pytest.mark.gpu
UNDECIDED_CAP = 0.10
Q_TOL = 1e-6


def dev(a, dtype, cuda):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(cuda)


def run_kernel(cuda, case, steps=None, rows=None):
    from a3vt_amd import ops
    hand = gr.hand()
    pick = slice(None) if rows is None else rows
    out = ops.grasp_close(dev(case["verts"], np.float32, cuda), dev(case["faces"], np.int32, cuda), case["offsets"],
                          list(np.asarray(case["which"])[pick]), dev(case["base_pos"][pick], np.float32, cuda),
                          dev(case["base_rot"][pick], np.float32, cuda), hand.table(), hand.q0, case["steps"] if steps is None else steps)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def make_case(meshes, which, base_pos, base_rot, steps, track_near=False):
    verts, faces, offsets = gr.batch(meshes)
    near = set() if track_near else None
    q, blocked, margin, link_pos, link_rot = gr.close(verts, faces, offsets, which, base_pos, base_rot, gr.hand(), steps, near)
    return dict(verts=verts, faces=faces, offsets=offsets, which=list(which), base_pos=base_pos, base_rot=base_rot, steps=steps, q=q,
                blocked=blocked, margin=margin, near=near)


def placed_case(meshes, picks, steps, **kw):
    which, base_pos, base_rot = gr.placements(meshes, picks)
    assert len(which) == len(picks)
    return make_case(meshes, which, base_pos, base_rot, steps, **kw)


TILT = np.array([[0.96, -0.28, 0.0], [0.28, 0.96, 0.0], [0.0, 0.0, 1.0]], np.float32)     # a rotation with exact float32 entries


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs and the float64 reference of one named case, computed once per session and never changed."""
    hand = gr.hand()
    if name == "single":                 # G = 1, F = 1: one triangle in the path of finger 1's first joint
        pos = np.array([[0.01, -0.02, 0.03]], np.float32)
        return make_case([gr.blocking_triangle(hand, 1, 0.4, pos[0], TILT)], [0], pos, TILT[None], 64)
    if name in ("two", "two_s1"):        # G = 3, M = 2: grasp_mesh indirection
        return placed_case([gr.icosphere(2, 0.08), gr.box_mesh()], [(0, 9), (1, 6), (0, 30)], 64 if name == "two" else 1)
    if name == "all50":                  # every action of an icosphere-3
        return placed_case([gr.icosphere(3, 0.07, (1.0, 0.8, 1.2))], [(0, a) for a in range(50)], 16)
    if name == "ragged":                 # the same sphere without its last 3 faces: F = 1277
        v, f = gr.icosphere(3, 0.07, (1.0, 0.8, 1.2))
        return placed_case([(v, f[:-3])], [(0, a) for a in range(0, 50, 5)], 16)
    if name == "overflow":               # in-reach faces above the LDS capacity
        return placed_case([gr.icosphere(5, 0.10, (1.0, 0.9, 1.1))], [(0, 17)], 16, track_near=True)
    if name == "far":                    # G = 2, every face out of reach
        v, f = gr.icosphere(2, 0.08, centre=(1.0, 1.0, 1.0))
        pos = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, -0.1]], np.float32)
        return make_case([(v, f)], [0, 0], pos, np.stack([np.eye(3, dtype=np.float32), TILT]), 8)
    if name == "rest_overlap":           # a triangle through link 1 of finger 0 at the rest pose
        pos, rot = gr.chain_poses(hand, 0, np.zeros(3), np.eye(3), hand.q0[:7])
        centre = pos[1] + rot[1] @ hand.box_centre[1]
        tri = (centre + np.array([[0.03, 0.001, 0.0], [-0.03, 0.002, 0.004], [0.0, -0.001, -0.005]])).astype(np.float32)
        return make_case([(tri, np.array([[0, 1, 2]]))], [0], np.zeros((1, 3), np.float32), np.eye(3, dtype=np.float32)[None], 16)
    raise KeyError(name)


def fk32(hand, base_pos, base_rot, q16):
    """The kernel's chain arithmetic in float32 NumPy (every product and sum rounded to float32) -> (28, 3), (28, 3, 3)."""
    f32 = np.float32
    pos, rot = np.zeros((28, 3), f32), np.zeros((28, 3, 3), f32)
    table = hand.table()
    for i in range(28):
        c, k = divmod(i, 7)
        parent = int(hand.parent[i])
        p, R = (base_pos.astype(f32), base_rot.astype(f32)) if parent < 0 else (pos[parent], rot[parent])
        pos[i] = p + R @ table[i, 2:5].astype(f32)
        rot[i] = R @ table[i, 5:14].astype(f32).reshape(3, 3)
        if hand.revolute[i]:
            x, y, z = table[i, 14:17].astype(f32)
            a = f32(q16[4 * c + k])
            s, co = np.sin(a, dtype=f32), np.cos(a, dtype=f32)
            t = f32(1) - co
            turn = np.array([[t * x * x + co, t * x * y - s * z, t * x * z + s * y], [t * x * y + s * z, t * y * y + co, t * y * z - s * x],
                             [t * x * z - s * y, t * y * z + s * x, t * z * z + co]], f32)
            rot[i] = rot[i] @ turn
    return pos, rot


def full_angles(hand, q16):
    q = np.array(hand.q0, np.float64)
    for c in range(4):
        q[7 * c:7 * c + 4] = q16[4 * c:4 * c + 4]
    return q


def check_against_reference(name, got, ref):
    decided = ref["margin"] >= gr.DECIDED                                    # (G, 4)
    share = 1.0 - decided.mean()
    print(f"{name}: G={len(ref['which'])} undecided {int((~decided).sum())}/{decided.size}")
    assert share <= UNDECIDED_CAP, (name, share)
    mask = np.repeat(decided, 4, axis=1)
    assert np.array_equal(got["blocked_step"][mask], ref["blocked"][mask]), name
    err = np.abs(got["q"].astype(np.float64) - ref["q"])[mask].max()
    print(f"{name}: max |q - reference| on decided pairs {err:.3g}")
    assert err <= Q_TOL, (name, err)


def check_poses(name, got, ref):
    """Link poses and frames against float64 forward kinematics on the kernel's own angles; tolerance 8 x the float32 emulation's."""
    hand = gr.hand()
    worst = dict(emu_pos=0.0, emu_rot=0.0, ker_pos=0.0, ker_rot=0.0)
    for g in range(len(ref["which"])):
        q = full_angles(hand, got["q"][g].astype(np.float64))
        pos64, rot64 = hand.forward(ref["base_pos"][g], ref["base_rot"][g], q)
        pos32, rot32 = fk32(hand, ref["base_pos"][g], ref["base_rot"][g], got["q"][g])
        worst["emu_pos"] = max(worst["emu_pos"], np.abs(pos32 - pos64).max())
        worst["emu_rot"] = max(worst["emu_rot"], np.abs(rot32 - rot64).max())
        worst["ker_pos"] = max(worst["ker_pos"], np.abs(got["link_pos"][g] - pos64).max())
        worst["ker_rot"] = max(worst["ker_rot"], np.abs(got["link_rot"][g] - rot64).max())
        assert np.array_equal(got["frame_pos"][g], got["link_pos"][g][[6, 13, 20, 27]]), name
        assert np.array_equal(got["frame_rot"][g], got["link_rot"][g][[6, 13, 20, 27]]), name
    print(f"{name}: float32 emulation vs float64: pos {worst['emu_pos']:.3g} rot {worst['emu_rot']:.3g}; kernel: pos "
          f"{worst['ker_pos']:.3g} rot {worst['ker_rot']:.3g}")
    assert worst["ker_pos"] <= 8 * worst["emu_pos"] and worst["ker_rot"] <= 8 * worst["emu_rot"], (name, worst)


@pytest.mark.parametrize("name", ["single", "two", "two_s1", "all50", "ragged", "far", "rest_overlap"])
def test_kernel_against_reference(cuda, name):
    ref = case(name)
    got = run_kernel(cuda, ref)
    check_against_reference(name, got, ref)
    check_poses(name, got, ref)
    if name == "single":                 # finger 1 stops part of the way; no other finger is touched
        assert (0 < ref["blocked"][0, 5:8]).all() and (ref["blocked"][0, 5:8] < 64).all() and (np.delete(ref["blocked"][0], [5, 6, 7]) == 64).all()
    if name == "far":
        upper = np.array([gr.hand().upper[7 * c + j] for c in range(4) for j in range(4)], np.float32)
        assert (got["blocked_step"] == 8).all() and np.array_equal(got["q"], np.tile(upper, (2, 1)))
    if name == "rest_overlap":           # joints 0 and 1 of finger 0 test link 1's box: neither moves; no other finger is touched
        assert (got["blocked_step"][0, :2] == 0).all() and (got["blocked_step"][0, 2:4] > 0).all() and (got["blocked_step"][0, 4:] == 16).all()
    if name == "two_s1":
        assert set(np.unique(got["blocked_step"])) <= {0, 1}


def test_more_candidates_than_the_lds_holds(cuda):
    """An icosphere-5 whose in-reach faces exceed the capacity (asserted from the host): the reference, and the same mesh cut to the
    faces that ever come within 1 mm of a box on the reference's path, which fits LDS and must give the same bytes."""
    from a3vt_amd import ops
    ref = case("overflow")
    hand = gr.hand()
    capacity = ops.grasp_limits()["capacity"]
    counts = ops.grasp_candidates(ref["verts"], ref["faces"], ref["offsets"], ref["which"], ref["base_pos"], ref["base_rot"], hand.table())
    print("overflow: candidates per finger", counts[0], "capacity", capacity)
    assert counts.min() > capacity + 256
    got = run_kernel(cuda, ref)
    check_against_reference("overflow", got, ref)
    check_poses("overflow", got, ref)
    keep = np.array(sorted(ref["near"]))
    cut = dict(ref, faces=ref["faces"][keep], offsets=[0, len(keep)])
    cut_counts = ops.grasp_candidates(cut["verts"], cut["faces"], cut["offsets"], cut["which"], cut["base_pos"], cut["base_rot"], hand.table())
    assert 0 < cut_counts.max() < capacity - 256
    small = run_kernel(cuda, cut)
    for key in got:
        assert got[key].tobytes() == small[key].tobytes(), key


def test_repeatable_and_batch_invariant(cuda):
    ref = case("all50")
    first, second = run_kernel(cuda, ref), run_kernel(cuda, ref)
    for key in first:
        assert first[key].tobytes() == second[key].tobytes(), key
    for g in (0, 17, 49):
        alone = run_kernel(cuda, ref, rows=slice(g, g + 1))
        for key in first:
            assert alone[key][0].tobytes() == first[key][g].tobytes(), (key, g)


def test_more_grasps_than_one_launch_takes(cuda):
    """70 grasps: two launches, the second one's rows against the same grasps alone."""
    from a3vt_amd import ops
    ref = case("all50")
    per_launch = ops.grasp_limits()["per_launch"]
    rows = np.arange(per_launch + 6) % 50
    ops.grasp_launches(reset=True)
    many = run_kernel(cuda, ref, rows=rows)
    assert ops.grasp_launches() == {"calls": 1, "launches": 2}
    base = run_kernel(cuda, ref)
    for key in many:
        assert many[key].tobytes() == base[key][rows].tobytes(), key


def test_no_grasp_launches_nothing(cuda):
    from a3vt_amd import ops
    ref = case("two")
    ops.grasp_launches(reset=True)
    out = run_kernel(cuda, ref, rows=slice(0, 0))
    assert ops.grasp_launches() == {"calls": 0, "launches": 0}
    assert out["q"].shape == (0, 16) and out["frame_rot"].shape == (0, 4, 3, 3)


def two_objects():
    return {"ball": gr.icosphere(2, 0.08), "brick": gr.box_mesh()}


def test_grasp_table_is_one_call_and_serves_the_sampler(cuda):
    """``grasp_table`` of two objects: one ``a3vt_grasp_close`` call; and ``RenderedSampler`` with ``GraspFrames`` gives, at E = 2 and
    A = 50, the table it gives for the same frames as a plain dict, bit for bit."""
    from a3vt_amd import ops
    from a3vt_amd.pterotactyl.policies.rendered import RenderedSampler
    from a3vt_amd.pterotactyl.simulator.physics.grasping import GraspFrames, KinematicGrasp
    geometry = two_objects()
    grasper = KinematicGrasp(gr.hand(), steps=16, device=cuda)
    ops.grasp_launches(reset=True)
    table = grasper.grasp_table(geometry, ["ball", "brick"], 50)
    assert ops.grasp_launches()["calls"] == 1
    assert table["pos"].shape == (2, 50, 4, 3) and table["present"].all(axis=2).sum() == table["present"].any(axis=2).sum() > 0
    frames = GraspFrames(grasper, geometry)
    plain = {(obj, a): (table["pos"][e, a], table["rot"][e, a], table["present"][e, a]) for e, obj in enumerate(("ball", "brick"))
             for a in range(50)}
    results = []
    for source in (frames, plain):
        sampler = RenderedSampler(source, geometry=geometry, device=cuda)
        sampler.load_objects(["ball", "brick"])
        results.append(sampler.sample_table(50))
    assert set(results[0]) == set(results[1])
    for key, value in results[0].items():
        other = results[1][key]
        if isinstance(value, torch.Tensor):
            assert value.cpu().numpy().tobytes() == other.cpu().numpy().tobytes(), key
        else:
            assert np.array_equal(np.asarray(value), np.asarray(other)), key
    assert (results[0]["touch_code"] == 2).any()


def test_save_simulation_leaves_a_tree_the_touch_bake_accepts(cuda, tmp_path):
    from a3vt_amd.pterotactyl.policies import recorded
    from a3vt_amd.pterotactyl.utility import data_making
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "object_info"))
    for name, (v, f) in two_objects().items():
        np.save(os.path.join(root, "object_info", f"{name}_verts.npy"), v)
        np.save(os.path.join(root, "object_info", f"{name}_faces.npy"), f)
    counts = data_making.save_simulation(root, gr.hand(), batch=2, num_actions=50, steps=16, device=cuda)
    assert counts["written"] == 2 and counts["grasps"] == 100 and counts["placed"] > 0
    assert counts["images"]["written"] == 2 and counts["touch"]["written"] == 2 and counts["touch"]["touch"] > 0
    frames = recorded.tree_frames(root, "ball", 0)
    assert frames is not None and frames[2].all()
    again = data_making.save_touch_signals(root, batch=2, num_actions=50, device=cuda)
    assert again["skipped_existing"] == 2 and again["written"] == 0
    assert not os.path.exists(os.path.join(root, "grasp_info", "ball", data_making.BAKING_MARKER))
