"""``a3vt_scene_render_posed`` and ``a3vt_pose_parts`` (csrc/posed_render.hip) on the GPU, and ``RenderedSampler``'s
``vision_occluded`` built on them.

The main check is BIT EQUALITY with the existing kernel: ``ops.scene_render_posed`` against ``ops.scene_render`` on
``ops.pose_parts``' output — ``rgb`` equal, ``depth`` equal as uint32, (``prim_inst``, ``prim_face``) equal to ``prim`` under the
materialised numbering, on every pixel.  The cull of a posed instance never shows in that comparison unless it drops something
the materialised form sees, so it also proves the cull conservative (the scaled pose included).  Two views go through the fp64
yardstick of ``scene_render_util`` as well (``posed_render_util.yard_view``), with the posed triangles formed in float64 on the host.

Measured on an MI355X: every bit-equality case holds on every pixel; against fp64 (depth: the float32 emulation's largest relative
deviation, then the kernel's; undecided pixels): synthetic 7.7e-7, 2.1e-7 (0 of 960), golden 2.9e-7, 2.1e-7 (0 of 960), no colour
level off, no hit and no prim differs; the box scaled by 3 covers 782 pixels against 69 unscaled; the file takes 5 s."""
import numpy as np
import pytest
import torch

import posed_render_util as pu
import scene_render_util as su

pytestmark = pytest.mark.gpu
CAMERA = dict(znear=su.ZNEAR, zfar=su.ZFAR, lights=su.LIGHTS, ambient=su.AMBIENT, background=su.BACKGROUND)


@pytest.fixture(scope="module")
def ops(cuda):
    from a3vt_amd import ops
    return ops


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def cameras(n, pos, rot):
    pos = np.tile(su.NARROW_POS, (n, 1)) if pos is None else np.broadcast_to(np.asarray(pos, np.float64), (n, 3))
    rot = np.tile(su.CAM_ROT, (n, 1, 1)) if rot is None else np.broadcast_to(np.asarray(rot, np.float64), (n, 3, 3))
    return dev(pos, np.float32), dev(rot, np.float32)


def instances(t):
    return [dev(t["inst_part"], np.int32), dev(t["inst_pos"], np.float32), dev(t["inst_rot"], np.float32), dev(t["inst_rgb"], np.uint8)]


def posed(ops, parts, images, W=su.COUNT_SIZE[0], H=su.COUNT_SIZE[1], pos=None, rot=None, yfov=su.NARROW_YFOV, scene=CAMERA, table=None):
    """``ops.scene_render_posed`` on a list of images -> the dict as NumPy arrays (the NARROW camera unless given)."""
    table = ops.PartTable(parts) if table is None else table
    t = pu.tables(images)
    out = ops.scene_render_posed(table, *instances(t), t["inst_offset"], *cameras(len(images), pos, rot), yfov=yfov, width=W, height=H, **scene)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def materialised(ops, parts, images, W=su.COUNT_SIZE[0], H=su.COUNT_SIZE[1], pos=None, rot=None, yfov=su.NARROW_YFOV, scene=CAMERA):
    """The same images through ``ops.pose_parts`` and the EXISTING ``ops.scene_render`` -> its dict, and ``pose_parts``' tables."""
    table = ops.PartTable(parts)
    t = pu.tables(images)
    m = ops.pose_parts(table, *instances(t), inst_offset=t["inst_offset"])
    n = len(images)
    none = torch.zeros((0, 3), device="cuda")
    out = ops.scene_render(m["verts"], m["faces"], m["face_rgb"], none, torch.zeros(0, device="cuda"), none.to(torch.uint8), m["face_offset"],
                           [0] * (n + 1), list(range(n)), *cameras(n, pos, rot), yfov=yfov, width=W, height=H, **scene)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, m, table, t


def both(ops, parts, images, **kw):
    """Render both ways, assert the bits equal on every pixel, return the posed result."""
    got = posed(ops, parts, images, **kw)
    want, m, table, t = materialised(ops, parts, images, **kw)
    prim = pu.materialised_index(table.face_offset, t["inst_part"], m["face_base"], got["prim_inst"], got["prim_face"])
    assert np.array_equal(got["rgb"], want["rgb"])
    assert np.array_equal(bits(got["depth"]), bits(want["depth"]))
    assert np.array_equal(prim, want["prim"])
    assert np.array_equal(got["prim_inst"] < 0, got["prim_face"] < 0) and np.array_equal(got["prim_inst"] < 0, got["depth"] == 0)
    return got


TILT = pu.rotation((0.1, -0.05, 0.7))


# ---- bit equality with scene_render on the materialised triangles ---------------------------------------------------------------
def test_part_sizes(ops):
    """Parts of 1, 255, 256, 257 and 513 faces (the face chunk's edges), one image each, every fan filling its image under a tilt and
    a shift; a sixth part that no instance uses."""
    parts = [pu.fan(n) for n in su.FACE_COUNTS] + [pu.tetra()]
    images = [[(k, (0.002 * k, -0.001, 0.003), TILT if k % 2 else pu.QUARTER, su.PALETTE[k])] for k in range(len(su.FACE_COUNTS))]
    got = both(ops, parts, images)
    assert (got["depth"] > 0).all()                                          # watertight: no ray leaks through a shared edge
    for k in range(len(images)):
        assert (got["prim_inst"][k] == k).all()
        lo, hi = np.cumsum([0] + [len(f) for _, f in parts])[k:k + 2]
        assert got["prim_face"][k].min() >= lo and got["prim_face"][k].max() < hi
    assert len(np.unique(got["prim_face"][4])) > 20


def test_instance_counts(ops):
    """0, 1, 21, 257 and 513 instances in an image (the instance chunk's edges), 40 x 24 (partial tiles): five images of one call
    that share one part under different poses."""
    parts = [pu.tetra(), pu.box()]
    images = [pu.scatter(n, seed=10 + n) for n in (0, 1, 21, 257, 513)]
    got = both(ops, parts, images, W=40, H=24)
    assert (got["prim_inst"][0] == -1).all() and (got["rgb"][0] == 255).all()
    assert (got["prim_inst"][1] >= 0).any()
    seen = np.unique(got["prim_inst"][4])
    assert seen.max() >= 1 + 21 + 257 + 256 and len(seen) > 50              # instances of the third chunk are seen, by global index
    assert ((got["prim_inst"][3] >= 22) | (got["prim_inst"][3] < 0)).all() and got["prim_inst"][3].max() < 22 + 257


def test_culled_empty_behind_and_straddling(ops):
    parts = [pu.box((0.02, 0.02, 0.02)), pu.tetra()]
    aside = [(1, p + np.array([5.0, 0, 0]), r, c) for _, p, r, c in pu.scatter(30)]          # all culled: far outside every pyramid
    behind = [(0, su.NARROW_POS - pu.FORWARD * 1.0, pu.GENERIC, su.PALETTE[1])] + pu.scatter(4, part=1)
    straddle = [(0, su.NARROW_POS + pu.FORWARD * su.ZNEAR, pu.EYE, su.PALETTE[2])]          # the box holds the camera and znear's plane
    got = both(ops, parts, [aside, [], behind, straddle])
    for k in (0, 1):
        assert (got["prim_inst"][k] == -1).all() and not got["depth"][k].any() and (got["rgb"][k] == 255).all()
    first = len(aside)
    assert not (got["prim_inst"][2] == first).any() and (got["prim_inst"][2] > first).any()    # the box behind the camera is not seen
    assert (got["prim_inst"][3] == first + 5).all() and (got["depth"][3] >= su.ZNEAR).all()    # its far side is, beyond znear


@pytest.mark.parametrize("W,H", [(1, 1), (17, 16), (16, 33)])
def test_partial_tiles(ops, W, H):
    got = both(ops, [pu.tetra(0.02), pu.fan(257)], [pu.scatter(21, spread=0.02), [(1, (0, 0, 0), TILT, su.PALETTE[3])]], W=W, H=H)
    assert (got["depth"][1] > 0).all() and got["rgb"].shape == (2, H, W, 3)


def test_two_launches(ops):
    """I = 129 images at 16 x 16: the 129th goes in a second launch, with its own instance range."""
    parts = [pu.tetra(0.01)]
    images = [pu.scatter(3, seed=i, spread=0.02) for i in range(129)]
    ops.posed_launches(reset=True)
    got = posed(ops, parts, images, W=16, H=16)
    assert ops.posed_launches() == {"calls": 1, "kernels": 2, "pose_parts": 0}
    want, m, table, t = materialised(ops, parts, images, W=16, H=16)
    assert np.array_equal(got["rgb"], want["rgb"]) and np.array_equal(bits(got["depth"]), bits(want["depth"]))
    last = got["prim_inst"][128]
    assert (last >= 0).any() and last[last >= 0].min() >= 3 * 128
    alone = posed(ops, parts, images[128:], W=16, H=16)
    assert np.array_equal(alone["rgb"][0], got["rgb"][128]) and np.array_equal(bits(alone["depth"][0]), bits(got["depth"][128]))


def test_rotations_and_a_scale(ops):
    """A quarter turn, a generic rotation and a pose that scales by 3: R is used as given.  The scaled box covers nine times the
    pixels, so a cull that bounded it by the unscaled part would lose hits that the materialised form has."""
    parts = [pu.box(), pu.tetra()]
    at = np.array([0.004, -0.002, 0.0])
    images = [[(0, at, R, su.PALETTE[1])] + pu.scatter(6, part=1, seed=8) for R in (pu.QUARTER, pu.GENERIC, 3.0 * pu.GENERIC)]
    got = both(ops, parts, images)
    hits = [(got["prim_inst"][k] == 7 * k).sum() for k in range(3)]
    print("pixels of the box under a quarter turn, a generic rotation, the same scaled by 3:", hits)
    assert hits[1] > 20 and hits[2] > 6 * hits[1]


def test_coincident_instances(ops):
    """Two instances of one part under one pose: equal depths everywhere, and the lower instance is seen — whichever colour it has."""
    parts = [pu.ico(2, 0.03)]
    pose = ((0.003, 0.001, 0.0), pu.GENERIC)
    for colours in ((su.PALETTE[1], su.PALETTE[2]), (su.PALETTE[2], su.PALETTE[1])):
        got = both(ops, parts, [[(0, *pose, colours[0]), (0, *pose, colours[1])]])
        hit = got["prim_inst"][0] >= 0
        assert hit.any() and (got["prim_inst"][0][hit] == 0).all()
        alone = posed(ops, parts, [[(0, *pose, colours[0])]])
        assert all(np.array_equal(bits(alone[k]), bits(got[k])) for k in got)


def test_identity_pose_is_scene_render_on_the_stored_mesh(ops):
    scene = su.ico(3, 0.03, face_rgb=su.PALETTE[0])
    got = posed(ops, [(scene["verts"], scene["faces"])], [[(0, np.zeros(3), pu.EYE, su.PALETTE[0])]])
    t = su.pack([scene])
    want = ops.scene_render(dev(t["verts"], np.float32), dev(t["faces"], np.int32), dev(t["face_rgb"], np.uint8), dev(t["centres"], np.float32),
                            dev(t["radii"], np.float32), dev(t["sphere_rgb"], np.uint8), t["face_offset"], t["sphere_offset"], [0],
                            *cameras(1, None, None), yfov=su.NARROW_YFOV, width=su.COUNT_SIZE[0], height=su.COUNT_SIZE[1], **CAMERA)
    want = {k: v.cpu().numpy() for k, v in want.items()}
    assert np.array_equal(got["rgb"], want["rgb"]) and np.array_equal(bits(got["depth"]), bits(want["depth"]))
    assert np.array_equal(got["prim_face"], want["prim"]) and (got["prim_face"] >= 0).sum() > 500


# ---- bad inputs -------------------------------------------------------------------------------------------------------------------
def test_bad_instances_are_skipped(ops):
    """An out-of-range part id, a NaN or infinite pose: the image is the one without that instance, bit for bit."""
    parts = [pu.tetra(0.012), pu.box()]
    good = pu.scatter(6, seed=4, spread=0.02)
    want = posed(ops, parts, [good])
    nan_rot = pu.GENERIC.copy()
    nan_rot[1, 2] = np.nan
    for bad in ((2, (0, 0, 0.01), pu.EYE, (1, 2, 3)), (-1, (0, 0, 0.01), pu.EYE, (1, 2, 3)), (1, (0, np.nan, 0.01), pu.EYE, (1, 2, 3)),
                (1, (0, 0, 0.01), nan_rot, (1, 2, 3)), (1, (np.inf, 0, 0.01), pu.EYE, (1, 2, 3)), (1, (0, 0, 0.01), np.full((3, 3), np.inf), (1, 2, 3))):
        images = [good[:2] + [bad] + good[2:]]
        got = posed(ops, parts, images)
        assert np.array_equal(got["rgb"], want["rgb"]) and np.array_equal(bits(got["depth"]), bits(want["depth"])), bad
        shifted = np.where(want["prim_inst"] >= 2, want["prim_inst"] + 1, want["prim_inst"])
        assert np.array_equal(got["prim_inst"], shifted) and np.array_equal(got["prim_face"], want["prim_face"]), bad
        if bad[0] == 1:                                                      # (pose_parts sizes its output by the part: ids it knows)
            both(ops, parts, images)


def test_a_nan_template_vertex_drops_its_faces_only(ops):
    v, f = pu.tetra(0.02)
    broken = v.copy()
    broken[3] = np.nan
    rest = [(1, (0.01, 0.0, -0.02), pu.GENERIC, su.PALETTE[4])]
    got = both(ops, [(broken, f), pu.box()], [[(0, (0, 0, 0), TILT, su.PALETTE[1])] + rest])
    want = posed(ops, [(v, f[:1]), pu.box()], [[(0, (0, 0, 0), TILT, su.PALETTE[1])] + rest])         # face 0 is the one without vertex 3
    assert np.array_equal(got["rgb"], want["rgb"]) and np.array_equal(bits(got["depth"]), bits(want["depth"]))
    assert np.array_equal(got["prim_inst"], want["prim_inst"]) and (got["prim_inst"] == 0).any()
    assert (got["prim_face"][got["prim_inst"] == 0] == 0).all()


# ---- batch invariance and repeatability -------------------------------------------------------------------------------------------
def test_batch_invariance_and_repeatability(ops):
    parts = [pu.tetra(0.008), pu.box(), pu.ico(1, 0.02)]
    image = [(2, np.zeros(3), pu.EYE, su.PALETTE[0])] + pu.scatter(21, part=0, seed=2) + pu.scatter(5, part=1, seed=6)
    others = [pu.scatter(n, part=n % 2, seed=n) for n in (300, 2, 0, 40)]
    alone = posed(ops, parts, [image], W=40, H=24)
    batch = posed(ops, parts, others[:3] + [image] + others[3:], W=40, H=24)
    again = posed(ops, parts, others[:3] + [image] + others[3:], W=40, H=24)
    first = sum(len(o) for o in others[:3])
    assert np.array_equal(alone["rgb"][0], batch["rgb"][3]) and np.array_equal(bits(alone["depth"][0]), bits(batch["depth"][3]))
    assert np.array_equal(np.where(alone["prim_inst"][0] < 0, -1, alone["prim_inst"][0] + first), batch["prim_inst"][3])
    assert np.array_equal(alone["prim_face"][0], batch["prim_face"][3])
    assert all(np.array_equal(bits(batch[k]), bits(again[k])) for k in batch)
    assert (alone["prim_inst"] >= 0).sum() > 100


# ---- against the fp64 yardstick ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["synthetic", "golden"])
def test_against_fp64(ops, name):
    """A posed synthetic hand in front of an icosphere-2, and the golden hand at a grasp of the kinematic rule, 40 x 24: the posed
    triangles formed in float64 on the host, ``scene_render_ref.render_image``, ``scene_render_util.check``'s protocol (undecided
    pixels at most 0.1 %, depth within 8 x the float32 emulation's own error, colour within one level, no hit or prim differs)."""
    parts, image, pos, rot, yfov, scene, owner, want = pu.yard_view(name)
    W, H = pu.YARD_SIZE
    got = posed(ops, parts, [image], W=W, H=H, pos=pos, rot=rot, yfov=yfov, scene=pu.vision_scene())
    t = pu.tables([image])
    face_base = np.cumsum([0] + [len(parts[p][1]) for p in t["inst_part"]])
    face_offset = np.cumsum([0] + [len(f) for _, f in parts])
    prim = pu.materialised_index(face_offset, t["inst_part"], face_base, got["prim_inst"][0], got["prim_face"][0])
    su.check(dict(rgb=got["rgb"][0], depth=got["depth"][0], prim=prim), want, f"posed {name}")
    assert len(np.unique(got["prim_inst"][0])) > 5


def test_pose_parts_against_float64(ops):
    """``pose_parts``' vertices against the float64 product of the same float32 inputs, on the golden hand at a grasp.  The
    yardstick is the same route in float32 NumPy (``v @ R.T + p``, every product and sum rounded); the fma chain may err 4 x that,
    as the grasp tests allow their chains.  Measured on an MI355X (largest absolute error over the 4 298 vertices; the coordinates
    are below 0.5 m): float32 NumPy 1.091e-08 m, pose_parts 2.063e-08 m; the NumPy form of the rule and the device differ in 0 of
    the 12 894 coordinates."""
    parts, image, *_ = pu.yard_view("golden")
    t = pu.tables([image])
    m = ops.pose_parts(ops.PartTable(parts), *instances(t))
    got = m["verts"].cpu().numpy().astype(np.float64)
    exact, single = [], []
    for part, pos, rot in zip(t["inst_part"], t["inst_pos"], t["inst_rot"]):
        v = np.asarray(parts[part][0], np.float32)
        exact.append(v.astype(np.float64) @ rot.astype(np.float64).T + pos.astype(np.float64))
        single.append((v @ rot.T + pos).astype(np.float64))
    exact, single = np.concatenate(exact), np.concatenate(single)
    yard, err = np.abs(single - exact).max(), np.abs(got - exact).max()
    print(f"pose_parts against float64: float32 NumPy {yard:.3e}, the kernel {err:.3e} ({len(exact)} vertices)")
    assert got.shape == exact.shape and yard > 0 and err <= 4 * yard
    # and the NumPy form of the rule (float64 product and sum, rounded once) differs from the device by double rounding at most
    host = ops.pose_parts(ops.PartTable(parts, device="cpu"), *(torch.from_numpy(t[k]) for k in ("inst_part", "inst_pos", "inst_rot", "inst_rgb")))
    apart = np.abs(host["verts"].numpy().astype(np.float64) - got)
    print(f"pose_parts, NumPy form against the device: {int((apart > 0).sum())} of {apart.size} coordinates differ, at most {apart.max():.3e}")
    # (three fused multiply-adds, each apart by at most one ulp of a value below 0.5, carried on through factors of at most 1)
    assert apart.max() <= 3 * 2.0 ** -25 and np.array_equal(host["faces"].numpy(), m["faces"].cpu().numpy())
    assert np.array_equal(host["face_rgb"].numpy(), m["face_rgb"].cpu().numpy())


# ---- the sampler ----------------------------------------------------------------------------------------------------------------
SIZE = [40, 24]


@pytest.fixture(scope="module")
def sampler(ops):
    """``RenderedSampler`` over ``GraspFrames`` over a ``KinematicGrasp`` on the golden hand (on the GPU), an icosphere and a single
    triangle — no hull, so none of its grasps can be placed."""
    from a3vt_amd.pterotactyl.policies.rendered import RenderedSampler
    from a3vt_amd.pterotactyl.simulator.physics.grasping import GraspFrames, KinematicGrasp
    hand, visual = pu.golden_hand()
    geometry = dict(pu.grasp_geometry(), flat=(np.array([[-0.05, -0.04, 0], [0.05, -0.04, 0.01], [0, 0.06, 0]], np.float32), np.array([[0, 1, 2]])))
    frames = GraspFrames(KinematicGrasp(hand, steps=16), geometry, num_actions=50)
    s = RenderedSampler(frames, geometry, hand_visual=visual, resolution=SIZE)
    s.load_objects([pu.GRASP_OBJECT, "flat"])
    return s


def test_sampler_occluded(ops, sampler):
    out = sampler.sample([pu.GRASP_ACTION, 3], touch=False, vision=True, vision_occluded=True)
    occluded, vision = out["vision_occluded"], out["vision"]
    assert len(occluded) == 2 and all(im.shape == (SIZE[1], SIZE[0], 3) and im.dtype == np.uint8 for im in occluded)
    assert sampler.frames.hand_links(pu.GRASP_OBJECT, pu.GRASP_ACTION) is not None and sampler.frames.hand_links("flat", 3) is None
    assert not np.array_equal(occluded[0], vision[0])                        # a placed grasp: the hand is in the picture
    assert np.array_equal(occluded[1], vision[1])                            # an unplaced one: the object alone, bit for bit
    t = sampler.occluded_instances([[pu.GRASP_ACTION, 3]])
    assert t["inst_offset"].tolist() == [0, 22, 23]
    D = ops.VISION_DEFAULTS
    seen = ops.scene_render_posed(sampler.parts, *instances(t), t["inst_offset"], dev(t["cam_pos"], np.float32), dev(t["cam_rot"], np.float32),
                                  width=SIZE[0], height=SIZE[1])
    assert np.array_equal(seen["rgb"].cpu().numpy()[0], occluded[0]) and D["width"] == 256
    inst = seen["prim_inst"].cpu().numpy()
    assert ((inst[0] >= 1) & (inst[0] < 22)).any() and set(np.unique(inst[1])) <= {-1, 22}


def test_sampler_many_is_one_call_and_both_forms_agree(ops, sampler, monkeypatch):
    from a3vt_amd.pterotactyl.policies import rendered
    lists = [[pu.GRASP_ACTION, 3], [0, 0], [31, 49]]
    monkeypatch.setattr(rendered, "POSED_RENDER_DEFAULT", True)
    singles = [sampler.sample(a, touch=False, vision_occluded=True)["vision_occluded"] for a in lists]
    ops.posed_launches(reset=True)
    many = sampler.sample_many(lists, touch=False, vision_occluded=True)
    assert ops.posed_launches() == {"calls": 1, "kernels": 1, "pose_parts": 0}
    for k in range(3):
        assert all(np.array_equal(many[k]["vision_occluded"][e], singles[k][e]) for e in range(2))
    monkeypatch.setattr(rendered, "POSED_RENDER_DEFAULT", False)
    ops.posed_launches(reset=True)
    ops.scene_launches(reset=True)
    other = sampler.sample_many(lists, touch=False, vision_occluded=True)
    assert ops.posed_launches() == {"calls": 0, "kernels": 0, "pose_parts": 1} and ops.scene_launches()["calls"] == 1
    for k in range(3):
        assert all(np.array_equal(other[k]["vision_occluded"][e], singles[k][e]) for e in range(2))
    assert not np.array_equal(singles[0][0], singles[2][0])
    touch = sampler.sample(lists[0], vision_occluded=True)                   # next to the touch signals
    assert "touch_signal" in touch and np.array_equal(touch["vision_occluded"][0], singles[0][0])
