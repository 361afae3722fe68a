"""CPU tests (no GPU) of the host side of the occluded vision images: ``HandVisual``, ``GraspFrames.hand_links``, the NumPy form of
``ops.pose_parts``, ``ops.PartTable``'s bounds, ``RenderedSampler``'s instance lists with injected ``render_posed`` / ``render_scene``
fakes, and the two views the GPU tests hold against the fp64 yardstick (the reference alone must leave at most 0.1 % undecided)."""
import os

import numpy as np
import pytest
import torch

import posed_render_util as pu
from a3vt_amd import ops
from a3vt_amd.pterotactyl.policies import rendered
from a3vt_amd.pterotactyl.simulator import hand as hand_module
from a3vt_amd.pterotactyl.simulator.hand import HandVisual

LINKS = [-1, 0, 1, 2, 3, 4, 7, 8, 9, 10, 11, 14, 15, 16, 17, 18, 21, 22, 23, 24, 25]


@pytest.fixture(scope="module")
def golden():
    return pu.golden_hand()


# ---- the visual hand ------------------------------------------------------------------------------------------------------------
def test_hand_visual_round_trip(golden, tmp_path, monkeypatch):
    _, visual = golden
    assert len(visual.parts) == 10 and len(visual.nodes) == 21 and visual.links == LINKS and visual.num_faces == 7808
    assert [n[0] for n in visual.nodes] == [0] + [1, 2, 3, 4, 5] * 3 + [6, 7, 8, 9, 5]
    for part, link, rgb in visual.nodes:
        assert rgb == ((119, 225, 153) if part == 5 else (119, 136, 153))
    assert hand_module.HAND_COLOUR == (119, 136, 153) and hand_module.DIGIT_COLOUR == (119, 225, 153)
    assert all(v.dtype == np.float32 and f.dtype == np.int32 for v, f in visual.parts)
    path = str(tmp_path / "visual.npz")
    visual.save(path)
    with np.load(path, allow_pickle=False) as z:                             # arrays only
        assert all(z[k].dtype.kind in "fiuU" for k in z.files)
    monkeypatch.setenv("PTEROTACTYL_HAND_MESHES", path)
    back = HandVisual.load()
    assert back.nodes == visual.nodes and len(back.parts) == 10
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(back.parts, visual.parts))
    monkeypatch.delenv("PTEROTACTYL_HAND_MESHES")
    with pytest.raises(ValueError, match="PTEROTACTYL_HAND_MESHES"):
        HandVisual.load()
    with pytest.raises(ValueError, match="face indices"):
        HandVisual([(np.zeros((3, 3)), [[0, 1, 3]])], [(0, -1, (1, 2, 3))])
    with pytest.raises(ValueError, match="node"):
        HandVisual([(np.zeros((3, 3)), [[0, 1, 2]])], [(1, -1, (1, 2, 3))])


def test_live_load_against_the_fixture(golden):
    """Where the reference is present: a live load of ``meshes_obj`` equals the golden file, and every part drawn on a link
    intersects that link's collision box in the link frame (a condition of drawing the parts in the link frames)."""
    from oracle.ref_shim import REFERENCE_ROOT
    folder = os.path.join(REFERENCE_ROOT, "pterotactyl", "objects", "hand", "meshes_obj")
    if not os.path.isdir(folder):
        pytest.skip("the reference's hand files are not on this machine")
    hand, visual = golden
    live = HandVisual.load(folder)
    assert live.nodes == visual.nodes
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(live.parts, visual.parts))
    for part, link, _ in visual.nodes[1:]:
        lo, hi = visual.parts[part][0].min(axis=0), visual.parts[part][0].max(axis=0)
        c, h = hand.box_centre[link], hand.box_half[link]
        assert hand.has_box[link] and ((lo <= c + h) & (hi >= c - h)).all(), (part, link)
        if part in (1, 2, 3, 4, 7, 8, 9):                                    # and the finger parts' bounds ARE the boxes, to the millimetre
            assert np.abs(lo - (c - h)).max() < 1e-3 and np.abs(hi - (c + h)).max() < 1e-3, (part, link)


# ---- the link poses -------------------------------------------------------------------------------------------------------------
def test_hand_links_against_forward_kinematics(golden):
    from a3vt_amd.pterotactyl.simulator.physics.grasping import GraspFrames, KinematicGrasp
    hand, _ = golden
    geometry = dict(pu.grasp_geometry(), flat=(np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0]], np.float32), np.array([[0, 1, 2]])))
    grasper = KinematicGrasp(hand, steps=8, device="cpu")
    frames = GraspFrames(grasper, geometry, num_actions=50)
    before = frames[(pu.GRASP_OBJECT, 3)]
    links = frames.hand_links(pu.GRASP_OBJECT, 3)
    assert links is not None and [a.shape for a in links] == [(3,), (3, 3), (28, 3), (28, 3, 3)] and all(a.dtype == np.float32 for a in links)
    full = grasper.grasp_table(geometry, [pu.GRASP_OBJECT], 50, want_q=True, want_links=True)
    pos, rot = hand.forward(full["base_pos"][0, 3], full["base_rot"][0, 3], np.concatenate([full["q"][0, 3].reshape(4, 4), np.zeros((4, 3))], 1).ravel())
    assert np.array_equal(links[2], full["link_pos"][0, 3]) and np.array_equal(links[0], full["base_pos"][0, 3])
    assert np.abs(links[2] - pos).max() < 1e-6 and np.abs(links[3] - rot).max() < 1e-6       # float32 storage of a float64 chain
    # the frames are the rows of the touch cameras, and table() / __getitem__ answer as before
    after = frames[(pu.GRASP_OBJECT, 3)]
    assert all(np.array_equal(a, b) for a, b in zip(before, after)) and set(frames.table(pu.GRASP_OBJECT)) == {"pos", "rot", "present"}
    assert np.array_equal(links[2][hand.touch_cameras], after[0])
    assert frames.link_table(pu.GRASP_OBJECT) is frames.link_table(pu.GRASP_OBJECT)          # one table per object, kept
    assert frames.hand_links("flat", 0) is None                                              # no hull: not placed
    with pytest.raises(KeyError):
        frames.hand_links("absent", 0)
    with pytest.raises(KeyError):
        frames.hand_links(pu.GRASP_OBJECT, 50)


# ---- pose_parts in NumPy, the part table -----------------------------------------------------------------------------------------
def test_numpy_pose_parts():
    parts = [pu.tetra(), pu.box(), pu.fan(3)]
    table = ops.PartTable(parts, device="cpu")
    assert table.vert_offset.tolist() == [0, 4, 12, 16] and table.face_offset.tolist() == [0, 4, 16, 19] and table.faces.dtype == torch.int32
    assert int(table.faces[4:16].min()) == 4
    image = [(1, (0.1, -0.2, 0.3), pu.GENERIC, (1, 2, 3)), (7, (0, 0, 0), pu.EYE, (4, 5, 6)), (0, (0, 0, 0), pu.EYE, (7, 8, 9)),
             (0, (1.5, 0, 0), 3 * pu.QUARTER, (9, 9, 9))]
    t = pu.tables([image[:1], [], image[1:]])
    out = ops.pose_parts(table, *(torch.from_numpy(t[k]) for k in ("inst_part", "inst_pos", "inst_rot", "inst_rgb")), inst_offset=t["inst_offset"])
    assert out["vert_base"].tolist() == [0, 8, 8, 12, 16] and out["face_base"].tolist() == [0, 12, 12, 16, 20]     # the unknown part owns no rows
    assert out["face_offset"].tolist() == [0, 12, 12, 20]
    verts, faces, rgb = out["verts"].numpy(), out["faces"].numpy(), out["face_rgb"].numpy()
    R, p = t["inst_rot"][0].astype(np.float64), t["inst_pos"][0].astype(np.float64)
    assert np.abs(verts[:8] - (parts[1][0].astype(np.float64) @ R.T + p)).max() < 1e-7
    assert np.array_equal(verts[8:12], parts[0][0])                          # the identity leaves the template's bits
    quarter = parts[0][0].astype(np.float64) @ (3 * pu.QUARTER).T + [1.5, 0, 0]
    assert np.array_equal(verts[12:16], quarter.astype(np.float32))          # exact products: no rounding to differ by
    assert np.array_equal(faces[:12], parts[1][1]) and np.array_equal(faces[12:16], parts[0][1] + 8) and np.array_equal(faces[16:], parts[0][1] + 12)
    assert (rgb[:12] == [1, 2, 3]).all() and (rgb[12:16] == [7, 8, 9]).all() and (rgb[16:] == 9).all()
    row = pu.materialised_index(table.face_offset, t["inst_part"], out["face_base"], np.array([0, 2, 3, -1]), np.array([15, 0, 3, -1]))
    assert row.tolist() == [11, 12, 19, -1]
    nan = t["inst_pos"].copy()
    nan[0, 1] = np.nan
    bad = ops.pose_parts(table, torch.from_numpy(t["inst_part"]), torch.from_numpy(nan), torch.from_numpy(t["inst_rot"]), torch.from_numpy(t["inst_rgb"]))
    assert np.isnan(bad["verts"].numpy()[:8, 1]).all() and np.isfinite(bad["verts"].numpy()[8:]).all()


def test_part_table_bounds_and_refusals():
    g = np.random.default_rng(0)
    cloud = g.normal(size=(200, 3)).astype(np.float32) * [0.02, 0.3, 0.001] + [5.0, -2.0, 0.1]
    cloud[17] = np.nan
    table = ops.PartTable([(cloud, np.zeros((0, 3))), (np.full((3, 3), np.inf), [[0, 1, 2]]), pu.tetra()], device="cpu")
    centre, radius = table.bound[0, :3].astype(np.float64), float(table.bound[0, 3])
    good = np.delete(cloud, 17, axis=0).astype(np.float64)
    far = np.sqrt(((good - centre) ** 2).sum(axis=1).max())
    assert table.bound.dtype == np.float32 and radius >= far and radius <= far * (1 + 1e-6)        # holds every finite vertex, rounded UP
    assert table.bound[1].tolist() == [0, 0, 0, 0] and abs(table.bound[2, 3] - 0.004 * 3 ** 0.5) < 1e-8
    with pytest.raises(ValueError, match="face indices"):
        ops.PartTable([(np.zeros((3, 3)), [[0, 1, 3]])], device="cpu")
    with pytest.raises(ValueError, match="1..96"):
        ops.PartTable([pu.tetra()] * 97, device="cpu")
    with pytest.raises(ValueError, match="1..96"):
        ops.PartTable([], device="cpu")
    assert ops.POSED_LIMITS == dict(parts=96, instances=1 << 24)


# ---- the sampler with fakes -----------------------------------------------------------------------------------------------------
GEOMETRY = {"ball": pu.ico(1, 0.05), "egg": pu.ico(0, 0.03)}
NAMES = ["/data/object_info/ball", "/data/object_info/egg"]


class FakeFrames(dict):
    """A ``frames`` mapping that also knows link poses: odd actions are not placed."""

    def hand_links(self, obj, action):
        if action % 2:
            return None
        g = np.random.default_rng(action + 100 * len(obj))
        return (g.random(3).astype(np.float32), g.random((3, 3)).astype(np.float32), g.random((28, 3)).astype(np.float32),
                g.random((28, 3, 3)).astype(np.float32))


class FakePosed:
    """``ops.scene_render_posed``'s signature; image i is filled with its LAST instance's colour, and every call is kept."""

    def __init__(self):
        self.calls = []

    def __call__(self, table, inst_part, inst_pos, inst_rot, inst_rgb, inst_offset, cam_pos, cam_rot, **kw):
        self.calls.append(dict(kw, table=table, inst_part=inst_part, inst_pos=inst_pos, inst_rot=inst_rot, inst_rgb=inst_rgb,
                               inst_offset=list(inst_offset), cam_pos=cam_pos, cam_rot=cam_rot))
        rgb = torch.zeros((len(inst_offset) - 1, kw["height"], kw["width"], 3), dtype=torch.uint8)
        for i in range(len(inst_offset) - 1):
            rgb[i] = inst_rgb[inst_offset[i + 1] - 1]
        return {"rgb": rgb}


def fake_scene(verts, faces, face_rgb, centres, radii, sphere_rgb, face_offset, sphere_offset, image_scene, cam_pos, cam_rot, **kw):
    rgb = torch.zeros((len(image_scene), kw["height"], kw["width"], 3), dtype=torch.uint8)
    for i, m in enumerate(image_scene):
        rgb[i] = face_rgb[face_offset[m + 1] - 1]
    return {"rgb": rgb, "faces": faces, "verts": verts, "face_offset": list(face_offset)}


def make(visual, frames=None, **kw):
    s = rendered.RenderedSampler(FakeFrames() if frames is None else frames, GEOMETRY, render=lambda *a, **k: None, hand_visual=visual,
                                 resolution=[8, 6], **kw)
    s.load_objects(NAMES)
    return s


def test_the_instance_lists(golden):
    _, visual = golden
    fake = FakePosed()
    s = make(visual, render_posed=fake, render_scene=fake_scene, object_colours=[[10, 20, 30, 99], [40, 50, 60, 255]])
    assert s.parts.num_parts == 12 and s.parts.face_offset[-1] == sum(len(f) for _, f in visual.parts) + 80 + 20
    got = s.occluded_images([[4, 1], [3, 6]], posed=True)
    assert len(fake.calls) == 1 and len(got) == 2 and all(len(images) == 2 for images in got)
    call = fake.calls[0]
    D = ops.VISION_DEFAULTS
    assert call["inst_offset"] == [0, 22, 23, 24, 46] and call["table"] is s.parts and call["want_prim"] is False
    assert (call["width"], call["height"]) == (8, 6) and all(call[k] == D[k] for k in ("yfov", "znear", "zfar", "lights", "ambient", "background"))
    part, pos, rot, rgb = (call[k].numpy() for k in ("inst_part", "inst_pos", "inst_rot", "inst_rgb"))
    assert part.dtype == np.int32 and pos.dtype == np.float32 and rot.dtype == np.float32 and rgb.dtype == np.uint8
    node_part = [n[0] for n in visual.nodes]
    assert part.tolist() == [10] + node_part + [11] + [10] + [11] + node_part
    for row, colour in ((0, [10, 20, 30]), (22, [40, 50, 60]), (23, [10, 20, 30]), (24, [40, 50, 60])):      # the object: identity, its colour
        assert not pos[row].any() and np.array_equal(rot[row], np.eye(3)) and rgb[row].tolist() == colour
    base_pos, base_rot, link_pos, link_rot = FakeFrames().hand_links("ball", 4)
    assert np.array_equal(pos[1], base_pos) and np.array_equal(rot[1], base_rot)                            # node 0: the base
    assert np.array_equal(pos[2:22], link_pos[LINKS[1:]]) and np.array_equal(rot[2:22], link_rot[LINKS[1:]])
    assert np.array_equal(rgb[1:22], np.array([n[2] for n in visual.nodes], np.uint8))
    base_pos, _, link_pos, _ = FakeFrames().hand_links("egg", 6)
    assert np.array_equal(pos[25], base_pos) and np.array_equal(pos[26:46], link_pos[LINKS[1:]])
    # the images: K lists of E arrays; a placed grasp ends with a digit, an unplaced one is the object alone
    assert all(im.shape == (6, 8, 3) and im.dtype == np.uint8 for images in got for im in images)
    assert (got[0][0] == [119, 225, 153]).all() and (got[0][1] == [40, 50, 60]).all() and (got[1][0] == [10, 20, 30]).all()
    # sample / sample_many put them under "vision_occluded"
    out = s.sample_many([[4, 1], [3, 6]], touch=False, vision_occluded=True)
    assert len(fake.calls) == 2 and [set(o) for o in out] == [{"vision_occluded"}] * 2            # one more call for all K * E images
    assert fake.calls[1]["inst_offset"] == call["inst_offset"]
    assert all(np.array_equal(a, b) for k in range(2) for a, b in zip(out[k]["vision_occluded"], got[k]))


def test_both_forms_and_the_default(golden, monkeypatch):
    """The materialised form hands ``pose_parts``' triangles to ``render_scene``: one scene per image with exactly the instances'
    faces; ``POSED_RENDER_DEFAULT`` chooses when the caller does not."""
    _, visual = golden
    fake = FakePosed()
    s = make(visual, render_posed=fake, render_scene=fake_scene)
    a = s.occluded_images([[4, 1]], posed=False)
    assert not fake.calls and (a[0][0] == [119, 225, 153]).all() and (a[0][1] == ops.VISION_DEFAULTS["colour"]).all()
    monkeypatch.setattr(rendered, "POSED_RENDER_DEFAULT", False)
    b = s.sample([4, 1], touch=False, vision_occluded=True)["vision_occluded"]
    assert not fake.calls and all(np.array_equal(x, y) for x, y in zip(a[0], b))
    monkeypatch.setattr(rendered, "POSED_RENDER_DEFAULT", True)
    c = s.sample([4, 1], touch=False, vision_occluded=True)["vision_occluded"]
    assert len(fake.calls) == 1 and all(np.array_equal(x, y) for x, y in zip(a[0], c))


def test_camera_parameters(golden):
    _, visual = golden
    fake = FakePosed()
    s = make(visual, render_posed=fake)
    move = (np.array([0.1, 0.2, 0.5]), (10.0, 20.0, 30.0))
    s.occluded_images([[0, 0], [2, 2], [1, 1]], parameters=[None, move], posed=True)
    call = fake.calls[0]
    D = ops.VISION_DEFAULTS
    assert call["cam_pos"].shape == (6, 3) and call["cam_rot"].shape == (6, 3, 3)
    for k in range(3):                                                       # image (k, e) has element e's camera
        assert np.allclose(call["cam_pos"][2 * k].numpy(), D["cam_pos"]) and np.allclose(call["cam_pos"][2 * k + 1].numpy(), move[0])
        assert np.allclose(call["cam_rot"][2 * k].numpy(), rendered.camera_matrix(D["cam_euler_xyz_deg"]), atol=1e-7)
        assert np.allclose(call["cam_rot"][2 * k + 1].numpy(), rendered.camera_matrix(move[1]), atol=1e-7)


def test_error_paths(golden):
    _, visual = golden
    plain = rendered.RenderedSampler(FakeFrames(), GEOMETRY, render=lambda *a, **k: None)
    plain.load_objects(NAMES)
    with pytest.raises(NotImplementedError, match="hand model"):            # without a hand: as before
        plain.sample([0, 0], vision_occluded=True)
    with pytest.raises(ValueError, match="hand_visual"):
        plain.occluded_images([[0, 0]])
    tree = make(visual, frames={})                                           # a plain mapping stores finger frames only
    with pytest.raises(ValueError, match="hand_links"):
        tree.sample([0, 0], touch=False, vision_occluded=True)
    s = make(visual, render_posed=FakePosed())
    with pytest.raises(ValueError, match="1 actions for 2"):
        s.occluded_images([[0]])
    with pytest.raises(ValueError, match="3 camera parameters for 2"):
        s.occluded_images([[0, 0]], parameters=[None] * 3)
    fresh = rendered.RenderedSampler(FakeFrames(), GEOMETRY, render=lambda *a, **k: None, hand_visual=visual)
    with pytest.raises(RuntimeError, match="load_objects"):
        fresh.occluded_images([[]])
    few = HandVisual(visual.parts, [(0, 40, (1, 2, 3))])                     # a node on a link the grasp does not have
    with pytest.raises(ValueError, match="link 40"):
        make(few, render_posed=FakePosed()).occluded_images([[0, 0]], posed=True)


# ---- the yardstick views --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["synthetic", "golden"])
def test_the_yardstick_views_are_decided(name):
    parts, image, pos, rot, yfov, scene, owner, want = pu.yard_view(name)
    share = want["undecided"].mean()
    seen = np.unique(owner[want["prim"][want["prim"] >= 0], 0])
    print(f"{name}: {len(image)} instances, {len(scene['faces'])} faces, {int(want['undecided'].sum())} of {want['undecided'].size} pixels "
          f"undecided, hits {int((want['depth'] > 0).sum())}, instances seen {len(seen)}, float32 emulation's depth deviation {want['yard']:.3e}")
    assert share <= 1e-3
    assert len(seen) > 5 and 0 in seen and (seen > 0).any()                  # the object and the hand in front of it
    if name == "golden":
        assert len(image) == 22 and len(scene["faces"]) == 7808 + 320
