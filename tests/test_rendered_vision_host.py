"""CPU tests (no GPU) of the host logic around the data-set bake: ``RenderedSampler``'s vision images, packed cloud reads and
``sample_table`` extras with injected ``render`` / ``render_scene`` callables, and ``utility.data_making.save_image_info`` /
``save_touch_signals`` on a tree from ``chart_head_util.write_bake_tree`` with those fake renderers."""
import glob
import os

import numpy as np
import pytest
import torch

import scene_render_ref as sr
from chart_head_util import BAKE_OBJECTS as OBJECTS, bake_scene, write_bake_tree
from a3vt_amd import ops
from a3vt_amd.pterotactyl.policies import rendered
from a3vt_amd.pterotactyl.utility import data_making

A, PIX = 3, 121 * 121
NAMES = [f"/data/object_info/{o}" for o in OBJECTS]


def fake_render(verts, faces, face_offset, image_mesh, cam_pos, cam_rot, want_touch=True, want_points=True, **camera):
    """``ops.touch_render``'s signature and result from a generator seeded by the view's frame and mesh: equal views give equal
    signals, as a renderer's do.  A third of the views are "no_touch"; the counts stay below 50."""
    I = image_mesh.shape[0]
    out = {"depth": torch.zeros((I, 121, 121)), "status": torch.zeros(I, dtype=torch.int32)}
    touch, points, count = torch.zeros((I, 121, 121, 3)), torch.full((I, PIX, 3), float("nan")), torch.zeros(I, dtype=torch.int32)
    for i in range(I):
        m = int(image_mesh[i])                                                 # (the mesh by its size, not by its place in the batch)
        seed = int(np.abs(np.concatenate([cam_pos[i].numpy().ravel(), cam_rot[i].numpy().ravel()])).sum() * 1e6) + \
            int(face_offset[m + 1] - face_offset[m])
        g = np.random.default_rng(seed)
        out["status"][i] = int(seed % 3 != 0)
        count[i] = seed % 50                                                   # (a "no_touch" view may hold a count: it is dropped)
        touch[i] = torch.from_numpy(g.random((121, 121, 3)).astype(np.float32) * 255)
        points[i, :int(count[i])] = torch.from_numpy(g.random((int(count[i]), 3)).astype(np.float32))
    if want_touch:
        out["touch"] = touch
    if want_points:
        out["points"], out["count"] = points, count
    return out


class FakeScene:
    """``ops.scene_render``'s signature; image i is filled with its first face's colour, and every call is kept."""

    def __init__(self):
        self.calls = []

    def __call__(self, verts, faces, face_rgb, centres, radii, sphere_rgb, face_offset, sphere_offset, image_scene, cam_pos, cam_rot, **kw):
        self.calls.append(dict(kw, face_rgb=face_rgb, face_offset=list(face_offset), sphere_offset=list(sphere_offset),
                               image_scene=list(image_scene), cam_pos=cam_pos.clone(), cam_rot=cam_rot.clone(), spheres=centres.shape[0],
                               faces=faces))
        rgb = torch.zeros((len(image_scene), kw["height"], kw["width"], 3), dtype=torch.uint8)
        for i, m in enumerate(image_scene):
            rgb[i] = face_rgb[face_offset[m]]
        return {"rgb": rgb, "depth": torch.zeros(rgb.shape[:3])}


def make(scene=None, **kw):
    geometry, frames = bake_scene()
    s = rendered.RenderedSampler(frames, geometry, render=fake_render, render_scene=scene, **kw)
    s.load_objects(NAMES)
    return s


def test_the_vision_pose_looks_at_the_origin():
    D = ops.VISION_DEFAULTS
    R = rendered.camera_matrix(D["cam_euler_xyz_deg"])
    assert np.allclose(R, sr.camera_rotation((45.0, 0.0, 270.0)), atol=1e-15) and np.allclose(R @ R.T, np.eye(3), atol=1e-15)
    pos = np.asarray(D["cam_pos"])
    distance = np.linalg.norm(pos)
    assert abs(distance - 0.4243) < 5e-5
    assert np.allclose(pos + distance * (-R[:, 2]), 0.0, atol=1e-12)           # down its own -z, the origin is `distance` ahead
    assert np.array_equal(rendered.camera_matrix(R), R)
    with pytest.raises(ValueError, match="3 x 3"):
        rendered.camera_matrix(np.eye(4))
    assert D["lights"] == ((0.0, -0.8, 0.3, 1.0), (0.0, 0.8, 0.3, 1.0), (-1.0, 0.0, 1.0, 1.0), (1.0, 0.0, 1.0, 1.0))
    assert (D["ambient"], D["colour"], D["znear"], D["zfar"]) == (0.3, (228, 217, 111), 0.01, 10.0) and D["yfov"] == np.pi / 3
    assert D["background"] == ops.RENDER_DEFAULTS["background"]


def test_one_scene_call_with_the_reference_scene():
    scene = FakeScene()
    s = make(scene)
    got = s.sample([0, 1], vision=True)
    assert len(scene.calls) == 1
    call = scene.calls[0]
    D = ops.VISION_DEFAULTS
    geometry, _ = bake_scene()
    n_faces = [len(geometry[o][1]) for o in OBJECTS]
    assert call["face_offset"] == [0, n_faces[0], sum(n_faces)] and call["sphere_offset"] == [0, 0, 0] and call["image_scene"] == [0, 1]
    assert call["spheres"] == 0 and call["want_prim"] is False and (call["width"], call["height"]) == (256, 256)
    assert int(call["faces"][n_faces[0]:].min()) == len(geometry["ball"][0])   # global indices, as stored otherwise: no add_faces copies
    for key in ("yfov", "znear", "zfar", "lights", "ambient", "background"):
        assert call[key] == D[key], key
    assert call["face_rgb"].dtype == torch.uint8 and (call["face_rgb"] == torch.tensor(D["colour"], dtype=torch.uint8)).all()
    assert torch.equal(call["cam_pos"], torch.tensor([D["cam_pos"]] * 2))
    assert torch.equal(call["cam_rot"], torch.from_numpy(sr.camera_rotation(D["cam_euler_xyz_deg"]).astype(np.float32)).expand(2, 3, 3))
    images = got["vision"]
    assert isinstance(images, list) and len(images) == 2
    for image in images:
        assert isinstance(image, np.ndarray) and image.shape == (256, 256, 3) and image.dtype == np.uint8 and (image == D["colour"]).all()
    plain = s.sample([0, 1])                                                   # without vision: today's dict
    assert set(plain) == {"touch_status", "touch_signal", "depths", "finger_transfrom_pos", "finger_transform_rot_M"}
    assert set(got) == set(plain) | {"vision"} and all(torch.equal(got[k], plain[k]) for k in plain if k != "touch_status")
    assert s.sample([0, 1], touch=False) == {} and set(s.sample([0, 1], touch=False, vision=True)) == {"vision"}
    assert len(scene.calls) == 2
    many = s.sample_many([[0, 1], [1, 0]], vision=True)
    assert len(scene.calls) == 3 and many[0]["vision"] is many[1]["vision"]    # the images do not depend on the actions
    on_device = make(scene, to_host=False, resolution=[40, 24]).sample([0, 0], touch=False, vision=True)["vision"]
    assert all(isinstance(i, torch.Tensor) and i.shape == (24, 40, 3) and i.dtype == torch.uint8 for i in on_device)


def test_parameters_move_the_camera_and_colours_are_per_object():
    scene = FakeScene()
    s = make(scene, object_colours=[[10, 20, 30, 255], [200, 100, 50, 0]])
    euler = (30.0, -20.0, 110.0)
    matrix = sr.camera_rotation(euler)
    a = s.sample([0, 0], touch=False, vision=True, parameters=[((0.1, 0.2, 0.5), euler), None])["vision"]
    b = s.sample([0, 0], touch=False, vision=True, parameters=[((0.1, 0.2, 0.5), matrix), None])
    first, second = scene.calls
    assert torch.equal(first["cam_pos"], second["cam_pos"]) and torch.allclose(first["cam_rot"], second["cam_rot"], atol=1e-7, rtol=0)
    assert torch.equal(first["cam_pos"], torch.tensor([[0.1, 0.2, 0.5], list(ops.VISION_DEFAULTS["cam_pos"])]))
    assert torch.allclose(first["cam_rot"][0], torch.from_numpy(matrix.astype(np.float32)), atol=1e-7, rtol=0)
    assert torch.equal(first["cam_rot"][1], torch.from_numpy(sr.camera_rotation((45.0, 0.0, 270.0)).astype(np.float32)))
    assert (a[0] == (10, 20, 30)).all() and (a[1] == (200, 100, 50)).all() and (b["vision"][1] == (200, 100, 50)).all()   # alpha ignored
    one = make(scene, object_colours=[1, 2, 3, 4]).sample([0, 0], touch=False, vision=True)["vision"]
    assert (one[0] == (1, 2, 3)).all() and (one[1] == (1, 2, 3)).all()
    with pytest.raises(ValueError, match="object_colours"):
        make(scene, object_colours=np.zeros((3, 4))).sample([0, 0], vision=True)
    with pytest.raises(ValueError, match="1 camera parameters for 2"):
        s.sample([0, 0], vision=True, parameters=[None])
    with pytest.raises(NotImplementedError, match="hand model"):
        s.sample([0, 0], vision_occluded=True)
    with pytest.raises(RuntimeError, match="GPU"):                             # no render_scene given: the library's, which has no CPU form
        make().sample([0, 0], touch=False, vision=True)


def test_packed_and_padded_cloud_reads_are_the_same_bits():
    packs = []

    def counting(out, **kw):
        packs.append(kw)
        return rendered.pack_host(out, **kw)
    s = make(pack=counting)
    assert rendered.PACK_POINTS_DEFAULT in (True, False) and s.pack_points is rendered.PACK_POINTS_DEFAULT
    for lists in ([[0, 1]], [[2, 2], [1, 0], [7, 7]]):
        padded = s.sample_many(lists, touch_point_cloud=True, pack_points=False)
        assert not packs
        packed = s.sample_many(lists, touch_point_cloud=True, pack_points=True)
        assert packs == [dict(want_touch=False, want_points=True)]
        packs.clear()
        kept = 0
        for x, y in zip(padded, packed):
            assert x["touch_status"] == y["touch_status"] and torch.equal(x["touch_signal"], y["touch_signal"])
            for e in range(2):
                for f in range(4):
                    p, q = x["touch_point_cloud"][e][f], y["touch_point_cloud"][e][f]
                    assert p.dtype == q.dtype == np.float32 and p.shape == q.shape and np.array_equal(p.view(np.uint32), q.view(np.uint32))
                    assert (len(p) > 0) <= (x["touch_status"][e][f] == "touch")
                    kept += len(p)
        assert kept > 0
    s.sample([7, 7], touch_point_cloud=True, pack_points=True)                 # nothing rendered: nothing to pack
    assert not packs
    always = make(pack=counting, pack_points=True)
    always.sample([0, 1], touch_point_cloud=True)
    assert len(packs) == 1 and make(pack_points=False).pack_points is False


def test_pack_host_follows_the_contract():
    out = {"touch": torch.tensor([0.0, 0.5, 0.99999994, 1.0, 127.5, 254.99998, 255.0, -0.0, 300.0, -3.0, float("nan")]),
           "status": torch.tensor([1, 0, 1, 2, 1], dtype=torch.int32), "count": torch.tensor([2, 5, 0, 4, PIX + 9], dtype=torch.int32),
           "points": torch.arange(5 * PIX * 3, dtype=torch.float32).view(5, PIX, 3)}
    got = rendered.pack_host(out)
    assert got["touch_u8"].tolist() == [0, 0, 0, 1, 127, 254, 255, 0, 255, 0, 0]
    assert got["offsets"].tolist() == [0, 2, 2, 2, 2, 2 + PIX] and got["offsets"].dtype == torch.int32
    assert torch.equal(got["cloud"], torch.cat((out["points"][0, :2], out["points"][4])))


def test_the_table_with_clouds():
    packs = []

    def counting(out, **kw):
        packs.append(kw)
        return rendered.pack_host(out, **kw)
    s = make(pack=counting)
    plain = s.sample_table(A)
    assert set(plain) == {"touch_signal", "touch_code", "finger_transfrom_pos", "finger_transform_rot_M"} and not packs
    for kw in (dict(touch_point_cloud=True), dict(as_uint8=True), dict(touch_point_cloud=True, as_uint8=True, fingers=[3, 1])):
        packs.clear()
        table = s.sample_table(A, **kw)
        assert packs == [dict(want_touch=True, want_points=True)]              # one pack call for the whole table
        fingers = kw.get("fingers", [0, 1, 2, 3])
        Fs = len(fingers)
        assert set(table) == set(plain) | {"touch_u8", "cloud_offsets", "cloud"}
        if Fs == 4:
            assert all(torch.equal(table[k], plain[k]) for k in plain)         # the other keys keep their bits
        assert table["touch_u8"].shape == (2, A, Fs, 121, 121, 3) and table["touch_u8"].dtype == torch.uint8
        assert torch.equal(table["touch_u8"], table["touch_signal"].to(torch.uint8))
        offsets = table["cloud_offsets"]
        assert offsets.shape == (2 * A * Fs + 1,) and offsets.dtype == torch.int32 and int(offsets[0]) == 0
        assert table["cloud"].shape == (int(offsets[-1]), 3) and int(offsets[-1]) > 0
        for a in range(A):
            answer = s.sample([a, a], touch_point_cloud=True, pack_points=False)
            for e in range(2):
                for j, f in enumerate(fingers):
                    v = (e * A + a) * Fs + j
                    rows = table["cloud"][int(offsets[v]):int(offsets[v + 1])]
                    assert np.array_equal(rows.numpy().view(np.uint32), answer["touch_point_cloud"][e][f].view(np.uint32)), (e, a, f)
                    assert (len(rows) > 0) <= (int(table["touch_code"][e, a, j]) == 2)
    nothing = rendered.RenderedSampler({}, bake_scene()[0], render=fake_render)
    nothing.load_objects(NAMES)
    empty = nothing.sample_table(2, as_uint8=True)
    assert not empty["touch_u8"].any() and empty["cloud_offsets"].tolist() == [0] * 17 and empty["cloud"].shape == (0, 3)


# ---- the writers ----------------------------------------------------------------------------------------------------------------

def touch_files(root):
    return sorted(os.path.relpath(f, root) for kind in ("touch", "points") for f in glob.glob(os.path.join(root, "grasp_info", "*", "*", f"*_{kind}.npy")))


def read_all(root):
    return {f: open(os.path.join(root, f), "rb").read() for f in touch_files(root)}


@pytest.fixture()
def root(tmp_path):
    geometry, frames = bake_scene()
    root = write_bake_tree(str(tmp_path / "data"), geometry, frames)
    np.save(os.path.join(root, "object_info", "lonely_verts.npy"), np.zeros((3, 3), np.float32))      # an object without grasps
    np.save(os.path.join(root, "object_info", "lonely_faces.npy"), np.zeros((1, 3), np.int32))
    return root


def tree_sampler(root, **kw):
    return rendered.RenderedSampler(root, render=fake_render, to_host=False, **kw)


def test_save_touch_signals_files_counts_and_skips(root):
    frames_before = {f: open(f, "rb").read() for f in glob.glob(os.path.join(root, "grasp_info", "*", "*", "*_ref_frame.npy"))}
    counts = data_making.save_touch_signals(root, num_actions=A, sampler=tree_sampler(root), pack_points=True)
    s = tree_sampler(root)
    s.load_objects([os.path.join(root, "object_info", o) for o in OBJECTS])
    code = s.sample_table(A)["touch_code"].numpy()
    assert sorted(np.unique(code)) == [0, 1, 2]
    assert counts == dict(written=2, skipped_existing=0, skipped_no_grasps=1, views=2 * A * 4, touch=int((code == 2).sum()),
                          no_touch=int((code == 1).sum()), no_intersection=int((code == 0).sum()))
    want = sorted(os.path.join("grasp_info", o, str(a), f"{f}_{kind}.npy") for e, o in enumerate(OBJECTS) for a in range(A) for f in range(4)
                  for kind in ("touch", "points") if code[e, a, f] == 2)
    assert touch_files(root) == want                                          # the "touch" fingers and no other
    for e, obj in enumerate(OBJECTS):
        assert not os.path.exists(os.path.join(root, "grasp_info", obj, data_making.BAKING_MARKER))
        for a in range(A):
            answer = s.sample([a, a], touch_point_cloud=True, pack_points=False)
            d = os.path.join(root, "grasp_info", obj, str(a))
            if os.path.isdir(d):
                assert all(name.endswith(("_touch.npy", "_points.npy", "_ref_frame.npy")) for name in os.listdir(d)), os.listdir(d)
            for f in np.flatnonzero(code[e, a] == 2):
                touch, points = np.load(os.path.join(d, f"{f}_touch.npy")), np.load(os.path.join(d, f"{f}_points.npy"))
                assert touch.shape == (121, 121, 3) and touch.dtype == np.uint8 and points.dtype == np.float32 and points.ndim == 2
                assert np.array_equal(touch, answer["touch_signal"][e, f].numpy().astype(np.uint8))
                assert np.array_equal(points.view(np.uint32), answer["touch_point_cloud"][e][f].cpu().numpy().view(np.uint32))
    assert {f: open(f, "rb").read() for f in frames_before} == frames_before and \
        sorted(glob.glob(os.path.join(root, "grasp_info", "*", "*", "*_ref_frame.npy"))) == sorted(frames_before)   # read, never written
    first = read_all(root)
    stamps = {f: os.stat(os.path.join(root, f)).st_mtime_ns for f in first}
    again = data_making.save_touch_signals(root, num_actions=A, sampler=tree_sampler(root), pack_points=True)
    assert again == dict(written=0, skipped_existing=2, skipped_no_grasps=1, views=0, touch=0, no_touch=0, no_intersection=0)
    assert {f: os.stat(os.path.join(root, f)).st_mtime_ns for f in first} == stamps
    # a downloaded record is never silently replaced: one foreign file makes the whole object "existing"
    for f in touch_files(root):
        if f.startswith(os.path.join("grasp_info", "ball")):
            os.remove(os.path.join(root, f))
    foreign = os.path.join(root, "grasp_info", "ball", "0", "1_points.npy")
    np.save(foreign, np.ones((2, 3)))
    assert data_making.save_touch_signals(root, num_actions=A, sampler=tree_sampler(root))["skipped_existing"] == 2
    assert np.load(foreign).dtype == np.float64
    # ... a marker says the object was interrupted: it is written again, stale records go, the marker goes
    open(os.path.join(root, "grasp_info", "ball", data_making.BAKING_MARKER), "w").close()
    stale = os.path.join(root, "grasp_info", "ball", "2", "9_touch.npy")
    np.save(stale, np.zeros(1))
    third = data_making.save_touch_signals(root, num_actions=A, sampler=tree_sampler(root), pack_points=True)
    assert third["written"] == 1 and third["skipped_existing"] == 1 and third["views"] == A * 4
    assert not os.path.exists(stale) and not os.path.exists(os.path.join(root, "grasp_info", "ball", data_making.BAKING_MARKER))
    assert read_all(root) == first
    # ... and so does overwrite; packed or padded, the files are the same bytes
    fourth = data_making.save_touch_signals(root, num_actions=A, sampler=tree_sampler(root), pack_points=False, overwrite=True, batch=1)
    assert fourth == counts and read_all(root) == first
    dry = data_making.save_touch_signals(root, num_actions=A, sampler=tree_sampler(root), overwrite=True, write=False)
    assert dry == counts and {f: os.stat(os.path.join(root, f)).st_mtime_ns for f in first} != stamps
    with pytest.raises(ValueError, match=f"{5000 * 50 * 4} views"):
        data_making.save_touch_signals(root, batch=5000)


def test_the_marker_exists_while_an_object_is_written(root, monkeypatch):
    seen = []
    real = data_making._save_atomic

    def watching(directory, name, array):
        obj_dir = os.path.dirname(directory)
        seen.append((os.path.exists(os.path.join(obj_dir, data_making.BAKING_MARKER)),
                     [f for f in os.listdir(directory) if f.endswith(".tmp")]))
        real(directory, name, array)
    monkeypatch.setattr(data_making, "_save_atomic", watching)
    data_making.save_touch_signals(root, num_actions=A, sampler=tree_sampler(root), pack_points=True)
    assert seen and all(marker and not temporaries for marker, temporaries in seen)
    assert not glob.glob(os.path.join(root, "grasp_info", "*", data_making.BAKING_MARKER))
    assert not glob.glob(os.path.join(root, "grasp_info", "*", "*", ".*"))      # no temporary file is left


def test_save_image_info_with_a_fake_scene(root):
    np.save(os.path.join(root, "object_info", "empty_verts.npy"), np.zeros((3, 3), np.float32))
    np.save(os.path.join(root, "object_info", "empty_faces.npy"), np.zeros((0, 3), np.int32))
    scene = FakeScene()
    sampler = rendered.RenderedSampler({}, render=fake_render, render_scene=scene, object_colours=[9, 8, 7, 255])
    counts = data_making.save_image_info(root, batch=2, sampler=sampler)
    assert counts == dict(written=3, skipped_existing=0, skipped_no_surface=1)
    assert [c["image_scene"] for c in scene.calls] == [[0, 1], [0]]            # sorted ids, `batch` per call: ball, lonely | pebble
    assert sorted(os.listdir(os.path.join(root, "images_colourful"))) == ["ball.npy", "lonely.npy", "pebble.npy"]
    image = np.load(os.path.join(root, "images_colourful", "pebble.npy"))
    assert image.shape == (256, 256, 3) and image.dtype == np.uint8 and (image == (9, 8, 7)).all()
    assert data_making.save_image_info(root, sampler=sampler) == dict(written=0, skipped_existing=3, skipped_no_surface=1)
    assert len(scene.calls) == 2
    os.remove(os.path.join(root, "images_colourful", "ball.npy"))
    assert data_making.save_image_info(root, sampler=sampler)["written"] == 1 and scene.calls[-1]["image_scene"] == [0]
    assert data_making.save_image_info(root, sampler=sampler, overwrite=True)["written"] == 3
    with pytest.raises(ValueError, match="128"):
        data_making.save_image_info(root, batch=129, sampler=sampler)
