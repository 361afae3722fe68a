"""``a3vt_scene_render`` (csrc/scene_render.hip) on the GPU against the NumPy emulation ``scene_render_ref``, and the classes built on
it (``utility/pretty_render.py``, ``utils.visualize_prediction``, the vision trainer's ``visualize`` path).

The yardstick is ``scene_render_util``'s (the protocol of ``test_gpu_touch_render.py``): a pixel is *undecided* if its prim or its
depth (relative 1e-6) moves when faces and spheres are loosened and tightened by 1e-5, or if the fp64 winner and runner-up lie within
1e-6 of each other with a different colour or normal; such pixels may not exceed 0.1 % of an image (checked for the fp64 reference
alone in ``test_scene_render_ref_host.py``).  On the rest prim is equal, no hit is missed or invented, the relative depth error is at
most 8 x the float32 emulation's own against fp64, every colour channel within one level of the fp64 image.

Measured on an MI355X (depth: the float32 emulation's largest relative deviation, then the kernel's; undecided pixels):
    ico3_512                2.4e-6, 5.3e-6 (1 of 262 144)     size edges 40 x 24 .. 1 x 1      <= 4.4e-7, <= 2.6e-7 (0)
    faces 1 .. 513          1.3e-7 .. 9.3e-6, <= 2.6e-7 (<= 2) spheres 1 .. 257, mixed 257      <= 5.2e-6, <= 8.7e-7 (0)
    colour: at most one level off anywhere; no hit and no prim differs on a decided pixel; the file takes 6 s
    (`profiles/scene_render.txt` has every line)."""
import os

import numpy as np
import pytest
import torch

import scene_render_util as su

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(cuda):
    from a3vt_amd import ops
    return ops


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def render(ops, scenes, image_scene=(0,), pos=None, rot=None, W=su.COUNT_SIZE[0], H=su.COUNT_SIZE[1], yfov=su.NARROW_YFOV, lights=su.LIGHTS,
           **kw):
    """``ops.scene_render`` on a list of scenes -> the dict as NumPy arrays; the NARROW camera for every image unless given."""
    t = su.pack(scenes)
    n = len(image_scene)
    pos = np.tile(su.NARROW_POS, (n, 1)) if pos is None else np.asarray(pos).reshape(n, 3)
    rot = np.tile(su.CAM_ROT, (n, 1, 1)) if rot is None else np.asarray(rot).reshape(n, 3, 3)
    out = ops.scene_render(dev(t["verts"], np.float32), dev(t["faces"], np.int32), dev(t["face_rgb"], np.uint8), dev(t["centres"], np.float32),
                           dev(t["radii"], np.float32), dev(t["sphere_rgb"], np.uint8), t["face_offset"], t["sphere_offset"],
                           list(image_scene), dev(pos, np.float32), dev(rot, np.float32), yfov=yfov, width=W, height=H, lights=lights, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def first(out, i=0):
    return {k: v[i] for k, v in out.items()}


def same(a, b):
    return all(np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k], b[k].view(np.uint32) if b[k].dtype == np.float32
                              else b[k]) for k in ("rgb", "depth", "prim"))


def render_view(ops, name, **kw):
    scene, W, H, pos, yfov = su.views()[name]
    return first(render(ops, [scene], pos=pos, W=W, H=H, yfov=yfov, **kw))


# ---- against the yardstick ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ico3_512"] + [f"size_{w}x{h}" for w, h in su.SIZE_EDGES])
def test_image_size_edges(ops, name):
    """Partial tiles at the right edge, the bottom edge and both, a single pixel, and 1 024 tiles of an icosphere-3."""
    got = render_view(ops, name)
    su.check(got, su.view_reference(name), name)
    assert got["rgb"].shape == got["depth"].shape + (3,) and (got["prim"] >= 0).any()


@pytest.mark.parametrize("name", [f"faces_{n}" for n in su.FACE_COUNTS] + [f"spheres_{n}" for n in su.SPHERE_COUNTS] + ["mixed_257"])
def test_count_edges(ops, name):
    """One primitive, a chunk less one, a chunk, a chunk and one, two chunks and one; 257 of each kind, where the faces' last
    chunk and the spheres' first meet.  The meshes fill the image: a ray that sees the background has leaked through a shared edge."""
    got = render_view(ops, name)
    su.check(got, su.view_reference(name), name)
    if not name.startswith("spheres_"):
        assert (got["depth"] > 0).all() and (got["prim"] >= 0).all()


def test_order(ops):
    for name, front in (("sphere_before_triangle", 1), ("triangle_before_sphere", 0)):
        got = render_view(ops, name)
        su.check(got, su.view_reference(name), name)
        assert (got["prim"] == front).any() and ((got["prim"] == 1).any() == (front == 1))


def test_coincident_faces_and_reversed_tables(ops):
    from a3vt_amd.pterotactyl.utility import utils
    base = su.ico(2, 0.04)
    n = len(base["faces"])
    colours = np.repeat(su.PALETTE[:3], n, axis=0)                      # each copy of add_faces its own colour
    tripled = su.make(base["verts"], utils.add_faces(base["faces"]), face_rgb=colours)
    got = first(render(ops, [tripled]))
    hit = got["prim"] >= 0
    assert hit.any() and (got["prim"][hit] < n).all()                   # the lowest index of the three wins at every pixel
    alone = first(render(ops, [su.make(base["verts"], base["faces"], face_rgb=su.PALETTE[0])]))
    assert same(got, alone)
    # the same primitives in reverse table order: the same depth and the same primitive under the mapping, wherever one is decided
    scene = su.views()["mixed_257"][0]
    F, S = len(scene["faces"]), len(scene["centres"])
    flipped = su.make(scene["verts"], scene["faces"][::-1], scene["face_rgb"][::-1], scene["centres"][::-1], scene["radii"][::-1],
                      scene["sphere_rgb"][::-1])
    a, b = first(render(ops, [scene])), first(render(ops, [flipped]))
    mapped = np.where(b["prim"] < 0, -1, np.where(b["prim"] < F, F - 1 - b["prim"], F + (S - 1 - (b["prim"] - F))))
    ok = ~su.view_reference("mixed_257")["undecided"]
    assert np.array_equal(a["prim"][ok], mapped[ok]) and np.array_equal(a["depth"][ok].view(np.uint32), b["depth"][ok].view(np.uint32))
    assert np.array_equal(a["rgb"][ok], b["rgb"][ok])


def test_depth_range(ops):
    plane, ball = su.fan(1), su.make(**su.BALL)
    want_scene = su.merge(plane, ball)
    plain = first(render(ops, [want_scene]))
    # behind the camera, and the camera inside a sphere: as if they were not there
    behind = su.make([[-1, 3, 3], [1, 3, 3], [0, 3.5, 4]], [[0, 1, 2]], centres=[[0, 2.8, 2.8], su.NARROW_POS], radii=[0.5, 0.7])
    got = first(render(ops, [su.merge(want_scene, behind)]))
    assert np.array_equal(got["rgb"], plain["rgb"]) and np.array_equal(got["depth"].view(np.uint32), plain["depth"].view(np.uint32))
    assert np.array_equal(np.where(got["prim"] == 2, 1, got["prim"]), plain["prim"]) and set(np.unique(got["prim"])) == {0, 2}
    # the plane's depth runs across 1.98: with znear or zfar there, it is hit only beyond / before it, and so is the ball
    lo, hi = float(plain["depth"].min()), float(plain["depth"].max())
    assert lo < 1.975 < 1.985 < hi
    for kw, rule in ((dict(znear=1.975), lambda d: d >= np.float32(1.975)), (dict(zfar=1.985), lambda d: d <= np.float32(1.985))):
        scene, W, H, pos, yfov = su.views()["sphere_before_triangle"]
        want = su.reference(scene, W, H, pos=pos, yfov=yfov, **kw)
        got = first(render(ops, [scene], **kw))
        su.check(got, want, f"range {kw}")
        hit = got["depth"] > 0
        assert hit.any() and (~hit).any() and rule(got["depth"][hit]).all() and (got["prim"][~hit] == -1).all()
        unchanged = hit & (got["prim"] == plain["prim"])                 # (a ball cut away by znear shows the plane behind it)
        assert unchanged.any() and np.array_equal(got["depth"][unchanged].view(np.uint32), plain["depth"][unchanged].view(np.uint32))
    ball_depth = plain["depth"][plain["prim"] == 1]
    straddle = float(np.median(ball_depth))
    got = first(render(ops, [want_scene], znear=straddle))
    assert 0 < (got["prim"] == 1).sum() < (plain["prim"] == 1).sum() and (got["depth"][got["prim"] == 1] >= np.float32(straddle)).all()


def test_bad_data_disturbs_nothing(ops):
    scene = su.views()["mixed_257"][0]
    F = len(scene["faces"])
    cases = {}
    bad = {k: v.copy() for k, v in scene.items()}
    bad["verts"][7] = [np.nan, 0.1, 0.0]                                 # a rim vertex: two faces of the fan
    cases["a NaN vertex"] = (bad, (scene["faces"] == 7).any(axis=1), np.zeros(len(scene["radii"]), bool))
    for what, (key, value) in {"an Inf centre": ("centres", [np.inf, 0.0, 0.01]), "a zero radius": ("radii", 0.0),
                               "a negative radius": ("radii", -0.003), "a NaN radius": ("radii", np.nan)}.items():
        bad = {k: v.copy() for k, v in scene.items()}
        bad[key][100] = value
        gone = np.zeros(len(scene["radii"]), bool)
        gone[100] = True
        cases[what] = (bad, np.zeros(F, bool), gone)
    for what, (bad, no_face, no_sphere) in cases.items():
        got = first(render(ops, [bad]))
        kept = su.make(scene["verts"], scene["faces"][~no_face], scene["face_rgb"][~no_face], scene["centres"][~no_sphere],
                       scene["radii"][~no_sphere], scene["sphere_rgb"][~no_sphere])
        want = first(render(ops, [kept]))
        index = np.concatenate([[-1], np.flatnonzero(~no_face), F + np.flatnonzero(~no_sphere)])      # kept's prim -> the full table's
        assert np.array_equal(got["rgb"], want["rgb"]) and np.array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32)), what
        assert np.array_equal(got["prim"], index[want["prim"] + 1]), what
        assert np.isfinite(got["depth"]).all()


def test_batch(ops):
    """I = 5 over M = 3 scenes, one empty, one seen by two cameras: every image is what it is alone, twice."""
    scenes = [su.views()["mixed_257"][0], su.make(), su.views()["size_40x24"][0]]
    image_scene = [2, 0, 1, 2, 0]
    pos = np.stack([su.NARROW_POS + 0.01 * np.array([i, -i, 0.5 * i]) for i in range(5)])
    rot = np.stack([su.CAM_ROT @ su.sr.camera_rotation((0.2 * i, -0.3 * i, 5.0 * i)) for i in range(5)])
    together = render(ops, scenes, image_scene, pos, rot, W=40, H=24)
    again = render(ops, scenes, image_scene, pos, rot, W=40, H=24)
    assert all(same(first(together, i), first(again, i)) for i in range(5))
    for i in range(5):
        alone = render(ops, scenes, image_scene[i:i + 1], pos[i:i + 1], rot[i:i + 1], W=40, H=24)
        assert same(first(together, i), first(alone)), i
    empty = first(together, 2)
    assert (empty["rgb"] == su.BACKGROUND).all() and not empty["depth"].any() and (empty["prim"] == -1).all()
    assert not same(first(together, 0), first(together, 3)) and (together["prim"][[0, 1, 3, 4]] >= 0).any(axis=(1, 2)).all()
    F = sum(len(s["faces"]) for s in scenes)
    third = together["prim"][0]                                          # prim indexes the SHARED tables: scene 2's faces come last
    assert third[(third >= 0) & (third < F)].min() >= len(scenes[0]["faces"]) and third.max() >= F + len(scenes[0]["centres"])
    background = render(ops, scenes, [1], W=7, H=5, background=(1, 2, 3), want_prim=False)
    assert set(background) == {"rgb", "depth"} and (background["rgb"] == (1, 2, 3)).all()


def test_lights(ops):
    scene, W, H, pos, yfov = su.views()["sphere_before_triangle"]
    # no light: the ambient term alone, base * 0.3 in fp32, rounded half up
    got = first(render(ops, [scene], lights=np.zeros((0, 4))))
    base = np.concatenate([scene["face_rgb"], scene["sphere_rgb"]]).astype(np.float32)[got["prim"]]
    assert np.array_equal(got["rgb"], np.floor(base * np.float32(0.3) + np.float32(0.5)).astype(np.uint8)) and (got["prim"] >= 0).all()
    # eight lights against the yardstick
    g = np.random.default_rng(8)
    eight = np.concatenate([g.uniform(-1, 1, (8, 2)), g.uniform(0.3, 1.2, (8, 1)), g.uniform(0.2, 0.9, (8, 1))], axis=1)
    got = first(render(ops, [scene], lights=eight))
    su.check(got, su.reference(scene, W, H, pos=pos, yfov=yfov, lights=eight), "eight lights")
    # a light behind the surface adds nothing: on the plane alone (normal +z, towards the camera) one below it changes no bit
    plane = su.fan(1)
    below = np.concatenate([su.LIGHTS[:2], [[0.1, -0.2, -1.0, 50.0]], su.LIGHTS[2:]])
    assert same(first(render(ops, [plane], lights=below)), first(render(ops, [plane])))
    assert not same(first(render(ops, [plane], lights=su.LIGHTS[:3])), first(render(ops, [plane])))
    brighter = first(render(ops, [plane], ambient=0.9))
    assert (brighter["rgb"].astype(int) >= first(render(ops, [plane]))["rgb"]).all() and brighter["rgb"].max() == 255      # clipped


def test_refusals(ops):
    scene = su.views()["size_40x24"][0]
    t = su.pack([scene, su.make()])
    F, S = len(t["faces"]), len(t["centres"])
    device = dict(verts=dev(t["verts"], np.float32), faces=dev(t["faces"], np.int32), face_rgb=dev(t["face_rgb"], np.uint8),
                  centres=dev(t["centres"], np.float32), radii=dev(t["radii"], np.float32), sphere_rgb=dev(t["sphere_rgb"], np.uint8))
    good = dict(device, face_offset=t["face_offset"], sphere_offset=t["sphere_offset"], image_scene=[0, 1], cam_pos=dev(np.tile(su.CAM_POS, (2, 1)),
                np.float32), cam_rot=dev(np.tile(su.CAM_ROT, (2, 1, 1)), np.float32), width=8, height=8)
    before = ops.scene_launches(reset=True)
    assert set(before) == {"calls", "kernels"}
    ops.scene_render(**good)
    assert ops.scene_launches() == {"calls": 1, "kernels": 1}
    for change, words in ((dict(width=0), "W=0"), (dict(height=2049), "H=2049"), (dict(lights=np.ones((9, 4))), "L=9"),
                          (dict(face_offset=[0, F + 1, F + 1]), f"face_offset[2]={F + 1}"), (dict(face_offset=[0, F, F - 1]), "decrease"),
                          (dict(sphere_offset=[-1, S, S]), "sphere_offset[0]=-1"), (dict(sphere_offset=[0, S, S + 2]), f"S={S}"),
                          (dict(image_scene=[0, 2]), "image_scene[1]=2"), (dict(image_scene=[-1, 0]), "image_scene[0]=-1"),
                          (dict(yfov=0.0), "yfov"), (dict(znear=0.0), "znear"), (dict(zfar=0.001), "zfar"), (dict(ambient=float("nan")), "ambient"),
                          (dict(face_offset=dev(t["face_offset"], np.int32)), "host"), (dict(verts=t["verts"]), "GPU"),
                          (dict(face_rgb=device["face_rgb"].float()), "uint8"), (dict(faces=device["faces"].long()), "int32")):
        with pytest.raises(RuntimeError) as e:
            ops.scene_render(**dict(good, **change))
        assert words in str(e.value), (change.keys(), str(e.value))
    for change in (dict(image_scene=[0]), dict(sphere_offset=[0, S]), dict(radii=device["radii"][:-1]), dict(face_rgb=device["face_rgb"][:-1]),
                   dict(cam_rot=good["cam_rot"][:1]), dict(lights=np.ones((2, 3))), dict(background=(1, 2)), dict(face_offset=[0])):
        with pytest.raises(ValueError):
            ops.scene_render(**dict(good, **change))
    assert ops.scene_launches() == {"calls": 1, "kernels": 1}            # nothing of all that was launched


# ---- the renderer classes -------------------------------------------------------------------------------------------------------
def small_objects(tmp_path):
    """Two predicted meshes over one face table, and their ground truths on disk as the reference's data layout has them."""
    verts, faces = su.ico(2, 0.18, centre=(0, 0, 0))["verts"], su.ico(2, 0.18)["faces"]
    meshes = np.stack([verts * np.array([1.0, 0.7, 0.5], np.float32), verts * np.array([0.6, 1.0, 0.8], np.float32) + np.float32(0.02)])
    names = []
    for i in range(2):
        names.append(str(tmp_path / f"object_{i}"))
        truth = su.ico(1 + i, 0.15)
        np.save(names[-1] + "_verts.npy", truth["verts"])
        np.save(names[-1] + "_faces.npy", truth["faces"])
    return meshes.astype(np.float32), faces.astype(np.int64), names


def test_camera_renderer_and_render_representations(ops, tmp_path):
    image_module = pytest.importorskip("PIL.Image")
    from a3vt_amd.pterotactyl.utility import pretty_render, utils
    meshes, faces, names = small_objects(tmp_path)
    locations = [str(tmp_path / f"out_{i}") for i in range(2)]
    for location in locations:
        os.makedirs(location)
    ops.scene_launches(reset=True)
    seed_before = torch.random.get_rng_state()
    out = pretty_render.render_representations(locations, names, meshes, faces, num_points=2000, resolution=(96, 80))
    assert ops.scene_launches() == {"calls": 1, "kernels": 1}            # all six images from one library call
    assert torch.equal(torch.random.get_rng_state(), seed_before)        # looking at a result does not move the run's generator
    assert out["points"].shape == (2, 2000, 3) and len(out["images"]) == 2
    camera = pretty_render.CameraRenderer([96, 80])
    for i in range(2):
        separate = []
        camera.add_object(meshes[i], utils.add_faces(faces))
        separate.append(camera.render())
        camera.remove_objects()
        camera.add_points(out["points"][i], 0.01, ops.RENDER_DEFAULTS["colour"])
        separate.append(camera.render())
        camera.remove_objects()
        camera.add_object(np.load(names[i] + "_verts.npy"), utils.add_faces(np.load(names[i] + "_faces.npy")))
        separate.append(camera.render())
        camera.remove_objects()
        for image, alone, file in zip(out["images"][i], separate, ("mesh.png", "points.png", "ground_truth.png")):
            assert image.shape == (80, 96, 3) and image.dtype == np.uint8 and np.array_equal(image, alone), (i, file)
            assert np.array_equal(np.array(image_module.open(os.path.join(locations[i], file))), image)
            seen = (image != 255).any(axis=-1)
            assert 0.02 < seen.mean() < 0.9                              # the object is in view, on a white background
    assert ops.scene_launches() == {"calls": 7, "kernels": 7}
    assert camera.render().min() == 255                                  # nothing left in the scene
    # the camera can be moved, an object posed, and many scenes go through one call
    camera.add_object(meshes[0], faces, colour=(200, 60, 40), position=[0.05, 0, 0], orientation=[0, 0, 0.5])
    here = camera.render()
    camera.update_camera_pose([0, -0.6, 0.6], utils.euler_matrix([45.0, 0, 0], degrees=True))     # from the other side, at the origin
    moved = camera.scene()
    camera.update_camera_pose(ops.RENDER_DEFAULTS["cam_pos"], utils.euler_matrix(ops.RENDER_DEFAULTS["cam_euler_xyz_deg"], degrees=True))
    both = pretty_render.render_batch([camera.scene(), moved])
    assert np.array_equal(both[0], here) and (here != 255).any() and both[1].shape == here.shape
    with pytest.raises(ValueError):
        pretty_render.render_batch([camera.scene(), pretty_render.CameraRenderer([64, 64]).scene()])


def test_visualize_prediction_writes_the_reference_files(ops, tmp_path):
    pytest.importorskip("PIL.Image")
    from a3vt_amd.pterotactyl.utility import utils
    meshes, faces, names = small_objects(tmp_path)
    ops.scene_launches(reset=True)
    utils.visualize_prediction(str(tmp_path / "results"), torch.from_numpy(meshes).cuda(), torch.from_numpy(faces).cuda(), names)
    assert ops.scene_launches()["calls"] == 1
    for i in range(2):
        for file in ("mesh.png", "points.png", "ground_truth.png"):
            assert os.path.getsize(tmp_path / "results" / f"object_{i}" / file) > 0


def test_the_vision_trainer_visualizes_batch_five(cuda, ops, tmp_path):
    """``Engine.validate`` with ``eval`` and ``visualize`` renders the objects of batches 0 .. 5 after batch 5 (reference
    vision/train.py:193-198); without the flag nothing is written, and the score has the same bits either way."""
    pytest.importorskip("PIL.Image")
    from helpers import make_args
    from a3vt_amd.pterotactyl.reconstruction.vision import train
    from a3vt_amd.synthetic import SyntheticLoader
    os.chdir(tmp_path)
    truth = su.ico(1, 0.15)
    losses, calls = {}, {}
    for flag in (True, False):
        args = make_args(num_GCN_layers=3, hidden_GCN_size=64, number_points=500, exp_type="t", exp_id=f"visualize_{flag}", eval=True,
                         batch_size=2, log_interval=0, visualize=flag)
        loader = SyntheticLoader(args, 7, 2, seed=3)
        for batch in loader:
            for name in batch["names"]:
                np.save(name[0] + "_verts.npy", truth["verts"])
                np.save(name[0] + "_faces.npy", truth["faces"])
        engine = train.Engine(args, loaders=(None, loader))
        engine.setup()
        ops.scene_launches(reset=True)
        with torch.no_grad():
            engine.validate(loader, None)
        losses[flag], calls[flag] = engine.current_loss, ops.scene_launches()["calls"]
        written = sorted(os.listdir(engine.results_dir))
        if flag:
            assert written == sorted(f"synthetic_3_{s}_{i}" for s in range(6) for i in range(2))      # batch 6's objects are not rendered
            for folder in written:
                assert sorted(os.listdir(os.path.join(engine.results_dir, folder))) == ["ground_truth.png", "mesh.png", "points.png"]
        else:
            assert written == []
    assert calls == {True: 1, False: 0}
    assert np.float64(losses[True]).tobytes() == np.float64(losses[False]).tobytes() and np.isfinite(losses[True])
