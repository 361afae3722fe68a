"""``a3vt_touch_render`` / ``a3vt_touch_finish`` (csrc/touch_render.hip) on the GPU against the NumPy emulation
``touch_render_ref`` and the reference's recorded outputs in ``golden/g23_touch_render.npz``.

Depth.  A pixel is *undecided* if the fp64 emulation's depth moves by more than 1e-6 (relative; a hit coming or going counts) when
its three barycentric tests are loosened and tightened by 1e-5; such pixels are left out and may not exceed 0.1 % of an image.
Everywhere else hit / no-hit must agree exactly and the depth within 8 x the largest relative deviation of the FLOAT32 emulation
from the fp64 one on that scene (measured here from the emulation, never from the kernel; 8 because the kernel orders the
arithmetic differently — camera-frame transform first, plane form of the depth — and glancing hits amplify rounding).

Finish.  The fixture's depth maps go to the kernel through ``ops.touch_finish`` (the second launch alone).  Statuses, counts and the
points' order must equal the reference's; touch and points must be within 4 x the deviation of the float32 emulation from the
fixture (the "cap 4" convention of the touch-encoder tests).

Measured on an MI355X (yardstick = the float32 emulation's deviation, then the kernel's; `profiles/touch_render.txt`):
    depth, largest relative deviation on decided pixels    small1 3.2e-6, 2.4e-6 (0 undecided);  small2 5.4e-6, 3.0e-6 (0);
                                                           big 2.9e-7, 1.4e-7 (1);  mid 3.2e-7, 2.5e-7 (0);
                                                           one triangle 2.6e-7, 2.0e-7;  257 faces 3.2e-7, 2.6e-7
    finish, touch (of 255)                                 9.8e-5, 1.34e-4 (worst map; 1.01e-4 on the flat ones)
    finish, points                                         1.10e-8, 1.10e-8
    hit / no-hit mismatches on decided pixels: none; the whole file takes 6 s."""
import os

import numpy as np
import pytest
import torch

import touch_render_ref as tr
import touch_render_util as tu

pytestmark = pytest.mark.gpu
CHUNK = 256            # csrc/kernels.h's kTouchFaceChunk
DEPTH_SCENES = ("small1", "small2", "big", "mid")       # ("straddle" serves the finish stage, through the fixture)


@pytest.fixture(scope="module")
def ops(cuda):
    from a3vt_amd import ops
    return ops


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", tu.FIXTURE))


def emulate(verts, faces, pos=None, rot=None):
    """The yardstick of one view: fp64 depth, the undecided pixels, the float32 emulation's largest relative deviation."""
    pos32, rot32 = tu.frame32()
    pos, rot = (pos32 if pos is None else pos), (rot32 if rot is None else rot)
    loose, exact, tight = tr.cast(verts, faces, pos, rot, margins=(1e-5, 0.0, -1e-5))
    und = tr.undecided(loose, exact, tight)
    single = tr.cast(verts, faces, pos, rot, dtype=np.float32)[0].astype(np.float64)
    both = (exact > 0) & (single > 0) & ~und
    yard = float((np.abs(single - exact)[both] / exact[both]).max()) if both.any() else 0.0
    return dict(depth=exact, undecided=und, yard=yard)


@pytest.fixture(scope="module")
def scenes():
    """Computed once, shared, never changed."""
    return {name: dict(emulate(*tu.scene(name)), mesh=tu.scene(name)) for name in DEPTH_SCENES}


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def render(ops, meshes, image_mesh, pos, rot, **kw):
    """``ops.touch_render`` on a list of (verts, faces) meshes -> the dict, as NumPy arrays."""
    verts = np.concatenate([v for v, _ in meshes]) if meshes else np.zeros((0, 3))
    base = np.cumsum([0] + [len(v) for v, _ in meshes])
    faces = np.concatenate([f.reshape(-1, 3) + b for (_, f), b in zip(meshes, base)])
    offsets = np.cumsum([0] + [len(f) for _, f in meshes])
    out = ops.touch_render(dev(verts, np.float32), dev(faces, np.int32), dev(offsets, np.int32), dev(image_mesh, np.int32),
                           dev(pos, np.float32), dev(rot, np.float32), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def render_one(ops, verts, faces, pos=None, rot=None, **kw):
    pos32, rot32 = tu.frame32()
    return render(ops, [(verts, faces)], [0], (pos32 if pos is None else pos)[None], (rot32 if rot is None else rot)[None], **kw)


def check_depth(got, want, what):
    und, exact = want["undecided"], want["depth"]
    share = und.mean()
    ok = ~und
    mismatch = int(((got > 0) != (exact > 0))[ok].sum())
    both = ok & (got > 0) & (exact > 0)
    worst = float((np.abs(got.astype(np.float64) - exact)[both] / exact[both]).max()) if both.any() else 0.0
    print(f"{what}: hits {int((exact > 0).sum())}, undecided {int(und.sum())}, hit mismatches {mismatch}, yardstick {want['yard']:.3e}, "
          f"kernel {worst:.3e}, depths {exact[exact > 0].min() if (exact > 0).any() else 0:.5f} .. {exact.max():.5f}")
    assert share <= 1e-3, (what, int(und.sum()))
    assert mismatch == 0, what
    assert worst <= 8 * want["yard"], (what, worst, want["yard"])


@pytest.mark.parametrize("name", DEPTH_SCENES)
def test_depth_against_the_emulation(ops, scenes, name):
    """small1 / small2: the silhouette inside the image, background and in-range hits; big: every pixel hits, many rays cross shared
    edges; mid: 1 280 faces, five chunks."""
    got = render_one(ops, *scenes[name]["mesh"])
    check_depth(got["depth"][0], scenes[name], name)
    if name in ("big", "mid"):
        assert (got["depth"][0] > 0).all()              # watertight: no ray leaks through a shared edge to the background
    # the status and the count follow from the kernel's own depth
    d = got["depth"][0]
    contacts = int((d <= np.float32(tr.MAX_DEPTH)).sum()) - int((d == 0).sum())
    assert got["status"][0] == int(contacts > 0) and got["count"][0] == contacts


def test_face_count_edges(ops, scenes):
    pos32, rot32 = tu.frame32()
    eye = np.array([[-0.004, -0.003, -0.02], [0.005, -0.002, -0.018], [0.001, 0.006, -0.022]])
    one = ((eye @ tr.camera_rotation(tu.ROT).T + tu.POS).astype(np.float32), np.array([[0, 1, 2]], np.int32))
    got = render_one(ops, *one)
    check_depth(got["depth"][0], emulate(*one), "one triangle")
    assert 0 < (got["depth"][0] > 0).sum() < tr.PIX

    v, f = scenes["mid"]["mesh"]
    cut = (v, f[:CHUNK + 1])                                                    # one LDS chunk + 1
    got = render_one(ops, *cut)
    check_depth(got["depth"][0], emulate(*cut), "one chunk + 1 faces")

    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))          # a mesh without faces beside one with
    small = scenes["small1"]["mesh"]
    got = render(ops, [empty, small, empty], [0, 1, 2, 1], np.tile(pos32, (4, 1)), np.tile(rot32, (4, 1, 1)))
    assert not got["depth"][[0, 2]].any() and not got["status"][[0, 2]].any() and not got["count"][[0, 2]].any()
    check_depth(got["depth"][1], scenes["small1"], "beside empty meshes")
    assert np.array_equal(got["depth"][1], got["depth"][3])

    behind = rot32 @ tr.euler_xyz(np.array([0.0, 0.0, np.pi])).astype(np.float32)      # the finger looks the other way
    got = render_one(ops, *small, rot=behind)
    assert not got["depth"].any() and got["status"][0] == 0 and got["count"][0] == 0
    assert got["touch"].any()                                                   # (a flat gel image all the same)


def test_what_the_contract_says_about_bad_tables(ops, scenes):
    """``include/a3vt.h``: image_mesh is clamped into [0, M); face_offset entries into [0, F], an end below its start is an empty
    mesh; a face with an index outside [0, V) is skipped.  Straight through ``ops`` (which cannot check device contents)."""
    pos32, rot32 = tu.frame32()
    v, f = scenes["small1"]["mesh"]
    want = render_one(ops, v, f)["depth"][0]
    got = render(ops, [(v, f)], [-5, 7], np.tile(pos32, (2, 1)), np.tile(rot32, (2, 1, 1)))
    assert np.array_equal(got["depth"][0], want) and np.array_equal(got["depth"][1], want)
    bad = f.copy()
    bad[3] = [0, 1, len(v)]
    bad[5] = [-1, 2, 3]
    keep = np.ones(len(f), bool)
    keep[[3, 5]] = False
    assert np.array_equal(render_one(ops, v, bad)["depth"][0], render_one(ops, v, f[keep])["depth"][0])
    args = [dev(v, np.float32), dev(f, np.int32)]
    frame = [dev([0], np.int32), dev(pos32[None], np.float32), dev(rot32[None], np.float32)]
    out = ops.touch_render(*args, dev([-3, len(f) + 100], np.int32), *frame)
    assert np.array_equal(out["depth"][0].cpu().numpy(), want)
    out = ops.touch_render(*args, dev([40, 10], np.int32), *frame)
    assert not out["depth"].any()


def batch(scenes, n):
    pos32, rot32 = tu.frame32()
    meshes = [scenes["small1"]["mesh"], scenes["small2"]["mesh"]]
    image_mesh = np.arange(n) % 2
    pos = pos32 + 0.0004 * np.arange(n)[:, None].astype(np.float32) * np.array([1.0, -0.5, 0.25], np.float32)
    rot = np.stack([rot32 @ tr.euler_xyz(np.array([0.02 * i, -0.03 * i, 0.5 * i])).astype(np.float32) for i in range(n)])
    return meshes, image_mesh, pos, rot


def same(a, b, i, j=0):
    n = int(a["count"][i])
    return (all(np.array_equal(a[k][i].view(np.uint32) if a[k].dtype == np.float32 else a[k][i], b[k][j].view(np.uint32)
                               if b[k].dtype == np.float32 else b[k][j]) for k in ("depth", "touch", "status", "count"))
            and np.array_equal(a["points"][i, :n].view(np.uint32), b["points"][j, :n].view(np.uint32)))


@pytest.mark.parametrize("n", [1, 4, 9])
def test_an_image_does_not_depend_on_its_batch(ops, scenes, n):
    meshes, image_mesh, pos, rot = batch(scenes, n)
    together = render(ops, meshes, image_mesh, pos, rot)
    assert together["count"].max() > 0
    for i in range(n):
        alone = render(ops, meshes, image_mesh[i:i + 1], pos[i:i + 1], rot[i:i + 1])
        assert same(together, alone, i), i


def test_a_second_run_gives_the_same_bits(ops, scenes):
    meshes, image_mesh, pos, rot = batch(scenes, 4)
    a, b = render(ops, meshes, image_mesh, pos, rot), render(ops, meshes, image_mesh, pos, rot)
    assert all(same(a, b, i, i) for i in range(4))
    partial = render(ops, meshes, image_mesh, pos, rot, want_touch=False, want_points=False)
    assert set(partial) == {"depth", "status"} and np.array_equal(partial["depth"], a["depth"]) and np.array_equal(partial["status"], a["status"])


def test_finish_against_the_reference(ops, golden):
    n = len(golden["names"])
    pos, rot = np.tile(golden["pos"], (n, 1)), np.tile(golden["rot"], (n, 1, 1))
    out = ops.touch_finish(dev(golden["depth"], np.float32), dev(pos, np.float32), dev(rot, np.float32))
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert np.array_equal(got["status"], golden["status"]) and np.array_equal(got["count"], golden["count"])
    # the float32 emulation on the same float32 frames: the yardstick
    _, touch32, points32 = tr.finish(golden["depth"], pos.astype(np.float32), rot.astype(np.float32), dtype=np.float32)
    yard_touch = float(np.abs(touch32[:, tu.ROWS].astype(np.float64) - golden["touch"]).max())
    kernel_touch = np.abs(got["touch"][:, tu.ROWS].astype(np.float64) - golden["touch"]).max(axis=(1, 2, 3))
    stored = [tu.stored_points(c) for c in golden["count"]]
    want_points = golden["points"]
    mine32 = np.concatenate([p[s] for p, s in zip(points32, stored)]).astype(np.float64)
    mine = np.concatenate([got["points"][i, :c][s] for i, (c, s) in enumerate(zip(golden["count"], stored))]).astype(np.float64)
    yard_points, kernel_points = float(np.abs(mine32 - want_points).max()), float(np.abs(mine - want_points).max())
    print(f"finish: touch yardstick {yard_touch:.3e} (of 255), kernel per map {dict(zip(golden['names'], kernel_touch))}; "
          f"points yardstick {yard_points:.3e}, kernel {kernel_points:.3e}")
    assert kernel_touch.max() <= 4 * yard_touch
    assert kernel_points <= 4 * yard_points                # (a point out of order would be off by a pixel's width, 1e-4)


def test_the_sampler_on_the_gpu_against_the_emulated_one(ops, scenes):
    """The whole path: ``RenderedSampler`` with the library against ``RenderedSampler(render=emulation)`` on the same frames: depth
    by the rule above; touch and points against the fp64 finish of the sampler's OWN depth maps within 4 x the float32
    emulation's deviation on them; ``sample_many`` bit-equal to its ``sample`` calls."""
    from a3vt_amd.pterotactyl.policies import rendered
    geometry = {"small1": scenes["small1"]["mesh"], "small2": scenes["small2"]["mesh"]}
    pos, rot = np.tile(tu.POS, (4, 1)), np.tile(tu.ROT, (4, 1, 1))
    frames = {(o, 0): (pos, rot, np.array([True, False, False, True])) for o in geometry}
    frames[("small1", 1)] = (pos + 0.0003, rot, np.ones(4, bool))
    names = [f"/data/object_info/{o}" for o in geometry]
    fast, slow = rendered.RenderedSampler(frames, geometry), rendered.RenderedSampler(frames, geometry, render=tr.render)
    fast.load_objects(names)
    slow.load_objects(names)
    got, want = fast.sample([0, 0], touch_point_cloud=True), slow.sample([0, 0], touch_point_cloud=True)
    assert got["touch_status"] == want["touch_status"] == [["touch", "no_intersection", "no_intersection", "touch"]] * 2
    assert got["touch_signal"].device.type == "cpu" and got["depths"].dtype == torch.float32
    for key in ("finger_transfrom_pos", "finger_transform_rot_M"):
        assert torch.equal(got[key], want[key])
    pos32, rot32 = tu.frame32()
    for e, name in enumerate(geometry):
        for f in (0, 3):
            d = got["depths"][e, f].numpy()
            check_depth(d, scenes[name], f"sampler {name} finger {f}")
            assert np.array_equal(want["depths"][e, f].numpy(), scenes[name]["depth"].astype(np.float32))
            _, touch64, points64 = tr.finish_one(d, pos32, rot32)
            _, touch32, points32 = tr.finish_one(d, pos32, rot32, dtype=np.float32)
            cloud = got["touch_point_cloud"][e][f]
            assert cloud.shape == points64.shape
            assert np.abs(got["touch_signal"][e, f].numpy() - touch64).max() <= 4 * np.abs(touch32 - touch64).max()
            assert np.abs(cloud - points64).max() <= 4 * np.abs(points32 - points64).max()
        for f in (1, 2):
            assert not got["depths"][e, f].any() and not got["touch_signal"][e, f].any() and len(got["touch_point_cloud"][e][f]) == 0
    lists = [[0, 0], [1, 0], [5, 1]]
    many = fast.sample_many(lists, touch_point_cloud=True)
    for result, actions in zip(many, lists):
        single = fast.sample(actions, touch_point_cloud=True)
        assert result["touch_status"] == single["touch_status"]
        for key in ("touch_signal", "depths", "finger_transfrom_pos", "finger_transform_rot_M"):
            assert torch.equal(result[key], single[key]), key
        for a, b in zip(result["touch_point_cloud"], single["touch_point_cloud"]):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
    on_device = rendered.RenderedSampler(frames, geometry, to_host=False)
    on_device.load_objects(names)
    kept = on_device.sample([0, 0])
    assert kept["touch_signal"].is_cuda and torch.equal(kept["touch_signal"].cpu(), got["touch_signal"])
