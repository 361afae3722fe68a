"""GPU tests of ``RenderedSampler``'s vision images: ``sample(vision=True)`` against a direct ``ops.scene_render`` call under
``ops.VISION_DEFAULTS`` bit for bit, and that call against the fp64 caster with ``scene_render_util``'s own rule for decided pixels
(no new tolerance).  The shading is ``scene_render``'s Lambert model: nothing here is compared with an image of pyrender's.

The scene: two icospheres around the origin, where a data set's objects sit — 0.08 and 0.05 in radius, 0.42 from the camera, so each
covers the image's centre and leaves its corners to the background."""
import numpy as np
import pytest
import torch

import scene_render_ref as sr
import scene_render_util as su
from chart_head_util import bake_scene

pytestmark = pytest.mark.gpu

OBJECTS = ("big", "small")
NAMES = [f"/data/object_info/{o}" for o in OBJECTS]
SCENES = {"big": su.ico(2, 0.08), "small": su.ico(1, 0.05, centre=(-0.011, 0.017, 0.006))}
GEOMETRY = {o: (s["verts"], s["faces"]) for o, s in SCENES.items()}


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def direct(ops, colours, pos, rot, W=256, H=256, want_prim=True):
    """The two objects, one image each, straight from ``ops.scene_render`` under ``VISION_DEFAULTS`` -> NumPy arrays."""
    D = ops.VISION_DEFAULTS
    scenes = [su.make(SCENES[o]["verts"], SCENES[o]["faces"], face_rgb=np.asarray(c, np.uint8)) for o, c in zip(OBJECTS, colours)]
    t = su.pack(scenes)
    out = ops.scene_render(dev(t["verts"], np.float32), dev(t["faces"], np.int32), dev(t["face_rgb"], np.uint8), dev(t["centres"], np.float32),
                           dev(t["radii"], np.float32), dev(t["sphere_rgb"], np.uint8), t["face_offset"], t["sphere_offset"], [0, 1],
                           dev(pos, np.float32), dev(rot, np.float32), yfov=D["yfov"], znear=D["znear"], zfar=D["zfar"], width=W, height=H,
                           lights=D["lights"], ambient=D["ambient"], background=D["background"], want_prim=want_prim)
    return {k: v.cpu().numpy() for k, v in out.items()}, scenes


@pytest.fixture(scope="module")
def ops(cuda):
    from a3vt_amd import ops
    return ops


@pytest.fixture(scope="module")
def sampler(ops):
    from a3vt_amd.pterotactyl.policies import rendered
    s = rendered.RenderedSampler({}, GEOMETRY)
    s.load_objects(NAMES)
    return s


def default_camera(ops):
    D = ops.VISION_DEFAULTS
    return np.tile(np.asarray(D["cam_pos"]), (2, 1)), np.tile(sr.camera_rotation(D["cam_euler_xyz_deg"]), (2, 1, 1))


def test_the_images_are_the_direct_call_and_hold_against_fp64(ops, sampler):
    D = ops.VISION_DEFAULTS
    ops.scene_launches(reset=True)
    images = sampler.sample([0, 0], touch=False, vision=True)["vision"]
    assert ops.scene_launches() == {"calls": 1, "kernels": 1}                  # all E images from one call
    pos, rot = default_camera(ops)
    got, scenes = direct(ops, [D["colour"]] * 2, pos, rot)
    assert len(images) == 2
    for i, image in enumerate(images):
        assert isinstance(image, np.ndarray) and image.shape == (256, 256, 3) and image.dtype == np.uint8
        assert np.array_equal(image, got["rgb"][i])
        want = su.reference(scenes[i], 256, 256, pos=pos[i], rot=rot[i], lights=np.asarray(D["lights"]), ambient=D["ambient"],
                            background=D["background"], znear=D["znear"], zfar=D["zfar"], yfov=D["yfov"])
        first_face = sum(len(s["faces"]) for s in scenes[:i])                  # (prim is the face's index in the call's table)
        su.check({k: v[i] for k, v in got.items()}, want, f"vision image of {OBJECTS[i]!r}",
                 prim_map=lambda p: np.where(p >= 0, p - first_face, p))
        centre, corners = got["depth"][i][127:129, 127:129], got["depth"][i][[0, 0, -1, -1], [0, -1, 0, -1]]
        assert (centre > 0).all() and (corners == 0).all()                     # the camera looks at the object, and past it at the rim
        assert (image[[0, 0, -1, -1], [0, -1, 0, -1]] == D["background"]).all() and (image[127:129, 127:129] != D["background"]).any()
        assert abs(float(centre.mean()) - (0.4243 - (0.08, 0.05)[i])) < 0.02    # 0.4243 from the origin, less the radius


def test_parameters_move_the_camera(ops, sampler):
    euler = (60.0, 0.0, 200.0)
    R = sr.camera_rotation(euler)
    position = tuple(0.5 * R[:, 2])                                            # 0.5 behind the origin along the new view direction
    by_euler = sampler.sample([0, 0], touch=False, vision=True, parameters=[(position, euler), None])["vision"]
    by_matrix = sampler.sample([0, 0], touch=False, vision=True, parameters=[(position, R), None])["vision"]
    plain = sampler.sample([0, 0], touch=False, vision=True)["vision"]
    assert np.array_equal(by_euler[0], by_matrix[0]) and np.array_equal(by_euler[1], by_matrix[1])
    assert np.array_equal(by_euler[1], plain[1]) and not np.array_equal(by_euler[0], plain[0])
    pos, rot = default_camera(ops)
    pos[0], rot[0] = position, R
    got, _ = direct(ops, [ops.VISION_DEFAULTS["colour"]] * 2, pos, rot, want_prim=False)
    assert np.array_equal(by_euler[0], got["rgb"][0])
    hit = (by_euler[0] != ops.VISION_DEFAULTS["background"]).any(axis=-1)
    assert hit[127:129, 127:129].all() and hit.sum() < (plain[0] != ops.VISION_DEFAULTS["background"]).any(axis=-1).sum()   # further away


def test_a_colour_per_object_a_resolution_and_device_tensors(ops):
    from a3vt_amd.pterotactyl.policies import rendered
    colours = [[200, 60, 40, 255], [40, 90, 220, 0]]
    s = rendered.RenderedSampler({}, GEOMETRY, object_colours=colours, resolution=[40, 24], to_host=False)
    s.load_objects(NAMES)
    images = s.sample([0, 0], touch=False, vision=True)["vision"]
    pos, rot = default_camera(ops)
    got, _ = direct(ops, [c[:3] for c in colours], pos, rot, W=40, H=24, want_prim=False)
    for i, image in enumerate(images):
        assert isinstance(image, torch.Tensor) and image.is_cuda and image.shape == (24, 40, 3) and image.dtype == torch.uint8
        assert np.array_equal(image.cpu().numpy(), got["rgb"][i])
    lit = [images[i][12, 20].cpu().numpy().astype(int) for i in range(2)]
    assert lit[0][0] > lit[0][2] and lit[1][2] > lit[1][0]                     # red-ish and blue-ish: each object its own colour
    with pytest.raises(NotImplementedError, match="hand model"):
        s.sample([0, 0], vision=True, vision_occluded=True)


def test_a_call_without_vision_is_todays(ops, cuda):
    """On the bake scene: the keys and bits of the result as ``sample_many`` builds it from ``ops.touch_render``'s buffers, with the
    padded read and with the packed one; ``touch=False`` still returns the empty dict."""
    from a3vt_amd.pterotactyl.policies import rendered
    geometry, frames = bake_scene()
    names = ["/data/object_info/ball", "/data/object_info/pebble"]
    kept = []

    def keeping(*a, **k):
        kept.append(ops.touch_render(*a, **k))
        return kept[-1]
    s = rendered.RenderedSampler(frames, geometry, render=keeping, pack=ops.touch_pack, device=cuda)
    s.load_objects(names)
    got = s.sample([0, 1], touch_point_cloud=True, pack_points=False)
    packed = s.sample([0, 1], touch_point_cloud=True, pack_points=True)
    assert set(got) == set(packed) == {"touch_status", "touch_signal", "depths", "finger_transfrom_pos", "finger_transform_rot_M",
                                        "touch_point_cloud"}
    out = kept[0]
    live = [0, 1, 2, 3, 4, 5, 6]                                               # ("ball", 0): four fingers; ("pebble", 1): finger 3 has no frame
    assert torch.equal(got["touch_signal"].reshape(8, 121, 121, 3)[live], out["touch"].cpu()) and not got["touch_signal"][1, 3].any()
    assert torch.equal(got["depths"].reshape(8, 121, 121)[live], out["depth"].cpu())
    count, status = out["count"].cpu().numpy(), out["status"].cpu().numpy()
    for result in (got, packed):
        assert result["touch_status"] == got["touch_status"] and torch.equal(result["touch_signal"], got["touch_signal"])
        for v in live:
            cloud = result["touch_point_cloud"][v // 4][v % 4]
            want = out["points"][v, :count[v] if status[v] == 1 else 0].cpu().numpy()
            assert cloud.dtype == np.float32 and np.array_equal(cloud.view(np.uint32), want.view(np.uint32)), v
        assert result["touch_point_cloud"][1][3].shape == (0, 3)
    assert sum(len(c) for row in got["touch_point_cloud"] for c in row) > 0
    assert s.sample([0, 1], touch=False) == {}
