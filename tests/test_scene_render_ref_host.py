"""CPU tests of the scene-render emulation ``scene_render_ref`` (the yardstick of ``test_gpu_scene_render.py``) on cases that can be
solved by hand, and of the views those GPU tests use: the fp64 reference alone must leave at most 0.1 % of each undecided."""
import numpy as np
import pytest

import scene_render_ref as sr
import scene_render_util as su

EYE = np.eye(3)
ORIGIN = np.zeros(3)
YFOV = float(np.float32(60.0 / 180.0 * np.pi))         # (the C ABI takes a float, and the emulation rounds as it does)
HEAD_LIGHT = np.array([[0.0, 0.0, 0.0, 1.8]])          # at the camera
BASE = np.array([228, 217, 111])


def image(scene, W, H, pos=ORIGIN, rot=EYE, lights=HEAD_LIGHT, ambient=0.3, znear=0.01, zfar=10.0, **kw):
    return sr.render_image(scene["verts"], scene["faces"], scene["face_rgb"], scene["centres"], scene["radii"], scene["sphere_rgb"], pos, rot,
                           YFOV, znear, zfar, W, H, lights, ambient, (255, 255, 255), **kw)


def level(x):
    return np.floor(np.clip(x, 0, 255) + 0.5).astype(np.uint8)


def test_one_sphere_on_the_axis():
    d, r = 2.0, 0.5
    out = image(su.make(centres=[[0, 0, -d]], radii=[r], sphere_rgb=BASE), 5, 5)
    depth, rgb, prim = out["depth"][0], out["rgb"][0], out["prim"][0]
    # the middle pixel's ray is the axis: the hit is at d - r, the normal faces the light at the eye, |l| = d - r
    assert abs(depth[2, 2] - (d - r)) <= 1e-15 and prim[2, 2] == 0
    assert np.array_equal(rgb[2, 2], level(BASE * (0.3 + 1.8 / np.pi / (d - r) ** 2)))
    # every pixel: the textbook quadratic |t D - c|^2 = r^2 in the ray parameter t, which IS the depth (D = (x, y, -1))
    t = np.tan(YFOV / 2)
    c = np.array([0, 0, -d])
    for row in range(5):
        for col in range(5):
            D = np.array([((col + 0.5) / 5 * 2 - 1) * t, (1 - (row + 0.5) / 5 * 2) * t, -1.0])
            disc = (D @ c) ** 2 - (D @ D) * (c @ c - r * r)
            if disc < 0:
                assert depth[row, col] == 0 and prim[row, col] == -1 and np.array_equal(rgb[row, col], [255, 255, 255])
                continue
            want = (D @ c - np.sqrt(disc)) / (D @ D)
            assert abs(depth[row, col] - want) <= 1e-12 * want and prim[row, col] == 0
            p = want * D
            n, l = (p - c) / r, -p
            shade = 0.3 + 1.8 / np.pi * max(0.0, n @ l / np.linalg.norm(l)) / (l @ l)
            assert np.abs(rgb[row, col].astype(int) - level(BASE * shade).astype(int)).max() <= 1     # (a level's edge may round apart)
    assert 0 < (prim == 0).sum() < 25
    # no runner-up anywhere: one primitive
    assert np.isinf(out["second"]).all() and (out["second_prim"] == -1).all()


def test_a_ray_that_starts_inside_a_sphere_misses_it():
    out = image(su.make(centres=[[0, 0, -0.2]], radii=[0.5]), 5, 5)
    assert (out["prim"] == -1).all() and not out["depth"].any()
    out = image(su.make(centres=[[0, 0, 0.8]], radii=[0.5]), 5, 5)          # behind the camera
    assert (out["prim"] == -1).all()


def test_one_triangle_facing_the_camera():
    tri = np.array([[-1.0, -0.8, -2.0], [1.2, -0.6, -2.0], [0.1, 1.1, -2.0]])
    out = image(su.make(tri, [[0, 1, 2]], face_rgb=BASE), 9, 7)
    depth, prim, rgb = out["depth"][0], out["prim"][0], out["rgb"][0]
    t = np.tan(YFOV / 2)
    hits = 0
    for row in range(7):
        for col in range(9):
            x, y = ((col + 0.5) / 9 * 2 - 1) * t * 9 / 7 * 2, (1 - (row + 0.5) / 7 * 2) * t * 2      # where the ray meets z = -2
            edge = [(tri[(k + 1) % 3, 0] - tri[k, 0]) * (y - tri[k, 1]) - (tri[(k + 1) % 3, 1] - tri[k, 1]) * (x - tri[k, 0]) for k in range(3)]
            inside = all(e > 0 for e in edge)
            assert (prim[row, col] == 0) == inside
            if inside:
                hits += 1
                assert abs(depth[row, col] - 2.0) <= 1e-15               # the ray parameter is -z of the hit
                p = np.array([x, y, -2.0])
                shade = 0.3 + 1.8 / np.pi * (2.0 / np.linalg.norm(p)) / (p @ p)
                assert np.abs(rgb[row, col].astype(int) - level(BASE * shade).astype(int)).max() <= 1
    assert 0 < hits < 63


def test_the_lowest_index_wins_a_tie_and_the_normal_turns_to_the_eye():
    tri = np.array([[-1.0, -0.8, -2.0], [1.2, -0.6, -2.0], [0.1, 1.1, -2.0]])
    faces = np.array([[0, 1, 2], [0, 2, 1], [2, 1, 0]])                      # add_faces' three copies: both windings
    colours = np.array([[200, 60, 40], [40, 90, 220], [30, 160, 70]], np.uint8)
    out = image(su.make(tri, faces, face_rgb=colours), 9, 7)
    hit = out["prim"][0] >= 0
    assert hit.any() and (out["prim"][0][hit] == 0).all()
    assert (out["second_prim"][0][hit] == 1).all() and np.array_equal(out["second"][0][hit], out["depth"][0][hit])
    for order in ([1, 0, 2], [2, 1, 0]):
        other = image(su.make(tri, faces[order], face_rgb=colours[order]), 9, 7)
        assert np.array_equal(other["depth"], out["depth"]) and (other["prim"][0][hit] == 0).all()
        # the winner's colour is the first face's, whichever it is; the shade is the same, for the normal is turned to the eye
        ratio = other["rgb"][0][hit].astype(float) / colours[order[0]] - out["rgb"][0][hit].astype(float) / colours[0]
        assert np.abs(ratio).max() <= 0.5 / colours.min() * 2
    single = [image(su.make(tri, faces[k:k + 1], face_rgb=BASE), 9, 7) for k in range(3)]
    for s in single[1:]:
        assert np.array_equal(s["rgb"], single[0]["rgb"]) and np.array_equal(s["normal"], single[0]["normal"])
    assert (single[0]["normal"][0][hit] @ np.array([0, 0, 1.0]) > 0.999).all()       # towards the eye at the origin: +z
    # coincident copies of one colour are decided pixels; of different colours they are not
    wide = image(su.make(tri, faces, face_rgb=BASE), 9, 7, margins=sr.MARGINS)
    assert not sr.undecided(wide).any()
    wide = image(su.make(tri, faces, face_rgb=colours), 9, 7, margins=sr.MARGINS)
    assert np.array_equal(sr.undecided(wide), hit)


def test_margins_range_and_bad_data():
    scene = su.merge(su.ico(2, 0.3, centre=(0.01, -0.02, -1.5)), su.make(centres=[[0.5, 0.4, -1.4], [-0.5, 0.3, -1.2]], radii=[0.2, 0.15]))
    out = image(scene, 64, 48, margins=(1e-2, 0.0, -1e-2))
    n = (out["prim"] >= 0).sum(axis=(1, 2))
    assert n[0] > n[1] > n[2] > 0
    exact = image(scene, 64, 48)
    assert 0 < sr.undecided(image(scene, 64, 48, margins=sr.MARGINS)).sum() < 0.2 * 64 * 48   # (large spheres: their rims are undecided)
    # the depth range: nothing nearer than znear or farther than zfar is hit
    near = image(scene, 64, 48, znear=1.3)
    assert ((near["depth"] == 0) | (near["depth"] >= 1.3)).all() and (near["depth"] > 0).any() and (near["prim"] != exact["prim"]).any()
    far = image(scene, 64, 48, zfar=1.3)
    assert (far["depth"] <= 1.3).all() and (far["depth"] > 0).any()
    # a NaN vertex, an infinite centre, a zero radius: as if the primitive were not there
    bad = {k: v.copy() for k, v in scene.items()}
    bad["verts"][scene["faces"][5, 1]] = np.nan
    touched = (scene["faces"] == scene["faces"][5, 1]).any(axis=1)
    bad["centres"][0, 2] = np.inf
    bad["radii"][1] = 0.0
    got = image(bad, 64, 48)
    keep = su.make(scene["verts"], scene["faces"][~touched], face_rgb=scene["face_rgb"][~touched])
    want = image(keep, 64, 48)
    assert np.array_equal(got["depth"], want["depth"]) and np.array_equal(got["rgb"], want["rgb"])
    # the float32 emulation stays close to the fp64 one
    single = image(scene, 64, 48, dtype=np.float32)
    both = (single["prim"][0] == exact["prim"][0]) & (exact["prim"][0] >= 0)
    assert both.sum() > 200 and np.abs(single["depth"][0][both] / exact["depth"][0][both] - 1).max() < 1e-4


def test_shared_tables_and_empty_scenes():
    a, b = su.ico(1, 0.2, centre=(0, 0, -1.5)), su.make(centres=[[0.1, 0, -1.2]], radii=[0.1])
    t = su.pack([a, su.make(), b])
    pos, rot = np.zeros((3, 3)), np.tile(EYE, (3, 1, 1))
    out = sr.render(t["verts"], t["faces"], t["face_rgb"], t["centres"], t["radii"], t["sphere_rgb"], t["face_offset"], t["sphere_offset"],
                    [2, 1, 0], pos, rot, YFOV, 0.01, 10.0, 16, 16, HEAD_LIGHT, 0.3, (9, 8, 7))
    assert set(np.unique(out[0]["prim"])) == {-1, len(t["faces"])}                       # the sphere: F + 0
    assert (out[1]["prim"] == -1).all() and not out[1]["depth"].any() and (out[1]["rgb"] == [9, 8, 7]).all()
    assert out[2]["prim"].max() < len(a["faces"]) and (out[2]["prim"] >= 0).any()


@pytest.mark.parametrize("name", sorted(su.views()))
def test_the_views_of_the_gpu_tests_are_decided(name):
    want = su.view_reference(name)
    share = want["undecided"].mean()
    print(f"{name}: {int(want['undecided'].sum())} of {want['undecided'].size} pixels undecided, hits {int((want['depth'] > 0).sum())}, "
          f"float32 emulation's depth deviation {want['yard']:.3e}")
    assert share <= 1e-3
    assert (want["depth"] > 0).any()
    if name.startswith(("faces_", "mixed_")):
        assert (want["depth"] > 0).all()                                # a full-image mesh: the watertight check means something
    if name == "sphere_before_triangle":
        assert (want["prim"] == 1).any() and (want["prim"] == 0).any()
    if name == "triangle_before_sphere":
        assert (want["prim"] == 0).any() and not (want["prim"] == 1).any()   # hidden behind the lid, as seen from this camera
