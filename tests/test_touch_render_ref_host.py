"""CPU tests of the emulation ``touch_render_ref`` itself (the yardstick of ``test_gpu_touch_render.py``): its finish stage against
the REFERENCE's ``render_depth`` / ``depth_to_touch`` / ``depth_to_points`` as recorded in ``golden/g23_touch_render.npz``, and its
ray caster against closed forms."""
import os

import numpy as np
import pytest

import touch_render_ref as tr
import touch_render_util as tu


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", tu.FIXTURE))


def test_the_fixture_holds_what_the_generator_describes(golden):
    assert list(golden["names"]) == list(tu.CAST_MAPS + tu.HAND_MAPS)
    assert golden["depth"].dtype == np.float32 and golden["touch"].shape == (6, len(tu.ROWS), tr.RES, 3)
    for i, name in enumerate(tu.HAND_MAPS, start=len(tu.CAST_MAPS)):
        assert np.array_equal(golden["depth"][i], tu.hand_map(name)), name
    by = dict(zip(golden["names"], zip(golden["status"], golden["count"])))
    assert by["empty"] == (0, 0) and by["beyond"] == (0, 0)
    assert by["threshold"] == (1, 1)                       # float32(0.025) <= max_depth as a float32 comparison; one ulp above is not
    assert by["corner"][0] == 1 and by["small1"][0] == 1 and 0 < by["straddle"][1] < tr.PIX
    assert len(golden["points"]) == sum(len(tu.stored_points(c)) for c in golden["count"])


def test_finish_matches_the_reference(golden):
    n = len(golden["names"])
    status, touch, points = tr.finish(golden["depth"], [golden["pos"]] * n, [golden["rot"]] * n)
    assert np.array_equal(status, golden["status"])
    assert [len(p) for p in points] == list(golden["count"])
    err = np.abs(touch[:, tu.ROWS] - golden["touch"]).max(axis=(1, 2, 3))
    print("touch: max |emulation - reference| per map", dict(zip(golden["names"], err)))
    assert err.max() <= 1e-9 * 255
    mine = np.concatenate([p[tu.stored_points(len(p))] for p in points])       # (the order is part of the result)
    perr = np.abs(mine - golden["points"]).max()
    print(f"points: max |emulation - reference| {perr:.3e}")
    assert perr <= 1e-12


def test_float32_finish_stays_close(golden):
    """The float32 evaluation is a yardstick's other half: it must agree in everything discrete."""
    n = len(golden["names"])
    status, touch, points = tr.finish(golden["depth"], [golden["pos"]] * n, [golden["rot"]] * n, dtype=np.float32)
    assert touch.dtype == np.float32 and points[0].dtype == np.float32
    assert np.array_equal(status, golden["status"]) and [len(p) for p in points] == list(golden["count"])
    assert np.abs(touch[:, tu.ROWS] - golden["touch"]).max() < 0.05          # (of 255)


def view(rot, yfov=tr.YFOV):
    """Eye-frame ray directions (121, 121, 3) by the contract's formula, written out here on purpose."""
    t = np.tan(yfov / 2)
    c = (np.arange(tr.RES) + 0.5) / tr.RES * 2 - 1
    return np.stack(np.broadcast_arrays(c[None, :] * t, -c[:, None] * t, -1.0), -1)


def quad(corners):
    return np.array(corners, np.float64), np.array([[0, 1, 2], [0, 2, 3]])


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-12), (np.float32, 2e-5)])
def test_plane_facing_the_camera_and_tilted(dtype, tol):
    """An eye-frame plane n . p = h: depth = h / (n . d) for the ray d = (x, y, -1).  Built in the eye frame, moved to the world."""
    C = tr.camera_rotation(tu.ROT)
    d = view(tu.ROT)
    for normal, h in (((0.0, 0.0, -1.0), 0.02), ((0.3, -0.2, -1.0), 0.02)):
        normal = np.array(normal)
        # ONE big triangle in the plane (no shared edge: in float32 a ray along one may miss both faces), z from the plane equation
        eye = np.array([[x, y, 0.0] for x, y in ((-3, -1), (3, -1), (0, 3))])
        eye[:, 2] = (h - normal[0] * eye[:, 0] - normal[1] * eye[:, 1]) / normal[2]
        verts, faces = eye @ C.T + tu.POS, np.array([[0, 1, 2]])
        got = tr.cast(verts, faces, tu.POS, tu.ROT, dtype=dtype)[0]
        want = h / (d @ normal)
        assert got.dtype == dtype and (got > 0).all()
        assert np.abs(got - want).max() <= tol * want.max(), (normal, np.abs(got - want).max())


@pytest.mark.parametrize("dtype,tol", [(np.float64, 3e-5), (np.float32, 3e-5)])
def test_sphere(dtype, tol):
    """A level-3 icosphere against the sphere it is inscribed in: no hit outside the sphere's silhouette, and inside it the depth
    is the sphere's own up to the facets' sagitta.  An edge subtends 63.4 / 8 = 7.9 degrees = 0.138 rad, up to about 0.165 after
    the subdivision's unequal thirds; a facet's middle is then at most 0.165 / sqrt(3) = 0.095 rad from its corners and
    r (1 - cos 0.095) = 4.5e-3 r = 1.8e-5 inside the sphere.  Along a ray that meets the surface at an angle whose cosine is at
    least sqrt(0.5) (the rim is left out: the squared cosine is the discriminant over its value on the axis) that is at most
    2.6e-5 of depth: the bound is 3e-5, of depths 0.011 .. 0.015."""
    from a3vt_amd import mesh
    radius, ahead = 0.004, 0.015
    v, f = mesh.icosphere(3, radius)
    verts = v.astype(np.float64) + tu.POS + ahead * tu.ROT[:, 0]
    got = tr.cast(verts, f, tu.POS, tu.ROT, dtype=dtype)[0].astype(np.float64)
    d = view(tu.ROT)
    a, b, c = (d * d).sum(-1), -2 * ahead * -d[..., 2], ahead * ahead - radius * radius      # |t d - (0, 0, -ahead)|^2 = r^2
    disc = b * b - 4 * a * c
    assert not (got[disc < 0] > 0).any()
    inner = disc > 0.5 * disc.max()
    want = (-b[inner] - np.sqrt(disc[inner])) / (2 * a[inner])
    assert (got[inner] > 0).all()
    assert np.abs(got[inner] - want).max() <= tol, np.abs(got[inner] - want).max()
    assert (got[inner] >= want - 1e-9).all()                      # the inscribed mesh is never nearer than the sphere


def test_range_and_sidedness():
    """Nearest hit within [znear, zfar] only; both windings are seen; an object behind the camera is not."""
    C = tr.camera_rotation(tu.ROT)
    def plane(z, flip=False):
        # (lopsided: a square's diagonal would run through pixel centres, where either face may claim or miss the ray by rounding)
        eye = np.array([[-1, -1.3, -z], [1, -1, -z], [1.2, 1, -z], [-1, 1.1, -z]], np.float64)
        verts, faces = quad(eye @ C.T + tu.POS)
        return verts, faces[:, ::-1] if flip else faces
    for flip in (False, True):
        assert np.allclose(tr.cast(*plane(0.02, flip), tu.POS, tu.ROT)[0], 0.02, rtol=1e-12)
    assert not tr.cast(*plane(-0.02), tu.POS, tu.ROT)[0].any()
    assert not tr.cast(*plane(0.02), tu.POS, tu.ROT, znear=0.03)[0].any()
    assert not tr.cast(*plane(0.02), tu.POS, tu.ROT, zfar=0.01)[0].any()
    near, far = plane(0.02), plane(0.05)
    both = np.concatenate([far[0], near[0]]), np.concatenate([far[1], near[1] + 4])
    assert np.allclose(tr.cast(*both, tu.POS, tu.ROT)[0], 0.02, rtol=1e-12)
    assert np.allclose(tr.cast(*both, tu.POS, tu.ROT, znear=0.03)[0], 0.05, rtol=1e-12)
