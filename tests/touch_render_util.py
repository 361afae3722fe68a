"""What the rendered-touch tests and ``golden/make_golden_touch_render.py`` must build alike: the scenes, the hand-made depth maps
of the fixture ``g23_touch_render.npz`` and the rows of it that are stored.

A scene is a ``mesh.icosphere`` seen from a finger frame rotated by xyz Euler angles (0.3, -0.7, 1.1) and moved to
(0.1, -0.05, 0.2); the camera looks along the finger's +x and the sphere's centre lies that way, ``ahead`` of the finger.  The sphere
itself keeps the world's axes: turned with the finger, the icosahedron's edges in its coordinate planes would run exactly along the
image's middle row and column, and all 121 rays of each would pass through an edge (a whole line of "undecided" pixels that says
nothing about a ray caster)."""
import numpy as np

import touch_render_ref as tr
from a3vt_amd import mesh

FIXTURE = "g23_touch_render.npz"
EULER = (0.3, -0.7, 1.1)
POS = np.array([0.1, -0.05, 0.2])
ROT = tr.euler_xyz(np.array(EULER))
# name -> (icosphere level, radius, distance of the centre ahead of the finger)
# "straddle": every pixel hits and the depths run 0.022 .. 0.028, on both sides of max_depth
SCENES = {"small1": (1, 0.004, 0.015), "small2": (2, 0.004, 0.015), "big": (2, 0.05, 0.06), "mid": (3, 0.03, 0.045),
          "straddle": (3, 0.02, 0.042)}
# the fixture's maps: two cast ones and the hand-made ones
CAST_MAPS = ("small1", "straddle")
HAND_MAPS = ("empty", "beyond", "threshold", "corner")
# touch rows kept in the fixture (float64 images are its bulk): the first and last 8 in full — with all their columns — and every
# third between
ROWS = np.array(sorted(set(range(8)) | set(range(tr.RES - 8, tr.RES)) | set(range(8, tr.RES - 8, 3))))


def stored_points(n):
    """Indices of a cloud of n points that the fixture keeps: the first and last 64 and every fourth between."""
    i = np.arange(n)
    return i[(i < 64) | (i >= n - 64) | (i % 4 == 0)]


def scene(name, rot=ROT, pos=POS):
    """(verts (V, 3) float32 in the world frame, faces (F, 3) int32) of a named scene."""
    level, radius, ahead = SCENES[name]
    v, f = mesh.icosphere(level, radius)
    return (v.astype(np.float64) + np.asarray(pos) + ahead * np.asarray(rot)[:, 0]).astype(np.float32), f.astype(np.int32)


def frame32():
    """The scenes' finger frame as the library gets it: (pos (3,), rot (3, 3)) float32."""
    return POS.astype(np.float32), ROT.astype(np.float32)


def hand_map(name):
    """A hand-made float32 depth map (121, 121)."""
    md = np.float32(tr.MAX_DEPTH)
    d = np.zeros((tr.RES, tr.RES), np.float32)
    if name == "beyond":                     # everything hit, nothing within the gel's reach
        d[:] = np.linspace(0.03, 0.2, tr.PIX, dtype=np.float32).reshape(tr.RES, tr.RES)
    elif name == "threshold":                # the only observed pixel sits exactly on float32(max_depth): "touch", yet flat
        d[60, 60] = md
        d[10, 100] = np.nextafter(md, np.float32(1))      # one ulp beyond: out of range
    elif name == "corner":                   # contact only in two corners: the reflect boundary and the one-sided gradient rows
        r, c = np.mgrid[0:tr.RES, 0:tr.RES].astype(np.float32)
        bowl = np.float32(0.012) + np.float32(2e-5) * (r * r + np.float32(0.7) * c * c) + np.float32(3e-4) * np.sin(r + 2 * c)
        d[:6, :5] = bowl[:6, :5]
        d[-4:, -9:] = bowl[:4, :9][::-1, ::-1] + np.float32(0.004)
        d[-1, 0] = np.float32(0.02)
    elif name != "empty":
        raise KeyError(name)
    return d
