"""What the scene-render tests build alike: scenes, their packing into ``a3vt_scene_render``'s tables, and the yardstick.

A scene is a dict ``verts (V, 3) float32, faces (F, 3) int32 (local indices), face_rgb (F, 3) uint8, centres (S, 3) float32,
radii (S,) float32, sphere_rgb (S, 3) uint8``.  Icospheres are turned by generic Euler angles and moved off the origin: kept on the
world's axes, their edges in the plane x = 0 would project onto the middle column of an image of odd width, whose rays would all run
through an edge (a line of "undecided" pixels that says nothing about a ray caster; ``touch_render_util`` has the same care).

The yardstick (the protocol of ``test_gpu_touch_render.py``): ``reference(...)`` renders one view in fp64 at the margins
(+1e-5, 0, -1e-5) and in float32; ``undecided`` pixels (``scene_render_ref.undecided``) are left out and may not exceed 0.1 % of an
image; on the rest ``prim`` is equal, no hit is missed or invented, the relative depth error is at most 8 x the float32 emulation's own
against fp64, and every colour channel is within one level of the fp64 image."""
import numpy as np

import scene_render_ref as sr
from a3vt_amd import mesh

YFOV, ZNEAR, ZFAR = 60.0 / 180.0 * np.pi, 0.01, 10.0
CAM_POS = np.array([0.0, 0.6, 0.6])
CAM_ROT = sr.camera_rotation((45.0, 0.0, 180.0))
LIGHTS = np.array([[0.0, -0.8, 0.3, 1.8], [0.0, 0.8, 0.3, 1.8], [-1.0, 0.0, 1.0, 1.8], [1.0, 0.0, 1.0, 1.8]])
AMBIENT, BACKGROUND = 0.3, (255, 255, 255)
# the close-up camera of the scenes with spheres: the same direction from 1.98 away, seeing +-0.05 around the origin
NARROW_POS, NARROW_YFOV = np.array([0.0, 1.4, 1.4]), 2 * np.arctan(0.025)
TURN = sr.camera_rotation(tuple(np.degrees([0.3, -0.7, 1.1])))
PALETTE = np.array([[228, 217, 111], [200, 60, 40], [40, 90, 220], [30, 160, 70], [250, 250, 250], [90, 20, 140]], np.uint8)


def make(verts=None, faces=None, face_rgb=None, centres=None, radii=None, sphere_rgb=None):
    verts = np.zeros((0, 3)) if verts is None else verts
    faces = np.zeros((0, 3)) if faces is None else faces
    centres = np.zeros((0, 3)) if centres is None else centres
    radii = np.zeros(0) if radii is None else radii
    faces, centres = np.asarray(faces, np.int32).reshape(-1, 3), np.asarray(centres, np.float32).reshape(-1, 3)
    face_rgb = PALETTE[np.arange(len(faces)) % len(PALETTE)] if face_rgb is None else face_rgb
    sphere_rgb = PALETTE[(np.arange(len(centres)) + 2) % len(PALETTE)] if sphere_rgb is None else sphere_rgb
    return dict(verts=np.asarray(verts, np.float32).reshape(-1, 3), faces=faces,
                face_rgb=np.broadcast_to(np.asarray(face_rgb, np.uint8), (len(faces), 3)).copy(), centres=centres,
                radii=np.asarray(radii, np.float32).reshape(-1),
                sphere_rgb=np.broadcast_to(np.asarray(sphere_rgb, np.uint8), (len(centres), 3)).copy())


def merge(a, b):
    """Both scenes' primitives in one scene (a's first)."""
    return make(np.concatenate([a["verts"], b["verts"]]), np.concatenate([a["faces"], b["faces"] + len(a["verts"])]),
                np.concatenate([a["face_rgb"], b["face_rgb"]]), np.concatenate([a["centres"], b["centres"]]),
                np.concatenate([a["radii"], b["radii"]]), np.concatenate([a["sphere_rgb"], b["sphere_rgb"]]))


def ico(level, radius=0.2, centre=(0.013, -0.021, 0.008), **kw):
    v, f = mesh.icosphere(level, radius)
    return make(v.astype(np.float64) @ TURN.T + np.asarray(centre), f, **kw)


def fan(n, radius=0.3):
    """n faces in the plane z = 0 that cover the disc of radius 0.15 at least, more than the NARROW camera sees: one huge
    triangle (n = 1) or a fan of n >= 3 triangles around an off-centre hub.  Every inner edge is shared by
    vertex index: a ray that sees the background has leaked through one.  (The radius is no larger than it must be: a barycentric
    margin of 1e-5 is 1e-5 radius / rho of a sliver's width at the distance rho from the hub, the share of undecided pixels there.)"""
    if n == 0:
        return make()
    if n == 1:
        return make([[-20, -12, 0], [20, -12, 0], [0, 25, 0]], [[0, 1, 2]])
    assert n >= 3
    a = 2 * np.pi * (np.arange(n) + 0.137) / n
    rim = np.stack([radius * np.cos(a), radius * np.sin(a), np.zeros(n)], 1)
    verts = np.concatenate([[[0.0171, 0.0093, 0.0]], rim])
    return make(verts, [[0, 1 + i, 1 + (i + 1) % n] for i in range(n)])


def cloud(n, seed=5, radius=0.003, spread=0.04, lift=0.01):
    """n small spheres scattered over a box above the plane z = 0, for the NARROW camera.  Small against their distance on purpose:
    loosening a sphere to r (1 + 1e-5) moves its depth by 1e-5 r / sqrt(1 - (w / r)^2) at the distance w from its axis, so the
    yardstick calls the ring with sqrt(1 - (w / r)^2) < 10 r / depth undecided, a share (10 r / depth)^2 of the sphere's disc; at
    r / depth = 0.0015 that is 2e-4 of it, at 0.1 all of it."""
    g = np.random.default_rng(seed)
    centres = np.stack([g.uniform(-spread, spread, n), g.uniform(-spread, spread, n), g.uniform(lift, lift + 0.02, n)], 1)
    return make(centres=centres, radii=g.uniform(0.6 * radius, radius, n))


def pack(scenes):
    """A list of scenes -> the shared tables (faces made global) as a dict of arrays, offsets included."""
    base = np.cumsum([0] + [len(s["verts"]) for s in scenes])
    cat = lambda key, shape, dtype: (np.concatenate([s[key] for s in scenes]) if scenes else np.zeros(shape)).astype(dtype)  # noqa: E731
    return dict(verts=cat("verts", (0, 3), np.float32),
                faces=np.concatenate([s["faces"] + b for s, b in zip(scenes, base)]).astype(np.int32), face_rgb=cat("face_rgb", (0, 3), np.uint8),
                centres=cat("centres", (0, 3), np.float32), radii=cat("radii", (0,), np.float32), sphere_rgb=cat("sphere_rgb", (0, 3), np.uint8),
                face_offset=np.cumsum([0] + [len(s["faces"]) for s in scenes]).astype(np.int32),
                sphere_offset=np.cumsum([0] + [len(s["centres"]) for s in scenes]).astype(np.int32))


SIZE_EDGES = ((40, 24), (17, 16), (16, 33), (1, 1))            # partial tiles on either axis, and a single pixel
FACE_COUNTS, SPHERE_COUNTS, COUNT_SIZE = (1, 255, 256, 257, 513), (1, 256, 257), (96, 64)      # around the chunk of 256 (0: the empty scene)
BALL = dict(centres=[[0.004, -0.003, 0.01]], radii=[0.004])


def views():
    """name -> (scene, W, H, camera position, yfov): every view the GPU tests hold against the yardstick.  The host tests check
    that the fp64 reference alone leaves at most 0.1 % of each undecided."""
    out = {"ico3_512": (ico(3), 512, 512, CAM_POS, YFOV)}
    for W, H in SIZE_EDGES:
        out[f"size_{W}x{H}"] = (merge(ico(1, 0.03), cloud(12, radius=0.005)), W, H, NARROW_POS, NARROW_YFOV)
    for n in FACE_COUNTS:
        out[f"faces_{n}"] = (fan(n), *COUNT_SIZE, NARROW_POS, NARROW_YFOV)
    for n in SPHERE_COUNTS:
        out[f"spheres_{n}"] = (cloud(n), *COUNT_SIZE, NARROW_POS, NARROW_YFOV)
    out["mixed_257"] = (merge(fan(257), cloud(257)), *COUNT_SIZE, NARROW_POS, NARROW_YFOV)
    out["sphere_before_triangle"] = (merge(fan(1), make(**BALL)), *COUNT_SIZE, NARROW_POS, NARROW_YFOV)
    lid = make([[-0.02, -0.02, 0.03], [0.03, -0.01, 0.03], [0.0, 0.03, 0.03]], [[0, 1, 2]])
    out["triangle_before_sphere"] = (merge(lid, make(**BALL)), *COUNT_SIZE, NARROW_POS, NARROW_YFOV)
    return out


_REFERENCES = {}


def view_reference(name):
    """``reference`` of a named view: computed once, shared, never changed."""
    if name not in _REFERENCES:
        scene, W, H, pos, yfov = views()[name]
        _REFERENCES[name] = reference(scene, W, H, pos=pos, yfov=yfov)
    return _REFERENCES[name]


def camera32(pos=CAM_POS, rot=CAM_ROT):
    """A camera as the library gets it, and as the emulation must see it: float32 values."""
    return np.asarray(pos, np.float32), np.asarray(rot, np.float32)


def reference(scene, W, H, pos=CAM_POS, rot=CAM_ROT, lights=LIGHTS, ambient=AMBIENT, background=BACKGROUND, znear=ZNEAR, zfar=ZFAR,
              yfov=YFOV):
    """The yardstick of one view of one scene: the fp64 result at the exact margin (``rgb, depth, prim``), the undecided pixels and
    the float32 emulation's largest relative depth deviation on decided pixels that both hit."""
    pos, rot = camera32(pos, rot)
    lights = np.asarray(lights, np.float32).reshape(-1, 4)
    args = (scene["verts"], scene["faces"], scene["face_rgb"], scene["centres"], scene["radii"], scene["sphere_rgb"], pos, rot, yfov,
            np.float32(znear), np.float32(zfar), W, H, lights, np.float32(ambient), background)
    wide = sr.render_image(*args, dtype=np.float64, margins=sr.MARGINS)
    single = sr.render_image(*args, dtype=np.float32)
    und = sr.undecided(wide)
    exact, d32 = wide["depth"][1], single["depth"][0].astype(np.float64)
    both = (exact > 0) & (d32 > 0) & ~und
    yard = float((np.abs(d32 - exact)[both] / exact[both]).max()) if both.any() else 0.0
    return dict(rgb=wide["rgb"][1], depth=exact, prim=wide["prim"][1], undecided=und, yard=yard)


def check(got, want, what, prim_map=None):
    """One image of the kernel (``rgb, depth, prim`` arrays) against ``reference``'s; prints the worst values, then asserts."""
    und, exact = want["undecided"], want["depth"]
    ok = ~und
    prim = got["prim"] if prim_map is None else prim_map(got["prim"])
    mismatch = int(((got["depth"] > 0) != (exact > 0))[ok].sum())
    wrong_prim = int((prim != want["prim"])[ok].sum())
    both = ok & (got["depth"] > 0) & (exact > 0)
    worst = float((np.abs(got["depth"].astype(np.float64) - exact)[both] / exact[both]).max()) if both.any() else 0.0
    levels = int(np.abs(got["rgb"].astype(np.int32) - want["rgb"].astype(np.int32))[ok].max()) if ok.any() else 0
    print(f"{what}: {exact.shape[1]} x {exact.shape[0]}, hits {int((exact > 0).sum())}, undecided {int(und.sum())}, hit mismatches "
          f"{mismatch}, prim mismatches {wrong_prim}, depth yardstick {want['yard']:.3e}, kernel {worst:.3e}, colour levels off {levels}")
    assert und.mean() <= 1e-3, (what, int(und.sum()))
    assert mismatch == 0 and wrong_prim == 0, (what, mismatch, wrong_prim)
    assert worst <= 8 * want["yard"], (what, worst, want["yard"])
    assert levels <= 1, (what, levels)
