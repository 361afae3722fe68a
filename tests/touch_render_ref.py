"""The project's own NumPy emulation of ``a3vt_touch_render`` (``include/a3vt.h``, csrc/touch_render.hip): test infrastructure, in
the manner of ``adam_ref.py``.  Two stages, as the library's two launches:

* ``cast`` — the depth map by ray casting: Möller–Trumbore against every face in the WORLD frame (the kernel moves the faces to the
  camera frame first and tests edges by another formula: the emulation is a different route to the same number), nearest hit with
  ``znear <= t <= zfar``, two-sided, 0 without a hit.  ``margin`` loosens (> 0) or tightens (< 0) the three barycentric tests:
  ``undecided`` marks the pixels whose depth moves when it does.
* ``finish`` — status, gel image and contact points from float32 depth maps, following ``simulator/scene/instance.py:142``,
  ``:207-258`` and ``:154-204`` step by step.

``dtype=`` is the precision of the arithmetic.  ``np.float64`` is the yardstick.  For ``finish`` it means what NumPy itself computes
in the reference from a float32 map: the comparisons with ``max_depth``, the gel scaling, the stored 7 x 7 means, the gradient and the
normal are float32 there (a float32 array keeps its dtype against Python scalars), the mean's accumulation, the light directions,
the shading and the points are float64.  ``np.float32`` evaluates every step in float32, as the kernel does.

``render(...)`` has the call shape of ``ops.touch_render`` on NumPy arrays or CPU tensors and serves ``RenderedSampler(render=)``."""
import numpy as np

RES = 121
PIX = RES * RES
MAX_DEPTH, YFOV, ZNEAR, ZFAR = 0.025, 40.0 / 180.0 * np.pi, 1e-4, 10.0
R_Y_MINUS_90 = np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])
LIGHTS = np.array([[-0.5, 0.5, 1.0], [1.3, -0.4, 1.0], [1.3, 1.4, 1.0]])


def euler_xyz(angles):
    """Extrinsic x, y, z rotations (SciPy's ``from_euler("xyz", angles)``): R_z . R_y . R_x."""
    (cx, cy, cz), (sx, sy, sz) = np.cos(angles), np.sin(angles)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rz @ ry @ rx


def camera_rotation(rot, dtype=np.float64):
    """``cam_rot . R_y(-90 deg)`` (instance.py:127-133): columns (rot[:, 2], rot[:, 1], -rot[:, 0])."""
    return np.asarray(rot, dtype) @ R_Y_MINUS_90.astype(dtype)


def rays(rot, yfov=YFOV, dtype=np.float64):
    """World-frame ray directions (121, 121, 3) through the pixel centres, row 0 at the top; the ray parameter is the depth."""
    t = dtype(np.tan(0.5 * yfov))
    centre = (np.arange(RES, dtype=dtype) + dtype(0.5)) / dtype(RES) * dtype(2)
    x, y = (centre - dtype(1)) * t, (dtype(1) - centre) * t
    eye = np.stack([np.broadcast_to(x[None, :], (RES, RES)), np.broadcast_to(y[:, None], (RES, RES)), -np.ones((RES, RES), dtype)], -1)
    return (eye.reshape(-1, 3) @ camera_rotation(rot, dtype).T).reshape(RES, RES, 3)


def cast(verts, faces, pos, rot, yfov=YFOV, znear=ZNEAR, zfar=ZFAR, dtype=np.float64, margins=(0.0,), chunk=64):
    """Depth maps (len(margins), 121, 121) of one view, one per barycentric margin, in ``dtype``."""
    verts, faces = np.asarray(verts, dtype), np.asarray(faces).reshape(-1, 3)
    origin, d = np.asarray(pos, dtype).reshape(3), rays(rot, yfov, dtype).reshape(-1, 1, 3)
    best = np.full((len(margins), PIX), np.inf, dtype)
    one = dtype(1)
    for f0 in range(0, len(faces), chunk):
        tri = verts[faces[f0:f0 + chunk]]                       # (n, 3, 3)
        v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        pvec = np.cross(d, e2[None])                            # (P, n, 3)
        det = (e1[None] * pvec).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = one / det
            tvec = (origin - v0)[None]
            u = (tvec * pvec).sum(-1) * inv
            qvec = np.cross(tvec, e1[None])
            v = (d * qvec).sum(-1) * inv
            t = (e2[None] * qvec).sum(-1) * inv
            ranged = (t >= dtype(znear)) & (t <= dtype(zfar))   # (a NaN fails)
            for i, margin in enumerate(margins):
                m = dtype(margin)
                hit = ranged & (u >= -m) & (v >= -m) & (u + v <= one + m)
                best[i] = np.minimum(best[i], np.where(hit, t, np.inf).min(axis=1))
    return np.where(np.isinf(best), dtype(0), best).reshape(len(margins), RES, RES)


def undecided(loose, exact, tight, rel=1e-6):
    """Pixels whose depth moves by more than ``rel`` (relative; a hit that comes or goes counts) between the three margins."""
    out = np.zeros(exact.shape, bool)
    for other in (loose, tight):
        out |= (other == 0) != (exact == 0)
        out |= np.abs(other - exact) > rel * np.abs(exact)
    return out


def _smooth(gel, wide):
    """The 7 x 7 mean with SciPy's ``reflect`` boundary (d c b a | a b c d), accumulated in ``wide`` over the window in row-major
    order, each term weighted by 1 / 49 as a convolution does; returned in the map's own dtype."""
    pad = np.pad(gel, 3, mode="symmetric").astype(wide)
    weight, acc = wide(1.0) / wide(49.0), np.zeros(gel.shape, wide)
    for dr in range(7):
        for dc in range(7):
            acc = acc + pad[dr:dr + RES, dc:dc + RES] * weight
    return acc.astype(gel.dtype)


def finish_one(depth, pos, rot, max_depth=MAX_DEPTH, yfov=YFOV, dtype=np.float64):
    """One float32 depth map -> (status 0/1, touch (121, 121, 3), points (n, 3)); see the module docstring for ``dtype``."""
    wide = dtype
    d = np.array(depth, np.float32)
    md = np.float32(max_depth)
    status = int((d <= md).sum()) - int((d == 0).sum()) > 0
    d[d > md] = 1.0
    d[d == 0] = 1.0

    zeros = d >= md
    gel = -(d - md)
    gel[zeros] = 0
    gel = gel * np.float32(6) / md
    gel = gel / np.float32(30.0) + np.float32(0.4)
    gel[zeros] = _smooth(gel, wide)[zeros]
    zy, zx = np.gradient(gel)
    normal = np.stack([-zx, -zy, np.ones_like(gel)], -1)
    normal = normal / np.sqrt((normal * normal).sum(-1, dtype=np.float32))[..., None]
    grid = np.arange(RES).astype(wide) / wide(RES)
    position = np.stack([np.broadcast_to(grid[:, None], (RES, RES)), np.broadcast_to(grid[None, :], (RES, RES)), gel.astype(wide)], -1)
    touch = np.zeros((RES, RES, 3), wide)
    for i in range(3):
        light = LIGHTS[i].astype(wide) - position
        light = light / np.sqrt((light * light).sum(-1))[..., None]
        touch[..., i] = np.clip(wide(2.0) * (normal.astype(wide) * light).sum(-1), 0, 1)
    touch = np.clip(touch * wide(255.0), 0, 255)

    t = wide(np.tan(0.5 * yfov))
    offset = np.arange(RES) - RES // 2
    xs, ys = np.broadcast_to(offset[None, :], (RES, RES)), np.broadcast_to(offset[:, None], (RES, RES))
    dw = d.astype(wide)
    cloud = np.stack([dw * (np.abs(xs).astype(wide) / wide(60.0) * t) * np.sign(xs).astype(wide),
                      dw * (np.abs(ys).astype(wide) / wide(60.0) * t) * -np.sign(ys).astype(wide), -dw], -1)
    cloud = cloud[d < 1.0].reshape(-1, 3)
    points = cloud @ camera_rotation(rot, wide).T + np.asarray(pos, wide).reshape(3)
    return status, touch, points


def finish(depth, cam_pos, cam_rot, max_depth=MAX_DEPTH, yfov=YFOV, dtype=np.float64):
    """(I, 121, 121) maps -> (status (I,) int32, touch (I, 121, 121, 3), points: I arrays (n, 3))."""
    out = [finish_one(depth[i], cam_pos[i], cam_rot[i], max_depth, yfov, dtype) for i in range(len(depth))]
    return np.array([s for s, _, _ in out], np.int32), np.stack([t for _, t, _ in out]), [p for _, _, p in out]


def render(verts, faces, face_offset, image_mesh, cam_pos, cam_rot, max_depth=MAX_DEPTH, yfov=YFOV, znear=ZNEAR, zfar=ZFAR,
           want_touch=True, want_points=True, dtype=np.float64):
    """``ops.touch_render`` on the host: the same arguments (arrays or CPU tensors) and the same dict of float32 / int32 CPU tensors;
    the contract's clamps included."""
    import torch
    verts, faces = np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(faces).reshape(-1, 3)
    face_offset, image_mesh = np.asarray(face_offset).reshape(-1), np.asarray(image_mesh).reshape(-1)
    cam_pos, cam_rot = np.asarray(cam_pos, np.float64).reshape(-1, 3), np.asarray(cam_rot, np.float64).reshape(-1, 3, 3)
    I, M, F = len(image_mesh), len(face_offset) - 1, len(faces)
    depth = np.zeros((I, RES, RES), np.float32)
    for i in range(I):
        m = min(max(int(image_mesh[i]), 0), M - 1)
        f0 = min(max(int(face_offset[m]), 0), F)
        f1 = min(max(int(face_offset[m + 1]), f0), F)
        mine = faces[f0:f1]
        mine = mine[((mine >= 0) & (mine < len(verts))).all(axis=1)]
        depth[i] = cast(verts, mine, cam_pos[i], cam_rot[i], yfov, znear, zfar, dtype)[0]
    status, touch, points = finish(depth, cam_pos, cam_rot, max_depth, yfov, dtype)
    out = {"depth": torch.from_numpy(depth), "status": torch.from_numpy(status)}
    if want_touch:
        out["touch"] = torch.from_numpy(touch.astype(np.float32))
    if want_points:
        table = np.zeros((I, PIX, 3), np.float32)
        for i, p in enumerate(points):
            table[i, :len(p)] = p
        out["points"], out["count"] = torch.from_numpy(table), torch.tensor([len(p) for p in points], dtype=torch.int32)
    return out
