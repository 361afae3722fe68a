"""The project's own NumPy emulation of ``a3vt_scene_render`` (``include/a3vt.h``, csrc/scene_render.hip): test infrastructure, in
the manner of ``touch_render_ref.py``.  A caster and a shader with the kernel's contract, by another route: everything happens in the
WORLD frame (the kernel moves the primitives to the camera frame first), triangles by Möller–Trumbore (the kernel tests rounded edge
functions and takes the depth from the plane), spheres by the contract's cancellation-free form.

``dtype=`` is the precision of the arithmetic: ``np.float64`` is the yardstick, ``np.float32`` what the kernel's own precision gives
by this route.  ``margins`` loosens (> 0) or tightens (< 0) BOTH primitive kinds at once: the three barycentric tests of a face by
the margin, a sphere's radius to ``r (1 + margin)``.  One result per margin comes back, stacked on a leading axis:

    rgb (n, H, W, 3) uint8, depth (n, H, W) dtype (0 without a hit), prim (n, H, W) int32 (-1 without one),
    second (n, H, W) dtype: the runner-up's depth (inf without one), second_prim (n, H, W) int32, normal (n, H, W, 3)

``undecided(result)`` is the yardstick's rule for the pixels a comparison leaves out; see its docstring.

Only the pixels inside a primitive's projected bounding window are tested against it (a window, not a verdict: generous, and the whole
image for a primitive that reaches the camera's plane), so a 512 x 512 image of a thousand faces takes a second."""
import numpy as np

MARGINS = (1e-5, 0.0, -1e-5)


def camera_rotation(euler_xyz_deg=(45.0, 0.0, 180.0)):
    """Extrinsic x, y, z rotations in degrees (SciPy's ``from_euler("xyz", ., degrees=True)``): R_z . R_y . R_x."""
    a = np.radians(np.asarray(euler_xyz_deg, np.float64))
    (cx, cy, cz), (sx, sy, sz) = np.cos(a), np.sin(a)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rz @ ry @ rx


def rays(rot, yfov, W, H, dtype=np.float64):
    """World-frame ray directions (H, W, 3) through the pixel centres, row 0 at the top; the ray parameter is the depth."""
    T = dtype
    yfov = float(np.float32(yfov))                       # (the C ABI takes a float)
    tan_y, tan_x = T(np.tan(0.5 * yfov)), T(np.tan(0.5 * yfov) * W / H)
    x = ((np.arange(W, dtype=T) + T(0.5)) / T(W) * T(2) - T(1)) * tan_x
    y = (T(1) - (np.arange(H, dtype=T) + T(0.5)) / T(H) * T(2)) * tan_y
    eye = np.stack([np.broadcast_to(x[None, :], (H, W)), np.broadcast_to(y[:, None], (H, W)), -np.ones((H, W), T)], -1)
    return (eye.reshape(-1, 3) @ np.asarray(rot, T).T).reshape(H, W, 3)


def _window(centre, radius, pos, rot, yfov, W, H):
    """Rows and columns (r0, r1, c0, c1) that can see a bounding sphere, None when none can (fp64; generous)."""
    q = np.asarray(rot, np.float64).T @ (np.asarray(centre, np.float64) - np.asarray(pos, np.float64))
    w, rad = -q[2], float(radius) * 1.01 + 1e-9
    if not (np.isfinite(q).all() and np.isfinite(rad)):
        return 0, H, 0, W
    if w + rad <= 0:
        return None
    if w - rad <= 1e-6:
        return 0, H, 0, W
    tan_y = np.tan(0.5 * yfov)
    tan_x = tan_y * W / H
    xs = [(q[0] + sx * rad) / (w + sw * rad) for sx in (-1, 1) for sw in (-1, 1)]
    ys = [(q[1] + sy * rad) / (w + sw * rad) for sy in (-1, 1) for sw in (-1, 1)]
    c0, c1 = int(np.floor((min(xs) / tan_x + 1) / 2 * W)) - 2, int(np.ceil((max(xs) / tan_x + 1) / 2 * W)) + 2
    r0, r1 = int(np.floor((1 - max(ys) / tan_y) / 2 * H)) - 2, int(np.ceil((1 - min(ys) / tan_y) / 2 * H)) + 2
    r0, r1, c0, c1 = max(r0, 0), min(r1, H), max(c0, 0), min(c1, W)
    return (r0, r1, c0, c1) if r0 < r1 and c0 < c1 else None


def _dot(a, b):
    return (a * b).sum(-1)


def _offer(state, i, win, t, hit, ident):
    """Primitive ``ident`` offers depth ``t`` where ``hit`` in the window ``win`` of margin ``i``: the nearest hit wins, the lower
    index among equal depths; what it beats, or what beats it, is the runner-up."""
    r0, r1, c0, c1 = win
    best, prim = state["depth"][i, r0:r1, c0:c1], state["prim"][i, r0:r1, c0:c1]
    second, second_prim = state["second"][i, r0:r1, c0:c1], state["second_prim"][i, r0:r1, c0:c1]
    wins = hit & ((t < best) | ((t == best) & (ident < prim)))
    places = hit & ~wins & ((t < second) | ((t == second) & (ident < second_prim)))
    second[wins], second_prim[wins] = best[wins], prim[wins]
    best[wins], prim[wins] = t[wins], ident
    second[places], second_prim[places] = t[places], ident


def render_image(verts, faces, face_rgb, centres, radii, sphere_rgb, pos, rot, yfov, znear, zfar, W, H, lights, ambient, background,
                 dtype=np.float64, margins=(0.0,)):
    """One image of one scene (its own tables: ``prim`` counts faces from 0 and spheres from ``len(faces)``); see the module."""
    T = dtype
    verts, faces = np.asarray(verts, T).reshape(-1, 3), np.asarray(faces).reshape(-1, 3)
    face_rgb = np.asarray(face_rgb).reshape(-1, 3)
    centres, radii, sphere_rgb = np.asarray(centres, T).reshape(-1, 3), np.asarray(radii, T).reshape(-1), np.asarray(sphere_rgb).reshape(-1, 3)
    lights = np.asarray(lights, T).reshape(-1, 4)
    o, F, n = np.asarray(pos, T).reshape(3), len(faces), len(margins)
    D = rays(rot, yfov, W, H, T)
    length = np.sqrt(_dot(D, D))
    state = {"depth": np.full((n, H, W), np.inf, T), "prim": np.full((n, H, W), -1, np.int32),
             "second": np.full((n, H, W), np.inf, T), "second_prim": np.full((n, H, W), -1, np.int32)}
    one, near, far = T(1), T(znear), T(zfar)
    normals = np.zeros((F, 3), T)
    with np.errstate(all="ignore"):
        for f in range(F):
            idx = faces[f]
            if (idx < 0).any() or (idx >= len(verts)).any() or not np.isfinite(verts[idx]).all():
                continue
            v0, v1, v2 = verts[idx]
            e1, e2 = v1 - v0, v2 - v0
            normals[f] = np.cross(e1, e2)
            g = verts[idx].astype(np.float64).mean(0)
            win = _window(g, np.linalg.norm(verts[idx].astype(np.float64) - g, axis=1).max(), pos, rot, yfov, W, H)
            if win is None:
                continue
            d = D[win[0]:win[1], win[2]:win[3]]
            pvec = np.cross(d, e2)
            inv = one / _dot(pvec, e1)
            tvec = o - v0
            u = _dot(pvec, tvec) * inv
            qvec = np.cross(tvec, e1)
            v = _dot(d, qvec) * inv
            t = _dot(qvec, e2) * inv
            ranged = (t >= near) & (t <= far)                       # (a NaN fails)
            for i, margin in enumerate(margins):
                m = T(margin)
                _offer(state, i, win, t, ranged & (u >= -m) & (v >= -m) & (u + v <= one + m), f)
        for s in range(len(centres)):
            c, r = centres[s], radii[s]
            if not (np.isfinite(c).all() and np.isfinite(r) and r > 0):
                continue
            win = _window(c, float(r) * (1 + max(margins)), pos, rot, yfov, W, H)
            if win is None:
                continue
            d, ln = D[win[0]:win[1], win[2]:win[3]], length[win[0]:win[1], win[2]:win[3]]
            unit = d / ln[..., None]
            oc = c - o
            b = _dot(unit, oc)
            w = oc - b[..., None] * unit
            w2 = _dot(w, w)
            for i, margin in enumerate(margins):
                rm = r * (one + T(margin))
                disc = rm * rm - w2
                t = (b - np.sqrt(disc)) / ln
                _offer(state, i, win, t, (disc >= 0) & (t >= near) & (t <= far), F + s)
        # shading
        prim, depth = state["prim"], state["depth"]
        hit = prim >= 0
        p = o + np.where(hit, depth, T(0))[..., None] * D[None]
        is_face = hit & (prim < F)
        is_sphere = hit & (prim >= F)
        nrm = np.zeros((n, H, W, 3), T)
        base = np.zeros((n, H, W, 3), T)
        if is_face.any():
            fn = normals[prim[is_face]]
            fn = fn / np.abs(fn).max(-1, keepdims=True)
            fn = fn / np.sqrt(_dot(fn, fn))[..., None]
            flip = _dot(fn, o - p[is_face]) < 0
            fn[flip] = -fn[flip]
            nrm[is_face], base[is_face] = fn, face_rgb[prim[is_face]].astype(T)
        if is_sphere.any():
            s = prim[is_sphere] - F
            nrm[is_sphere] = (p[is_sphere] - centres[s]) / radii[s][..., None]
            base[is_sphere] = sphere_rgb[s].astype(T)
        total = np.zeros((n, H, W), T)
        for k in range(len(lights)):
            l = lights[k, :3] - p
            l2 = _dot(l, l)
            ll = np.sqrt(l2)
            total = total + lights[k, 3] * np.maximum(T(0), _dot(nrm, l) / ll) / l2
        shade = T(ambient) + total * T(1.0 / np.pi)
        colour = np.floor(np.clip(base * shade[..., None], T(0), T(255)) + T(0.5))
        rgb = np.where(hit[..., None], colour, np.asarray(background, T).reshape(3)).astype(np.uint8)
        unit = normals.astype(np.float64)
        unit = unit / np.linalg.norm(unit, axis=1, keepdims=True)
    state["depth"] = np.where(hit, depth, T(0))
    state["rgb"], state["normal"] = rgb, nrm
    state["local_prim"], state["local_second_prim"] = state["prim"], state["second_prim"]       # (indices into this scene's tables)
    state["face_normals"], state["face_rgb"] = unit, face_rgb
    return state


def undecided(result, rel=1e-6):
    """Pixels the comparison leaves out, from a result rendered with ``margins=MARGINS`` (loose, exact, tight): those whose prim or
    depth (relative ``rel``; a hit coming or going counts) moves between the margins, and those whose exact winner and runner-up lie
    within ``rel`` of each other with a different colour or normal, that is, unless both are faces of one colour in one plane
    (``add_faces``' coincident copies: either may win and the pixel looks the same)."""
    depth, prim = result["depth"], result["prim"]
    exact, out = depth[1], np.zeros(depth.shape[1:], bool)
    for other in (0, 2):
        out |= prim[other] != prim[1]
        out |= np.abs(depth[other] - exact) > rel * np.abs(exact)
    second = result["second"][1]
    a, b = result["local_prim"][1], result["local_second_prim"][1]
    close = (a >= 0) & (b >= 0) & (np.abs(second - exact) <= rel * np.abs(exact))
    if close.any():
        n, colour = result["face_normals"], result["face_rgb"]
        F = len(n)
        same = (a[close] < F) & (b[close] < F)
        if F:
            fa, fb = np.minimum(a[close], F - 1), np.minimum(b[close], F - 1)
            same &= (colour[fa] == colour[fb]).all(-1) & (np.abs((n[fa] * n[fb]).sum(-1)) >= 1 - 1e-9)
        out[close] |= ~same
    return out


def render(verts, faces, face_rgb, centres, radii, sphere_rgb, face_offset, sphere_offset, image_scene, cam_pos, cam_rot, yfov, znear,
           zfar, W, H, lights, ambient, background, dtype=np.float64, margins=(0.0,)):
    """``ops.scene_render``'s tables on the host -> a list of I ``render_image`` results whose ``prim`` / ``second_prim`` are
    indices into the SHARED tables, as the kernel's."""
    verts, faces = np.asarray(verts).reshape(-1, 3), np.asarray(faces).reshape(-1, 3)
    F, out = len(faces), []
    for i, m in enumerate(np.asarray(image_scene).reshape(-1)):
        f0, f1, s0, s1 = face_offset[m], face_offset[m + 1], sphere_offset[m], sphere_offset[m + 1]
        res = render_image(verts, faces[f0:f1], np.asarray(face_rgb).reshape(-1, 3)[f0:f1], np.asarray(centres).reshape(-1, 3)[s0:s1],
                           np.asarray(radii).reshape(-1)[s0:s1], np.asarray(sphere_rgb).reshape(-1, 3)[s0:s1], cam_pos[i], cam_rot[i],
                           yfov, znear, zfar, W, H, lights, ambient, background, dtype, margins)
        for key in ("prim", "second_prim"):
            local = res[key]
            res[key] = np.where(local < 0, -1, np.where(local < f1 - f0, local + f0, local - (f1 - f0) + s0 + F)).astype(np.int32)
        out.append(res)
    return out
