"""oracle.pooling — explicit float64 reference of the per-vertex image-feature pooling (TEST INFRASTRUCTURE ONLY).

``csrc/pooling.hip`` (``a3vt_image_pool_fwd / _fwd_add / _bwd``) written out from the formulas in plain numpy, with no
``grid_sample``: projection with a 3 x 4 matrix, the reference's in-place patches (``p2 == 0 -> 0.1``, ``isinf(xs) -> 0.5``,
``isinf(ys) -> 0.5``), bilinear gather with zero padding and ``align_corners=True`` from every map, the concatenation, and the
gradients of all of it.

What is float32 and what is float64: the projection ``p_r = ((x m_r0 + y m_r1) + z m_r2) + m_r3`` and the three patch
decisions are evaluated in float32, because they are decisions on float32 values (``3e38 / 0.5`` is infinite in float32 only);
the patched depth is ``float32(0.1)``.  Everything after that is float64 on the float32 ``p`` values.

Besides every value the reference returns the sum of the magnitudes of exactly the terms that make it up (``abs_*``), for
error bounds of the form ``k * 2^-24 * abs_sum``.
"""
import numpy as np


def project(verts, matrix, f32_quotients=False):
    """float32 projection and patch decisions -> dict of (B, N) arrays: ``p0 p1 p2`` (float64 values of the float32
    results, ``p2`` after the depth patch), ``xs ys`` (float64, after the overflow patches), and the boolean
    ``z_patched xs_patched ys_patched``.  ``f32_quotients``: ``xs`` and ``ys`` are the float32 quotients the patch decisions
    were taken on instead of the float64 quotients of the same ``p`` (they differ where a division is inexact in float32)."""
    v = np.asarray(verts, dtype=np.float32)
    m = np.asarray(matrix, dtype=np.float32).reshape(3, 4)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        p = [((x * m[r, 0] + y * m[r, 1]) + z * m[r, 2]) + m[r, 3] for r in range(3)]
        z_patched = p[2] == np.float32(0.0)
        p2 = np.where(z_patched, np.float32(0.1), p[2]).astype(np.float32)
        xs32, ys32 = p[1] / p2 / np.float32(256.0), p[0] / p2 / np.float32(256.0)
        xs_patched, ys_patched = np.isinf(xs32), np.isinf(ys32)
        p0, p1, p2 = p[0].astype(np.float64), p[1].astype(np.float64), p2.astype(np.float64)
        xs = np.where(xs_patched, 0.5, xs32.astype(np.float64) if f32_quotients else p1 / p2 / 256.0)
        ys = np.where(ys_patched, 0.5, ys32.astype(np.float64) if f32_quotients else p0 / p2 / 256.0)
    return {"p0": p0, "p1": p1, "p2": p2, "xs": xs, "ys": ys,
            "z_patched": z_patched, "xs_patched": xs_patched, "ys_patched": ys_patched}


def _corners(ix, iy, H, W):
    """The four corners of every vertex: list of (in_range (B,N) bool, y index, x index, weight, d weight / d ix,
    d weight / d iy) in the order nw, ne, sw, se.  ``floor`` and the range tests stay in floating point; an
    out-of-range corner gets index 0 (and is masked), so no out-of-range value is ever cast to an integer."""
    fx, fy = np.floor(ix), np.floor(iy)
    x1, y1 = fx + 1.0, fy + 1.0
    wx0, wx1, wy0, wy1 = x1 - ix, ix - fx, y1 - iy, iy - fy
    out = []
    for cy, cx, w, dwx, dwy in ((fy, fx, wx0 * wy0, -wy0, -wx0), (fy, x1, wx1 * wy0, wy0, -wx1),
                                (y1, fx, wx0 * wy1, -wy1, wx0), (y1, x1, wx1 * wy1, wy1, wx1)):
        inside = (cx >= 0.0) & (cx <= W - 1.0) & (cy >= 0.0) & (cy <= H - 1.0)
        yi = np.where(inside, cy, 0.0).astype(np.int64)
        xi = np.where(inside, cx, 0.0).astype(np.int64)
        out.append((inside, yi, xi, w, dwx, dwy))
    return out


def pool_reference(maps, verts, matrix, grad_out=None, base=None, f32_quotients=False):
    """maps: list of (B, C_k, H_k, W_k); verts (B, N, 3); matrix 3 x 4; grad_out / base (B, N, sum C_k) or None.

    Returns a dict: ``feats`` (B, N, sum C_k) and ``abs_feats`` (sum |w m| + |base|); with ``grad_out`` also ``grad_maps``
    and ``abs_grad_maps`` (lists of (B, C_k, H_k, W_k)), ``grad_verts`` and ``abs_grad_verts`` (B, N, 3).  All float64.
    ``f32_quotients``: see ``project`` (the coordinates an fp32 kernel samples at; the gradient formulas are the same)."""
    maps = [np.asarray(m, dtype=np.float64) for m in maps]
    M = np.asarray(matrix, dtype=np.float32).reshape(3, 4).astype(np.float64)
    pr = project(verts, matrix, f32_quotients)
    B, N = pr["xs"].shape
    bidx = np.broadcast_to(np.arange(B)[:, None], (B, N))
    feats, abs_feats, gmaps, abs_gmaps = [], [], [], []
    ggx, ggy = np.zeros((B, N)), np.zeros((B, N))       # d / d ys and d / d xs before the factor 2 ...
    ax, ay = np.zeros((B, N)), np.zeros((B, N))         # ... and the sums of the magnitudes of their terms
    off = 0
    g_all = None if grad_out is None else np.asarray(grad_out, dtype=np.float64)
    for m in maps:
        _, C, H, W = m.shape
        cl = np.ascontiguousarray(m.transpose(0, 2, 3, 1))                 # (B, H, W, C)
        ix, iy = pr["ys"] * (W - 1), pr["xs"] * (H - 1)
        g = None if g_all is None else g_all[..., off:off + C]
        f, fa = np.zeros((B, N, C)), np.zeros((B, N, C))
        if g is not None:
            gm, gma = np.zeros_like(cl), np.zeros_like(cl)
            gix, giy, aix, aiy = np.zeros((B, N)), np.zeros((B, N)), np.zeros((B, N)), np.zeros((B, N))
        for inside, yi, xi, w, dwx, dwy in _corners(ix, iy, H, W):
            sel = np.nonzero(inside)
            if sel[0].size == 0:
                continue
            val = cl[bidx[sel], yi[sel], xi[sel]]                          # (n_in, C)
            term = w[sel][:, None] * val
            f[sel] += term
            fa[sel] += np.abs(term)
            if g is not None:
                gt = w[sel][:, None] * g[sel]
                np.add.at(gm, (bidx[sel], yi[sel], xi[sel]), gt)
                np.add.at(gma, (bidx[sel], yi[sel], xi[sel]), np.abs(gt))
                gv = g[sel] * val                                          # d w / d ix is the same for every channel
                sgv, agv = gv.sum(-1), np.abs(gv).sum(-1)
                gix[sel] += sgv * dwx[sel]
                giy[sel] += sgv * dwy[sel]
                aix[sel] += agv * np.abs(dwx[sel])
                aiy[sel] += agv * np.abs(dwy[sel])
        feats.append(f)
        abs_feats.append(fa)
        if g is not None:
            gmaps.append(gm.transpose(0, 3, 1, 2))
            abs_gmaps.append(gma.transpose(0, 3, 1, 2))
            ggx += gix * ((W - 1) / 2.0)
            ggy += giy * ((H - 1) / 2.0)
            ax += aix * ((W - 1) / 2.0)
            ay += aiy * ((H - 1) / 2.0)
        off += C
    feats, abs_feats = np.concatenate(feats, -1), np.concatenate(abs_feats, -1)
    if base is not None:
        base = np.asarray(base, dtype=np.float64)
        feats, abs_feats = base + feats, np.abs(base) + abs_feats
    res = {"feats": feats, "abs_feats": abs_feats}
    if grad_out is None:
        return res
    # grid = 2 (ys, xs) - 1; the in-place patches cut the gradient where they fired
    gys, ays = np.where(pr["ys_patched"], 0.0, 2.0 * ggx), np.where(pr["ys_patched"], 0.0, 2.0 * ax)
    gxs, axs = np.where(pr["xs_patched"], 0.0, 2.0 * ggy), np.where(pr["xs_patched"], 0.0, 2.0 * ay)
    p0, p1, p2 = pr["p0"], pr["p1"], pr["p2"]
    inv = 1.0 / (256.0 * p2)
    gp = [gys * inv, gxs * inv, np.where(pr["z_patched"], 0.0, -(gys * p0 + gxs * p1) * inv / p2)]
    ap = [ays * np.abs(inv), axs * np.abs(inv),
          np.where(pr["z_patched"], 0.0, (ays * np.abs(p0) + axs * np.abs(p1)) * np.abs(inv) / np.abs(p2))]
    res["grad_maps"], res["abs_grad_maps"] = gmaps, abs_gmaps
    res["grad_verts"] = np.stack([sum(gp[r] * M[r, d] for r in range(3)) for d in range(3)], -1)
    res["abs_grad_verts"] = np.stack([sum(ap[r] * abs(M[r, d]) for r in range(3)) for d in range(3)], -1)
    return res
