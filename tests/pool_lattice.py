"""Inputs of the image-pooling tests on which the kernel's fp32 geometry is exact (test_oracle_pooling, test_gpu_image_pool).

Matrix: the identity, so ``p = (x, y, z)``.  Vertices: ``x`` and ``y`` multiples of 2^-2 in [-64, 320], ``z`` in {0.5, 1, 2}.
Then ``ys = x / z / 256`` is a multiple of 2^-11 below 2^3 (14 bits), and ``gx = 2 ys - 1``, ``(gx + 1) / 2``, the product
with ``W - 1`` (W <= 46: 6 more bits), the floor, the four weight factors (at most 11 fractional bits each, values <= 1) and
their products (22 fractional bits) are all exact in fp32, with or without FMA contraction.  ``assert_geometry_exact``
checks exactly that, vertex by vertex and map size by map size, before a test goes to the GPU.
"""
import numpy as np

IDENTITY = [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]

# the vertices on which an in-place patch of the reference fires: depth; ys overflows; xs overflows; both
PATCH_VERTS = [(10.0, 20.0, 0.0), (3e38, 40.0, 0.5), (40.0, 3e38, 0.5), (3e38, -3e38, 0.5)]
HUGE_VERT = (1e30, 1e30, 1.0)     # finite, every corner of every map out of range: zero features, zero gradients


def special_verts(sizes):
    """Vertices that hit pixels exactly, for the map sizes ``[(H, W), ...]``: the four image corners, the centre,
    ``x = 256`` (ix = W - 1), the huge one, and per size the positions ``ix, iy`` in {-1, -0.5, size - 0.5} and the interior
    integer pixel (1, 1), wherever ``256 t / (size - 1)`` is a multiple of 2^-2 (so that it stays on the lattice: e.g.
    ix = -1 exists for W - 1 in 2, 4, 8, 16 ... and not for 22)."""
    out = [(0.0, 0.0, 1.0), (256.0, 0.0, 1.0), (0.0, 256.0, 1.0), (256.0, 256.0, 1.0), (128.0, 128.0, 1.0),
           (256.0, 128.0, 1.0), (128.0, 256.0, 1.0), HUGE_VERT]

    def at(t, size):       # the coordinate that puts the pixel coordinate at t on an axis of that size, or None
        if size < 2:
            return None
        c = 256.0 * t / (size - 1)
        return c if (c * 4.0).is_integer() else None

    for H, W in dict.fromkeys(sizes):
        for tx, ty in ((-1.0, -1.0), (-0.5, -0.5), (W - 0.5, H - 0.5), (1.0, 1.0)):
            x, y = at(tx, W), at(ty, H)
            if x is not None:
                out.append((x, 128.0, 1.0))
            if y is not None:
                out.append((128.0, y, 1.0))
            if x is not None and y is not None:
                out.append((x, y, 1.0))
    return list(dict.fromkeys(out))


def lattice_verts(B, N, sizes, seed):
    """(B, N, 3) float32 lattice vertices with the special vertices in the first slots (of sample 0, running on into the
    next samples where N is smaller than their number) and the patch vertices in the first slots of sample 1 (behind
    the special ones where there is one sample only, or where the special ones reach into sample 1).  Returns
    ``(verts, slots)`` with ``slots`` = {name: flat vertex index} for 'huge', 'depth', 'ys', 'xs', 'both'."""
    rng = np.random.default_rng(seed)
    v = np.empty((B * N, 3), dtype=np.float64)
    v[:, :2] = rng.integers(-256, 1281, (B * N, 2)) / 4.0
    v[:, 2] = rng.choice([0.5, 1.0, 2.0], B * N)
    sp = special_verts(sizes)
    first_patch = N if (B > 1 and N >= len(sp)) else len(sp)
    assert first_patch + len(PATCH_VERTS) <= B * N
    v[:len(sp)] = sp
    v[first_patch:first_patch + 4] = PATCH_VERTS
    slots = {"huge": sp.index(HUGE_VERT)}
    slots.update({name: first_patch + i for i, name in enumerate(("depth", "ys", "xs", "both"))})
    return v.astype(np.float32).reshape(B, N, 3), slots


def assert_geometry_exact(verts, sizes, inexact_quotient_rows=()):
    """The precondition of the strict bounds: the kernel's fp32 chain (bilinear_setup on the grid coordinates of project, in
    numpy float32, operation by operation) equals its float64 evaluation for every vertex and every map size — pixel
    coordinates, floors, the four weight factors and their four products.  A vertex all of whose corners are out of range
    on an axis in both evaluations (the huge one) need not agree beyond that.  The quotients ``x / z / 256`` themselves
    must be exact too, except on the flat rows ``inexact_quotient_rows`` (the depth-patched row divides by float32(0.1))."""
    from oracle.pooling import project
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    pr = project(v[None], IDENTITY)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        q32 = {}
        for name, num in (("xs", "p1"), ("ys", "p0")):
            p2 = pr["p2"][0].astype(np.float32)
            q = pr[num][0].astype(np.float32) / p2 / np.float32(256.0)
            q32[name] = np.where(pr[name + "_patched"][0], np.float32(0.5), q).astype(np.float32)
            inexact = np.nonzero(q32[name].astype(np.float64) != pr[name][0])[0]
            assert set(inexact.tolist()) <= set(inexact_quotient_rows), (name, inexact[:8])
        for H, W in dict.fromkeys(sizes):
            per_axis = []
            for q, size in ((q32["ys"], W), (q32["xs"], H)):
                g = q * np.float32(2.0) - np.float32(1.0)
                i32 = ((g + np.float32(1.0)) / np.float32(2.0)) * np.float32(size - 1)
                f32 = np.floor(i32)
                w32 = (f32 + np.float32(1.0) - i32, i32 - f32)
                i64 = q.astype(np.float64) * (size - 1)
                f64 = np.floor(i64)
                w64 = (f64 + 1.0 - i64, i64 - f64)
                assert i32.dtype == np.float32 and w32[0].dtype == np.float32
                far = ((i32 <= -1) | (i32 >= size)) & ((i64 <= -1) | (i64 >= size))
                same = (i32 == i64) & (f32 == f64) & (w32[0] == w64[0]) & (w32[1] == w64[1])
                assert bool((same | far).all()), (H, W, np.nonzero(~(same | far))[0][:8])
                per_axis.append((w32, w64, far))
            (wx32, wx64, farx), (wy32, wy64, fary) = per_axis
            live = ~(farx | fary)
            for a in range(2):
                for b in range(2):
                    p32 = wx32[a] * wy32[b]
                    assert p32.dtype == np.float32
                    assert bool((p32.astype(np.float64) == wx64[a] * wy64[b])[live].all()), (H, W, a, b)


def lattice_case(B, N, shapes, seed):
    """One seeded case: ``shapes`` = [(C, H, W), ...].  float32 numpy arrays ``verts`` (B, N, 3), ``maps`` (B, C, H, W) each,
    ``grad_out`` and ``base`` (B, N, sum C), and the slots of ``lattice_verts``."""
    sizes = [(h, w) for _, h, w in shapes]
    verts, slots = lattice_verts(B, N, sizes, seed)
    rng = np.random.default_rng(seed + 1)
    maps = [rng.standard_normal((B, c, h, w), dtype=np.float32) for c, h, w in shapes]
    ld = sum(c for c, _, _ in shapes)
    grad_out = rng.standard_normal((B, N, ld), dtype=np.float32)
    base = rng.standard_normal((B, N, ld), dtype=np.float32)
    return {"verts": verts, "maps": maps, "grad_out": grad_out, "base": base, "slots": slots, "sizes": sizes}
