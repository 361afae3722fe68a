"""Host references of csrc/chamfer.hip's gradient and reduction kernels for the tests (plain module, numpy only, no fixtures, no
torch): the closed-form gradient in float64 with what a per-element error bound needs (grad, scales, bound), common.h's fixed-point
shift (fix_shift), the kernel's arithmetic in numpy float32 (emulate), clouds on a binary grid with their exact integer search
(grid_cloud, nn_first), a float64 brute-force search (nn_float64), the float64 reduction (reduce), and the index tables and cases
the host and the GPU tests share (tile_edges, scatter_tables, EXACT_CASES, exact_case, BOUNDED_*).

The gradient, with g = gcd[b] / draws (x (draws,B,P,3), y (B,Q,3), ixy (draws,B,P) into y[b], iyx (draws,B,Q) into x[r,b]):

    gx[r,b,i] = g [ (2/P)(x_i - y_ixy[r,b,i]) + (2/Q) sum_{j: iyx[r,b,j] = i} (x_i - y_j) ]
    gy[b,j]   = g sum_r [ (2/Q)(y_j - x_iyx[r,b,j]) + (2/P) sum_{i: ixy[r,b,i] = j} (y_j - x_i) ]

Both are ct * (direct terms) + cs * (scattered terms) with ct = 2 g / nt, cs = 2 g / ns over nsrc source clouds: for gx the
target cloud is x[r,b] (nt = P), its one source y[b] (ns = Q); for gy the target is y[b] (nt = Q), its sources the draws x[:,b].

The bound of an fp32 evaluation, per element, u = 2^-24:

    |v - v64| <= u [ (nsrc + 8) |ct| A + 9 |cs| Bm ] + |cs| n 2^-shift + 2^-149

A: the sum of the magnitudes of the element's direct terms, Bm: of its scattered terms, n: how many of those there are.  Counted in
the kernel: a direct term's difference (1) and the nsrc - 1 additions of the direct sum; a scattered term's difference (1) and the
conversion of the integer sum to fp32 (1); six more for 1/draws, g, 2/n, ct or cs, the product and the final sum (a fused
multiply-add only removes one); one for second order.  n 2^-shift: one fixed-point quantum per scattered term (each is rounded to
an integer of 2^-shift; the integer sum is exact).  2^-149: a result that is a subnormal.
"""
import collections
import functools

import numpy as np

U = 2.0 ** -24
DENORM = 2.0 ** -149
F32 = np.float32
BWD_TILE = 6144                     # kBwdTile of csrc/chamfer.hip


# ---- the float64 gradient ------------------------------------------------------------------------------------------------------

Grad = collections.namedtuple("Grad", "gx gy Ax Bx nx Ay By ny")


def _scatter(shape, index, terms):
    """(sum, sum of magnitudes, count) of `terms` (..., 3) at `index` (a tuple of index arrays) of an array of `shape` (..., 3)."""
    s, m = np.zeros(shape), np.zeros(shape)
    n = np.zeros(shape[:-1], dtype=np.int64)
    np.add.at(s, index, terms)
    np.add.at(m, index, np.abs(terms))
    np.add.at(n, index, 1)
    return s, m, n


def grad(x, y, ixy, iyx, gcd):
    """float64 gradient of sum_b gcd[b] cd[b] for the given index tables.  Returns Grad: gx (draws,B,P,3), gy (B,Q,3) and per
    output element A (sum of |direct term|), B (sum of |scattered term|), both unscaled differences, and per point n (number of
    scattered terms): Ax, Bx like gx, nx (draws,B,P); Ay, By like gy, ny (B,Q)."""
    x, y, gcd = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(gcd, dtype=np.float64)
    ixy, iyx = np.asarray(ixy, dtype=np.int64), np.asarray(iyx, dtype=np.int64)
    R, B, P, _ = x.shape
    Q = y.shape[1]
    assert y.shape == (B, Q, 3) and ixy.shape == (R, B, P) and iyx.shape == (R, B, Q) and gcd.shape == (B,)
    assert ixy.min() >= 0 and ixy.max() < Q and iyx.min() >= 0 and iyx.max() < P
    r_, b_ = np.arange(R)[:, None, None], np.arange(B)[None, :, None]
    a = x - y[b_, ixy]                                   # x_i - y_nn(i)   (R,B,P,3): direct for x, scattered (negated) onto y
    d = x[r_, b_, iyx] - y[None]                         # x_nn(j) - y_j   (R,B,Q,3): scattered onto x, direct (negated) for y
    sx, mx, nx = _scatter(x.shape, (np.broadcast_to(r_, iyx.shape), np.broadcast_to(b_, iyx.shape), iyx), d)
    sy, my, ny = _scatter(y.shape, (np.broadcast_to(b_, ixy.shape), ixy), -a)
    g = gcd / R
    gx = g[None, :, None, None] * ((2.0 / P) * a + (2.0 / Q) * sx)
    gy = g[:, None, None] * ((2.0 / Q) * (-d).sum(axis=0) + (2.0 / P) * sy)
    return Grad(gx, gy, np.abs(a), mx, nx, np.abs(d).sum(axis=0), my, ny)


def fix_shift(bound32, count):
    """common.h's fix_scale: 62 - e - c with bound32 = m 2^e, 0.5 <= m < 1 (e = 0 for 0) and 2^c > count."""
    _, e = np.frexp(F32(bound32))
    c = 1
    while (1 << c) <= int(count):
        c += 1
    return 62 - int(e) - c


def _absmax32(a, axes):
    return np.abs(np.asarray(a, dtype=F32)).max(axis=axes)


Scales = collections.namedtuple("Scales", "ct cs shift nsrc")


def scales(x, y, gcd):
    """(for gx, for gy): float64 ct, cs and the integer fixed-point shift per target cloud — shapes (draws,B) and (B,) — and
    nsrc.  The kernel's bound is max|T| + max|S| over the clouds involved, the two maxima added once in fp32."""
    R, B, P, _ = x.shape
    Q = y.shape[1]
    g = np.asarray(gcd, dtype=np.float64) / R
    mx, my = _absmax32(x, (2, 3)), _absmax32(y, (1, 2))                                    # (R,B), (B,)
    bx = mx + my[None]                                                                     # fp32 + fp32 -> fp32
    by = my + mx.max(axis=0)
    assert bx.dtype == F32 and by.dtype == F32
    shx = np.array([[fix_shift(bx[r, b], Q) for b in range(B)] for r in range(R)], dtype=np.int64)
    shy = np.array([fix_shift(by[b], R * P) for b in range(B)], dtype=np.int64)
    return (Scales(np.broadcast_to(g * 2.0 / P, (R, B)), np.broadcast_to(g * 2.0 / Q, (R, B)), shx, 1),
            Scales(g * 2.0 / Q, g * 2.0 / P, shy, R))


def bound(A, Bm, n, sc):
    """The per-element bound of the module docstring; A, Bm (..., pts, 3), n (..., pts), sc: the matching Scales."""
    ct, cs = np.abs(sc.ct)[..., None, None], np.abs(sc.cs)[..., None, None]
    quantum = np.ldexp(1.0, -sc.shift)[..., None, None]
    b = U * ((sc.nsrc + 8) * ct * A + 9 * cs * Bm) + cs * n[..., None] * quantum
    return np.where((A == 0) & (n[..., None] == 0), 0.0, b + DENORM)


def bounds(gr, x, y, gcd):
    """(bound of gx, bound of gy) for gr = grad(x, y, ., ., gcd)."""
    sx, sy = scales(x, y, gcd)
    return bound(gr.Ax, gr.Bx, gr.nx, sx), bound(gr.Ay, gr.By, gr.ny, sy)


# ---- the kernel's arithmetic in numpy float32 --------------------------------------------------------------------------------------

def _fma(a, b, c):
    """fl32(a b + c) for fp32 a, b, c: the product is exact in float64, the sum is rounded to 53 bits before the 24 (a double
    rounding that moves a result by at most one more half ulp in 2^-29 of the cases: immaterial to a bound with a spare factor)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _emulate_one(T, S, t2s, s2t, g32, shift, fused):
    """One target cloud: T (nt,3) fp32, S (nsrc,ns,3) fp32, t2s (nsrc,nt), s2t (nsrc,ns), g32 = gcd * (1/draws) in fp32."""
    nt, (nsrc, ns, _) = T.shape[0], S.shape
    ct, cs = g32 * (F32(2.0) / F32(nt)), g32 * (F32(2.0) / F32(ns))
    direct = np.zeros((nt, 3), dtype=F32)
    acc = np.zeros((nt, 3), dtype=np.int64)
    for s in range(nsrc):
        direct = direct + (T - S[s][t2s[s]])                                              # fp32 difference, fp32 sum, in order
        term = T[s2t[s]] - S[s]                                                           # (ns,3) fp32
        np.add.at(acc, s2t[s], np.rint(np.ldexp(term.astype(np.float64), shift)).astype(np.int64))
    sc = np.ldexp(acc.astype(F32), -shift).astype(F32)
    if fused == "ct":
        return _fma(np.broadcast_to(ct, direct.shape), direct, cs * sc)
    if fused == "cs":
        return _fma(np.broadcast_to(cs, sc.shape), sc, ct * direct)
    assert fused is None
    return ct * direct + cs * sc


def emulate(x, y, ixy, iyx, gcd, fused=None):
    """chamfer_bwd_kernel's arithmetic on fp32 inputs: fp32 differences, integer accumulation at fix_shift (round to nearest
    even), conversion back, ct * direct + cs * scatter; `fused`: None, "ct" (fma(ct, direct, cs * scatter)) or "cs"
    (fma(cs, scatter, ct * direct)).  Returns (gx, gy) in fp32.  Finite inputs only."""
    x, y, gcd = np.asarray(x, dtype=F32), np.asarray(y, dtype=F32), np.asarray(gcd, dtype=F32)
    R, B, P, _ = x.shape
    sx, sy = scales(x, y, gcd)
    g32 = gcd * (F32(1.0) / F32(R))
    gx, gy = np.empty_like(x), np.empty_like(y)
    with np.errstate(under="ignore"):
        for b in range(B):
            for r in range(R):
                gx[r, b] = _emulate_one(x[r, b], y[b][None], ixy[r, b][None], iyx[r, b][None], g32[b], int(sx.shift[r, b]), fused)
            gy[b] = _emulate_one(y[b], x[:, b], iyx[:, b], ixy[:, b], g32[b], int(sy.shift[b]), fused)
    return gx, gy


# ---- clouds and searches -------------------------------------------------------------------------------------------------------------

def grid_cloud(rng, n, bits):
    """(n, 3) float64 coordinates k / 2^bits, k uniform in [-2^bits, 2^bits)."""
    return rng.integers(-(1 << bits), 1 << bits, (n, 3)).astype(np.float64) / (1 << bits)


def nn_first(x, y, bits=4):
    """Exact nearest neighbour of every row of the grid cloud x (P,3) in the grid cloud y (Q,3): (squared distance in units of
    4^-bits, int64 (P,); index of the first minimum, int64 (P,)).  |x|^2 + |y|^2 - 2 x.y on the integer coordinates, in float64:
    every intermediate is an integer far below 2^53."""
    kx, ky = np.asarray(x, dtype=np.float64) * (1 << bits), np.asarray(y, dtype=np.float64) * (1 << bits)
    assert np.array_equal(kx, np.rint(kx)) and np.array_equal(ky, np.rint(ky)), "not on the grid"
    assert max(np.abs(kx).max(), np.abs(ky).max()) < 2 ** 20
    d = (kx * kx).sum(axis=1)[:, None] + (ky * ky).sum(axis=1)[None, :] - 2.0 * (kx @ ky.T)
    idx = d.argmin(axis=1)                                                                # numpy: the first minimum
    return d[np.arange(len(kx)), idx].astype(np.int64), idx.astype(np.int64)


def nn_float64(x, y, chunk=1024):
    """float64 brute force, both directions from one distance matrix: (ixy (P,), iyx (Q,)), first minima."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    ixy = np.empty(len(x), dtype=np.int64)
    col, arg = np.full(len(y), np.inf), np.zeros(len(y), dtype=np.int64)
    for s in range(0, len(x), chunk):
        d = ((x[s:s + chunk, None, :] - y[None, :, :]) ** 2).sum(axis=-1)
        ixy[s:s + chunk] = d.argmin(axis=1)
        a = d.argmin(axis=0)
        m = d[a, np.arange(len(y))]
        better = m < col
        col[better], arg[better] = m[better], a[better] + s
    return ixy, arg


def reduce(dxy, dyx):
    """cd (B,) = (1/draws) sum_r (mean_i dxy[r,b,i] + mean_j dyx[r,b,j]) in float64."""
    dxy, dyx = np.asarray(dxy, dtype=np.float64), np.asarray(dyx, dtype=np.float64)
    return (dxy.mean(axis=2) + dyx.mean(axis=2)).mean(axis=0)


def k_reduce(p, q, draws):
    """Roundings on the longest path of chamfer_reduce_kernel: the per-thread serial sums, and 26 for two divisions, one sum,
    six butterfly levels, sixteen serial adds and 1/draws; one more serial add per draw."""
    return -(-p // 1024) + -(-q // 1024) + draws + 26


# ---- index tables ----------------------------------------------------------------------------------------------------------------

def tile_edges(n):
    """The launch's cut of n targets: (tile, [first index of the second, third, ... tile])."""
    tiles = -(-n // BWD_TILE)
    tile = -(-n // tiles)
    return tile, [k * tile for k in range(1, tiles)]


def random_table(rng, shape, n):
    """A random map into [0, n) with 0 and n - 1 present in every row (where the row has room)."""
    t = rng.integers(0, n, shape)
    if shape[-1] >= 2:
        t[..., 0], t[..., -1] = n - 1, 0
    return t


def scatter_tables(rng, shape, n):
    """The scatter tables of the exact cases, maps of `shape` (..., ns) into [0, n): {name: table}."""
    ns = shape[-1]
    tile, edges = tile_edges(n)
    out = {"random": random_table(rng, shape, n)}
    if ns == n:
        out["permutation"] = rng.permuted(np.broadcast_to(np.arange(n), shape), axis=-1)
    for hub in sorted({0, tile - 1, tile, n - 1} & set(range(n))):
        out[f"hub{hub}"] = np.full(shape, hub, dtype=np.int64)
    if edges:
        sides = np.array([e + o for e in edges for o in (-1, 0)])
        out["tile-edges"] = sides[rng.integers(0, len(sides), shape)]
        out["tile-edges"][..., :len(sides)] = sides[:ns]                                  # every side at least once
    return out


# (P, Q, draws, B).  8192 targets: two tiles of 4096; 16384: three of 5462, 5462, 5460.
EXACT_CASES = [(1, 1, 2, 3), (2, 1024, 4, 2), (1024, 1024, 1, 3), (8192, 8192, 4, 1), (16384, 2048, 2, 2), (2048, 16384, 1, 3)]
EXACT_BITS = 8
EXACT_GCD = (-0.125, 0.0, 32.0)     # powers of two of both signs and a zero (B = 2: the zero and one of the others; B = 1: one)


@functools.lru_cache(maxsize=None)
def exact_case(number):
    """x, y on the 2^-8 grid (float64), gcd, and {name: (ixy, iyx)} for EXACT_CASES[number]: every scatter table once as iyx
    beside a random ixy, once as ixy beside a random iyx.  Built once and shared: nobody writes into what this returns."""
    P, Q, R, B = EXACT_CASES[number]
    rng = np.random.default_rng(100 + number)
    x = grid_cloud(rng, R * B * P, EXACT_BITS).reshape(R, B, P, 3)
    y = grid_cloud(rng, B * Q, EXACT_BITS).reshape(B, Q, 3)
    gcd = np.roll(np.array(EXACT_GCD), number)[:B] if B != 2 else np.array([(32.0, 0.0), (0.0, -0.125)][number % 2])
    tables = {}
    for name, t in scatter_tables(rng, (R, B, Q), P).items():
        tables[f"x:{name}"] = (random_table(rng, (R, B, P), Q), t)
    for name, t in scatter_tables(rng, (R, B, P), Q).items():
        if name != "random":
            tables[f"y:{name}"] = (t, random_table(rng, (R, B, Q), P))
    return x, y, gcd, tables


def is_fp32(a):
    """Every value survives float64 -> float32 -> float64: the precondition of an exact case's expected values."""
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(over="ignore"):
        return bool(np.array_equal(a.astype(F32).astype(np.float64), a))


# ---- the bounded cases ---------------------------------------------------------------------------------------------------------------

BOUNDED_NT = (1023, 1024, 1025, 6143, 6144, 6145, 12288, 12289)   # 1 tile ... 1 full tile, 3073 + 3072, 2 full, 4097 + 4097 + 4095
BOUNDED_OTHER = 777
BOUNDED_DRAWS = 3
BOUNDED_CLOUDS = ("unit", "scale 1e-15", "scale 1e4", "offset", "one coordinate 1e6")
BOUNDED_GCD = (1.0, -0.37, 9000.0 / 16, 2.5e-3, -7.0)


def bounded_clouds(seed, P, Q, outlier=1e6):
    """x (3, 5, P, 3), y (5, Q, 3) float32: cloud b is BOUNDED_CLOUDS[b] (the single far coordinate sits in x[1, 4])."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, (BOUNDED_DRAWS, 5, P, 3))
    y = rng.uniform(-1.0, 1.0, (5, Q, 3))
    for a in (x, y):
        a[..., 1, :, :] *= 1e-15
        a[..., 2, :, :] *= 1e4
        a[..., 3, :, :] += np.array([1000.0, -2000.0, 500.0])
    x, y = x.astype(F32), y.astype(F32)
    x[1, 4, P // 2, 1] = outlier
    return x, y
