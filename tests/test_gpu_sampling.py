"""-m gpu: the surface-sampling kernels (csrc/sample.hip: face_cdf_kernel, sample_fwd_kernel, sample_bwd_kernel) against the
float64 reference oracle.chamfer and the exact host emulation tests/philox_ref.py, element by element.  What is exact is
asserted bit for bit (the Philox stream, the search, the CDF's zero steps, repeatability); what is rounded gets its own bound
per element, a named multiple of u = 2^-24 counted in the kernel source (an FMA contraction only removes a rounding).

CDF (face_cdf_kernel), c_f = sum_{g <= f} p_g, p_g = a_g / tot, in float64; per = faces per thread, nt = busy threads:

  |cdf_f - c_f| <= u [K_S c_f + K_A (H c_f + H_f)],   h_g = |e1||e2| / 2 >= a_g,  H_f = sum_{g <= f} h_g / tot,  H = H_last

  K_A = 11   the area: an edge difference (1), a product of two (3), the difference of two products (+1 on the sum of their
             magnitudes): |dn| <= 4 u sqrt(3) |e1||e2|, i.e. 7 u h on the area; the three squares and two sums (3, halved by
             the root: 1.5), the root (2): 3.5 u a <= 3.5 u h.  Relative to h, not a: a needle's area is a cancelled difference.
  K_S = 4 per + 2 nt + 2   the total is a serial sum of per terms per chunk, then of nt chunk sums: (per + nt) u of itself,
             and it divides every p; the quotient (1); the scan: the chunk sums (per, in parallel) and their serial sum (nt)
             make a base, a chunk adds per terms to it, and a chunk that starts with a zero-area face is joined to its
             predecessor by additions of local sums (per more): 3 per + nt; 1 for the second-order terms (K^2 u < 0.03).
             Adding the 0 of an empty thread is exact, hence nt and not 256.

  A face is certain to get an interval of its own when p_f exceeds this bound at f: the entry before it and the chunk's
  base are two fp32 sums of the same quotients, each within the scan's share of the bound of the exact sum, so the base plus
  a quotient above the whole bound lies above that entry by more than one spacing.

Points (sample_fwd_kernel), per coordinate d, M_d = max(|A_d|, |B_d|, |C_d|), against the float64 blend of the same fp32
(face, u, v):   |err| <= K_P u M_d,   K_P = 12: the root (1); w0 = 1 - su (2 absolute), w1 = su (1 - v) (3), w2 = su v (2):
7 on sum_k |dw_k| |X_k|; three products with sum_k w_k = 1 (1), two sums (2); 2 for second order and sum_k w_k = 1 + O(u).

Vertex gradient (sample_bwd_kernel), per vertex coordinate, over the terms (sample, corner k) that land on the vertex:

  |err| <= u [K_B sum |w_k g| + sum_{k = 0} sqrt(u_s) |g|] + n 2^(e + c - 62)

  K_B = 5    w1 = su (1 - v): root, difference, product (3 relative); the product with g (1); the conversion of the integer
             sum to fp32 (1).  w2 needs 4, and w0 = 1 - su needs 3 relative to itself ...
  ... plus the root's rounding, which is relative to su and not to the difference 1 - su: u su |g|, the second sum.  Without it
             no K holds: at su = 1 - 2^-24 half an ulp of su is all of w0.
  n 2^(e + c - 62): the fixed-point quantum of common.h's fix_scale, one per term: 2^e > max |grad_points| of the MESH
             (frexp), 2^c > draws * num.  It also covers a product that underflows to a subnormal.
A vertex no term lands on has bound 0: it must be exactly 0.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import philox_ref as pr
from helpers import template
from oracle import chamfer as och

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
K_A, K_P, K_B = 11, 12, 5
BWD_TILE = 6144                    # kSampleBwdTile


def k_s(F):
    per = pr.chunk_size(F)
    return 4 * per + 2 * -(-F // per) + 2


def _ratio(dev, ref, bound, what):
    """Asserts |dev - ref| <= bound for EVERY element and returns the largest err / bound."""
    err = np.abs(np.asarray(dev, dtype=np.float64) - ref)
    ok = err <= bound
    worst = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    if not ok.all():
        i = np.unravel_index(np.argmax(np.where(ok, 0.0, err)), err.shape)
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} elements out of bound; worst err/bound {worst:.3g}; at {i} "
                             f"device {dev[i]!r} reference {ref[i]!r} bound {bound[i]!r}")
    print(f"SAMPLING err/bound {what}: {worst:.4f}")
    return worst


# ---- CDF -------------------------------------------------------------------------------------------------------------------

def soup(B, F, seed, zero):
    """B triangle soups of F faces: verts (B, 3F, 3) float32, faces (F, 3) int64; zero (B, F): the faces whose three
    vertices are made one point."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1.0, 1.0, (B, F, 3, 3)).astype(np.float32)
    v[zero] = v[zero][:, :1]
    return torch.from_numpy(v.reshape(B, 3 * F, 3)), torch.arange(3 * F).reshape(F, 3)


def zero_faces(F, seed):
    """(3, F) masks of zero-area faces.  Mesh 0: face 0, the last three faces, the first and the last face of every chunk
    (when a chunk has more than two faces), a run of four across a chunk boundary, 5 % at random.  Mesh 1: the same without
    face 0 and the last face.  Mesh 2: 5 % at random only."""
    rng = np.random.default_rng(seed)
    per = pr.chunk_size(F)
    z = rng.random((3, F)) < 0.05
    if F < 8:
        return np.zeros((3, F), dtype=bool)
    for m in (0, 1):
        z[m, 0] = True
        z[m, -3:] = True
        if per > 2:
            z[m, ::per] = True
            z[m, per - 1::per] = True
        mid = per * max(1, (F // per) // 2)
        z[m, mid - 2:mid + 2] = True
    z[1, 0] = z[1, -1] = False
    assert not z.all(axis=1).any()
    return z


def device_cdf(cuda, verts, faces):
    from a3vt_amd import lib
    L = lib.load()
    vd, fd = verts.to(cuda).contiguous(), faces.to(torch.int32).to(cuda).contiguous()
    B, N, F = verts.shape[0], verts.shape[1], faces.shape[0]
    cdf = torch.full((B, F), -1.0, device=cuda)
    lib.check(L.a3vt_face_cdf(lib.ptr(vd), lib.ptr(fd), B, N, F, lib.ptr(cdf), None), "face_cdf")
    torch.cuda.synchronize()
    return cdf.cpu().numpy()


def cdf_reference(verts, faces):
    """float64: p (B, F) from oracle.chamfer.face_probabilities, its running sum, and h / tot with its running sum."""
    v = verts.double()
    p = och.face_probabilities(v, faces).numpy()
    tri = v[:, faces].numpy()
    e1, e2 = tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0]
    h = 0.5 * np.linalg.norm(e1, axis=-1) * np.linalg.norm(e2, axis=-1)
    a = 0.5 * np.linalg.norm(np.cross(e1, e2), axis=-1)
    h = np.where(np.isfinite(a), h, 0.0)                     # a face with a NaN corner: area 0 exactly, in both
    tot = np.nansum(a, axis=1, keepdims=True)
    return p, np.cumsum(p, axis=1), h / tot


def check_cdf(cdf, p, c, hn, F, what):
    """The four assertions of the CDF on (B, F) arrays; returns err / bound."""
    prev = np.concatenate([np.zeros((cdf.shape[0], 1), dtype=np.float32), cdf[:, :-1]], axis=1)
    assert cdf.dtype == np.float32 and (cdf >= prev).all(), f"{what}: the CDF steps down at {np.argwhere(cdf < prev)[:5]}"
    zero = p == 0
    assert np.array_equal(cdf[zero], prev[zero]), \
        f"{what}: {int((cdf[zero] != prev[zero]).sum())} of {int(zero.sum())} zero-area faces have an interval of their own"
    bound = U * (k_s(F) * c + K_A * (hn.sum(axis=1, keepdims=True) * c + np.cumsum(hn, axis=1)))
    sure = p > bound
    assert (cdf[sure] > prev[sure]).all(), f"{what}: a face of probability {p[sure][cdf[sure] <= prev[sure]][0]} has no interval"
    return _ratio(cdf, c, bound, what), int(zero.sum()), int(sure.sum())


@pytest.mark.parametrize("F", [1, 80, 256, 257, 1000, 1280, 5120])
def test_cdf_soup(cuda, F):
    """a3vt_face_cdf on three triangle soups with the zero-area faces of zero_faces: never a step down, a zero-area face
    repeats its predecessor bit for bit (cdf[0] == 0 when it is face 0), every face whose probability exceeds the bound steps up,
    and every entry is within the module docstring's bound of the float64 running sum of oracle.chamfer's probabilities.
    F = 1, 80: per = 1 with idle threads; 256 | 257: per 1 -> 2; 1000: per = 4, threads 250..255 idle; 1280: per = 5;
    5120: per = 20."""
    per = pr.chunk_size(F)
    assert per == {1: 1, 80: 1, 256: 1, 257: 2, 1000: 4, 1280: 5, 5120: 20}[F]
    zero = zero_faces(F, F)
    verts, faces = soup(3, F, 100 + F, zero)
    p, c, hn = cdf_reference(verts, faces)
    assert np.array_equal(p == 0, zero)
    cdf = device_cdf(cuda, verts, faces)
    if zero[0, 0]:
        assert cdf[0, 0] == 0.0
    _, nz, ns = check_cdf(cdf, p, c, hn, F, f"cdf F={F}")
    assert nz == zero.sum() and ns >= 0.75 * (~zero).sum()   # (the threshold leaves out few faces)
    if per > 2:                                               # the chunk starts and ends are among the zero faces
        assert zero[0, ::per].all() and zero[0, per - 1::per].all() and zero[1, per::per].all()


def test_cdf_scrubs(cuda):
    """The reference's NaN scrubs (utils.py:166-168) in one batch of perturbed ico3 meshes (1280 faces, per = 5): a normal
    mesh; one with a NaN vertex, whose faces get step 0 while the rest keeps the bound and ends at 1; one with every vertex
    at one point, whose CDF is 1, 2, ..., F exactly."""
    v, f = template("ico3")
    F = f.shape[0]
    g = torch.Generator().manual_seed(3)
    verts = torch.from_numpy(v)[None].repeat(3, 1, 1) + 0.02 * torch.randn(3, v.shape[0], 3, generator=g)
    verts[1, 7, 1] = float("nan")
    verts[2] = verts[2, 0].clone()
    faces = torch.from_numpy(f)
    with np.errstate(invalid="ignore"):
        p, c, hn = cdf_reference(verts, faces)
    nan_faces = (f == 7).any(axis=1)
    assert 5 <= nan_faces.sum() <= 6 and np.array_equal(p[1] == 0, nan_faces) and (p[2] == 1).all() and (p[0] > 0).all()
    cdf = device_cdf(cuda, verts, faces)
    assert np.array_equal(cdf[2], np.arange(1, F + 1, dtype=np.float32))
    check_cdf(cdf[:2], p[:2], c[:2], hn[:2], F, "cdf scrubs")
    assert abs(float(cdf[1, -1]) - 1.0) <= U * (k_s(F) + 2 * K_A * hn[1].sum())


# ---- search ----------------------------------------------------------------------------------------------------------------

def raw_forward(cuda, verts, faces, cdf, draws, num, seed, offset):
    """a3vt_sample_points_fwd on a CDF given as a host array -> face_idx, u, v, points as numpy arrays."""
    from a3vt_amd import lib
    L = lib.load()
    B, N, F = verts.shape[0], verts.shape[1], faces.shape[0]
    vd, fd = verts.to(cuda).contiguous(), faces.to(torch.int32).to(cuda).contiguous()
    cd = torch.from_numpy(np.ascontiguousarray(cdf, dtype=np.float32)).to(cuda)
    fi = torch.full((draws, B, num), -1, dtype=torch.int32, device=cuda)
    uu, vv = torch.empty(draws, B, num, device=cuda), torch.empty(draws, B, num, device=cuda)
    pts = torch.empty(draws, B, num, 3, device=cuda)
    lib.check(L.a3vt_sample_points_fwd(lib.ptr(vd), lib.ptr(fd), lib.ptr(cd), B, N, F, draws, num, None, None, None, seed, offset,
                                       lib.ptr(pts), lib.ptr(fi), lib.ptr(uu), lib.ptr(vv), None), "sample_points_fwd")
    torch.cuda.synchronize()
    return fi.cpu().numpy(), uu.cpu().numpy(), vv.cpu().numpy(), pts.cpu().numpy()


def handmade_cdfs(name):
    """Three CDFs (3, F) float32 with totals 1, 3.7 and F."""
    if name == "single":
        steps = np.ones((3, 1))
    elif name == "ties":                                      # at the start, in the middle, at the end
        steps = np.array([[0, 0, 0, 1, 2, 0, 0, 3, 3, 1, 0, 0]] * 3, dtype=np.float64)
        steps[1] = [0, 2, 0, 0, 0, 0, 5, 1, 0, 1, 1, 0]
        steps[2] = [1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0]
    else:                                                     # F = 1000: a quarter of the faces tied, runs at both ends
        rng = np.random.default_rng(5)
        steps = rng.uniform(0.1, 1.0, (3, 1000)) * (rng.random((3, 1000)) > 0.25)
        steps[:, :7] = 0
        steps[:2, -9:] = 0
    F = steps.shape[1]
    c = np.cumsum(steps, axis=1)
    c = (c / c[:, -1:] * np.array([[1.0], [3.7], [float(F)]])).astype(np.float32)
    c = np.maximum.accumulate(c, axis=1)
    tied = np.diff(np.concatenate([np.zeros((3, 1), dtype=np.float32), c], axis=1), axis=1) == 0
    assert np.array_equal(tied, steps == 0)                   # the rounding to fp32 neither made nor broke a tie
    return c, tied


@pytest.mark.parametrize("name", ["single", "ties", "f1000"])
def test_search_on_handmade_cdfs(cuda, name):
    """sample_fwd_kernel's search on CDFs built on the host (ties at the start, in the middle and at the end; totals 1, 3.7
    and F; one face; 1000 faces), 2 x 3 x 700 = 4200 samples (not a multiple of 256): faces, u and v equal the emulation
    exactly, and no tied, zero-width face is ever returned."""
    cdf, tied = handmade_cdfs(name)
    F = cdf.shape[1]
    verts, faces = soup(3, F, 11, np.zeros((3, F), dtype=bool))
    draws, num, seed, offset = 2, 700, 0x1234567887654321, 99
    fi, uu, vv, _ = raw_forward(cuda, verts, faces, cdf, draws, num, seed, offset)
    ef, eu, ev = pr.emulate_draws(cdf, seed, offset, draws, 3, num)
    assert np.array_equal(fi, ef) and np.array_equal(uu, eu) and np.array_equal(vv, ev)
    for b in range(3):
        assert not tied[b][fi[:, b]].any()
        if F > 1:
            assert len(np.unique(fi[:, b])) > 1


# ---- Philox stream ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ico2_batch():
    v, f = template("ico2")
    g = torch.Generator().manual_seed(21)
    verts = torch.from_numpy(v)[None].repeat(3, 1, 1) + 0.03 * torch.randn(3, v.shape[0], 3, generator=g)
    return verts, torch.from_numpy(f)


def test_uint64_words_reach_the_library_unharmed():
    """lib.py declares seed and offset as c_uint64: the largest values of test_philox_stream convert without loss."""
    from a3vt_amd import lib
    assert lib.SIGNATURES["a3vt_sample_points_fwd"][1][11:13] == [ctypes.c_uint64, ctypes.c_uint64]
    for x in (0, 1, 2 ** 32 - 3, 0xDEADBEEFCAFEF00D, 2 ** 64 - 5, 2 ** 64 - 1):
        assert ctypes.c_uint64(x).value == x


@pytest.mark.parametrize("offset", [0, 2 ** 32 - 3, 2 ** 64 - 5])
@pytest.mark.parametrize("seed", [0, 1, 0xDEADBEEFCAFEF00D, 2 ** 64 - 1])
def test_philox_stream(cuda, seed, offset):
    """ops.sample_points(..., return_samples=True) on three perturbed ico2 meshes, 2 draws of 700: u and v are bit-equal to
    the emulation (the offsets carry into the counter's high word and wrap at 2^64 inside the launch), the faces equal the
    emulation's search of the CDF read back from the device, sample 0 of seed 0 / offset 0 is the published known answer,
    the points are within K_P u M of the float64 blend, and re-injecting (face, u, v) returns the same bits."""
    from a3vt_amd import ops
    verts, faces = ico2_batch()
    draws, num, B = 2, 700, 3
    vd, fd = verts.to(cuda), faces.to(torch.int32).to(cuda)
    pts, fi, uu, vv = ops.sample_points(vd, fd, num, draws, seed=seed, offset=offset, return_samples=True)
    cdf = device_cdf(cuda, verts, faces)
    ef, eu, ev = pr.emulate_draws(cdf, seed, offset, draws, B, num)
    assert np.array_equal(uu.cpu().numpy(), eu) and np.array_equal(vv.cpu().numpy(), ev)
    assert np.array_equal(fi.cpu().numpy(), ef)
    if seed == 0 and offset == 0:
        assert uu[0, 0, 0].item() == 0xe169c5 * 2.0 ** -24 == (0xe169c58d >> 8) * 2.0 ** -24
        assert vv[0, 0, 0].item() == 0xbc57ac * 2.0 ** -24 == (0xbc57ac4c >> 8) * 2.0 ** -24
    fl, u64, v64 = fi.cpu().long(), uu.cpu().double(), vv.cpu().double()
    ref = torch.stack([och.sample_points(verts.double(), faces, fl[r], u64[r], v64[r]) for r in range(draws)]).numpy()
    tri = verts.double()[:, faces].abs().numpy()              # (B, F, 3 corners, 3)
    M = np.stack([tri[np.arange(B)[:, None], fl[r].numpy()].max(axis=2) for r in range(draws)])
    _ratio(pts.cpu().numpy(), ref, K_P * U * M, f"points seed={seed:#x} offset={offset:#x}")
    again = ops.SamplePointsFn.apply(vd, fd, num, draws, 0, 0, fi, uu, vv)
    assert torch.equal(again, pts)


# ---- backward --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def bwd_case(n_vert):
    """2000 faces with corners anywhere in [0, n_vert) (most straddle the backward's vertex tiles), the last ones on every
    tile's edges {v0 - 1, v0, v1 - 1} and with repeated corners; 2 meshes, 2 draws of 1500 samples (the 1024-thread loop takes a
    second, ragged turn), the first of them on those special faces."""
    rng = np.random.default_rng(n_vert)
    F, B, draws, num = 2000, 2, 2, 1500
    tiles = -(-n_vert // BWD_TILE)
    tile = -(-n_vert // tiles)
    faces = rng.integers(0, n_vert, (F, 3))
    special = [[max(t * tile - 1, 0), t * tile, min(n_vert, (t + 1) * tile) - 1] for t in range(tiles)]
    special += [[5, 5, 9], [9, 5, 9], [n_vert - 1, 17, 17], [33, 33, 33], [tile - 1, tile - 1, min(tile, n_vert - 1)]]
    faces[F - len(special):] = special
    fi = rng.integers(0, F, (draws, B, num))
    fi[:, :, :2 * len(special)] = np.tile(np.arange(F - len(special), F), 2)
    u = rng.random((draws, B, num), dtype=np.float32)
    v = rng.random((draws, B, num), dtype=np.float32)
    u[0, 0, 0], u[0, 0, 1], v[0, 0, 2], v[0, 0, 3] = 0.0, 1.0 - 2.0 ** -24, 0.0, 1.0 - 2.0 ** -24
    gp = rng.standard_normal((draws, B, num, 3)).astype(np.float32)
    return dict(n_vert=n_vert, tiles=tiles, tile=tile, faces=torch.from_numpy(faces), fi=torch.from_numpy(fi), u=torch.from_numpy(u),
                v=torch.from_numpy(v), gp=torch.from_numpy(gp), dims=(F, B, draws, num))


def bwd_reference(case, gp):
    """float64 autograd of oracle.chamfer.sample_points for the output gradient gp (fp32 values), and the terms of the
    bound: (grad, sum |w g|, sum over corner 0 of sqrt(u) |g|, number of terms), each (B, n_vert, 3)."""
    F, B, draws, num = case["dims"]
    n = case["n_vert"]
    fi, u, v = case["fi"], case["u"].double(), case["v"].double()
    x = torch.zeros(B, n, 3, dtype=torch.float64, requires_grad=True)
    pts = torch.stack([och.sample_points(x, case["faces"], fi[r], u[r], v[r]) for r in range(draws)])
    pts.backward(gp.double())
    w = np.stack([t.numpy() for t in och.barycentric(u, v)], axis=-1)          # (draws, B, num, 3 corners)
    corner = case["faces"].numpy()[fi.numpy()]                                  # (draws, B, num, 3 corners)
    ag = np.abs(gp.double().numpy())                                            # (draws, B, num, 3)
    mesh = np.broadcast_to(np.arange(B)[None, :, None, None], corner.shape)
    absw, root, count = np.zeros((B, n, 3)), np.zeros((B, n, 3)), np.zeros((B, n, 3))
    np.add.at(absw, (mesh, corner), w[..., None] * ag[:, :, :, None, :])
    np.add.at(count, (mesh, corner), 1.0)
    np.add.at(root, (mesh[..., 0], corner[..., 0]), np.sqrt(u.numpy())[..., None] * ag)
    return x.grad.numpy(), absw, root, count


def bwd_bound(case, gp, absw, root, count):
    F, B, draws, num = case["dims"]
    c = 1
    while (1 << c) <= draws * num:
        c += 1
    mx = gp.abs().amax(dim=(0, 2, 3)).numpy()                                   # per mesh, fp32
    e = np.frexp(mx)[1].astype(np.float64)
    return U * (K_B * absw + root) + count * (2.0 ** (e + c - 62))[:, None, None]


def bwd_device(cuda, case, gp):
    from a3vt_amd import ops
    F, B, draws, num = case["dims"]
    x = torch.zeros(B, case["n_vert"], 3, device=cuda, requires_grad=True)
    pts = ops.SamplePointsFn.apply(x, case["faces"].to(torch.int32).to(cuda), num, draws, 0, 0,
                                   case["fi"].to(torch.int32).to(cuda), case["u"].to(cuda), case["v"].to(cuda))
    pts.backward(gp.to(cuda))
    return x.grad.cpu().numpy()


@pytest.mark.parametrize("n_vert", [6144, 6145, 12289])
def test_backward_bound(cuda, n_vert):
    """The vertex gradient against float64 autograd, every element under the module docstring's bound.  6144: one full
    144 KiB tile; 6145: two tiles of 3073; 12289: three of 4097.  A vertex that no sample touches is exactly 0; an all-zero
    grad_points gives exact zeros everywhere (mx == 0); a second call returns the same bits."""
    case = bwd_case(n_vert)
    assert (case["tiles"], case["tile"]) == {6144: (1, 6144), 6145: (2, 3073), 12289: (3, 4097)}[n_vert]
    ref, absw, root, count = bwd_reference(case, case["gp"])
    dev = bwd_device(cuda, case, case["gp"])
    assert (count == 0).any() and (count > 3).any()
    assert not dev[count == 0].any()
    _ratio(dev, ref, bwd_bound(case, case["gp"], absw, root, count), f"grad_verts n_vert={n_vert}")
    if case["tiles"] > 1:                                     # faces do straddle the tiles
        t = case["faces"].numpy() // case["tile"]
        assert (t.min(axis=1) != t.max(axis=1)).mean() > 0.4
    assert np.array_equal(bwd_device(cuda, case, case["gp"]), dev)
    zero = bwd_device(cuda, case, torch.zeros_like(case["gp"]))
    assert not zero.any()


@pytest.mark.parametrize("n_vert", [6144, 12289])
def test_backward_scale_is_per_mesh(cuda, n_vert):
    """Mesh 0's output gradients times 1e30 and mesh 1's times 1e-30 in one call: the fixed-point scale belongs to the
    workgroup, i.e. to the mesh, so each mesh meets the bound at its own scale."""
    case = bwd_case(n_vert)
    gp = case["gp"].clone()
    gp[:, 0] *= 1e30
    gp[:, 1] *= 1e-30
    assert torch.isfinite(gp).all() and gp[:, 1].abs().max() < 1e-29
    ref, absw, root, count = bwd_reference(case, gp)
    dev = bwd_device(cuda, case, gp)
    bound = bwd_bound(case, gp, absw, root, count)
    for b in range(2):
        _ratio(dev[b], ref[b], bound[b], f"grad_verts n_vert={n_vert} mesh {b} scaled")
    assert np.abs(dev[1]).max() > 1e-31 and not dev[count == 0].any()


@pytest.mark.parametrize("value", [float("inf"), float("-inf"), float("nan")], ids=["inf", "-inf", "nan"])
@pytest.mark.parametrize("n_vert", [6145])
def test_backward_nonfinite_poisons_its_mesh_only(cuda, n_vert, value):
    """One Inf or NaN in mesh 1's grad_points (second draw, past the first 1024 samples): mesh 1's gradient is NaN in every
    element, of every tile; mesh 0 meets the bound."""
    case = bwd_case(n_vert)
    gp = case["gp"].clone()
    gp[1, 1, 1300, 2] = value
    dev = bwd_device(cuda, case, gp)
    assert np.isnan(dev[1]).all()
    clean = gp.clone()
    clean[1, 1, 1300, 2] = 0.0
    ref, absw, root, count = bwd_reference(case, clean)
    bound = bwd_bound(case, clean, absw, root, count)
    _ratio(dev[0], ref[0], bound[0], f"grad_verts n_vert={n_vert} mesh 0 beside {value}")
