"""-m gpu: the image-feature pooling kernels (csrc/pooling.hip, a3vt_image_pool_fwd / _fwd_add / _bwd) against the explicit
float64 reference oracle.pooling.pool_reference, element by element, on inputs whose fp32 geometry is exact (pool_lattice).

With exact pixel coordinates and weights, what is left of the kernel's error is the rounding of its fp32 sums, and every
element gets its own bound from the sum of the magnitudes of its terms (u = 2^-24):

  features        |err| <= K_F u (sum |w m| + |base|)
  map gradients   |err| <= K_M u sum |w g| + N 2^-40 max |g| of the channel block
  vertex gradient |err| <= K_V u S,  S = |M|^T [2 Ax inv, 2 Ay inv, (2 Ax |p0| + 2 Ay |p1|) inv / |p2|]

K = the fp32 roundings on the longest path to the output, counted in the kernel source without FMA contraction:

  K_F = 8   pool_fwd(2)_kernel: four products, three sums (the first goes to a zero accumulator), the sum with `base`.
  K_M = 2   pool_bwd_maps_body: the product w * g and the conversion of the integer sum to fp32.  The fixed-point
            quantisation is the second term: a term is rounded to 2^-shift, shift = 62 - e - c with 2^e <= 2 max|g| and
            2^c <= 2 N, i.e. by at most N 2^-61 max|g|; N terms per pixel at the most -> N^2 2^-61 max|g| < N 2^-40 max|g|.
  K_V = 32  pool_bwd_verts_kernel (the longer one): per term a product with the weight factor, three sums and the product
            with g (5); the lane's sum over 4 channels and 2 passes (8); the map's scale factor and the sum over four maps
            (5); six butterfly levels (6); 1 / (256 p2), the two products, the sum, the product and the quotient of the p2
            term (5); the matrix row: a product and two sums (3).  pool_bwd_verts2_kernel: 5 + 4 + 2 + 6 + 5 + 3 = 25.

An element whose terms are all zero (every corner out of range, a coordinate cut by a patch) has bound 0: it must be exactly 0.
The one inexact division of the lattice inputs is the depth-patched row's (by float32(0.1)); there the reference takes the
float32 quotient (f32_quotients), which is again on the lattice (100 / 256, 200 / 256), so that row is bounded like every other.
"""
import numpy as np
import pytest
import torch

import pool_lattice as pl
from helpers import assert_grad_close, rel_err
from oracle.pooling import pool_reference

pytestmark = pytest.mark.gpu

K_F, K_M, K_V = 8, 2, 32
U = 2.0 ** -24

CASES = {
    "pyramid": (3, 700, [(64, 23, 23), (128, 7, 7), (256, 3, 3)]),
    "nonsquare": (2, 900, [(8, 5, 9), (12, 17, 3), (4, 1, 5), (4, 9, 1)]),
    "two_per_trip": (7, 10001, [(4, 5, 9), (4, 3, 3), (8, 9, 5)]),
    "fallback": (1, 32771, [(260, 3, 5), (128, 5, 3), (64, 3, 3), (64, 2, 2)]),
    "fallback_small": (2, 300, [(260, 3, 5), (128, 5, 3), (64, 3, 3), (64, 2, 2)]),
    "one_map": (2, 500, [(4, 7, 7)]),
    "cb12": (512, 7, [(12, 3, 3)]),
    "cb_split": (511, 7, [(12, 3, 3)]),
    "lds_full": (2, 600, [(8, 32, 32)]),
}


def channel_block(B, C, H, W):
    """The channel block launch_pool_bwd gives a map (None: refused), restated to find the block of a channel."""
    cb = C
    while cb > 4 and (H * W * cb > 8192 or cb > 256):
        cb >>= 1
    if H * W * cb > 8192:
        return None
    while cb > 8 and B * -(-C // cb) < 512:
        cb >>= 1
    return (cb + 3) & ~3


def _matrix():
    return torch.tensor(pl.IDENTITY, dtype=torch.float32)


def _device(case, cuda, with_base=False, channels_last=False, backward=True, matrix=None):
    """One evaluation on the GPU -> numpy arrays: feats, grad_maps, grad_verts (and grad_base)."""
    from a3vt_amd import ops
    v = torch.from_numpy(case["verts"]).to(cuda).requires_grad_(True)
    ms = [torch.from_numpy(m).to(cuda) for m in case["maps"]]
    if channels_last:
        ms = [m.contiguous(memory_format=torch.channels_last) for m in ms]
    ms = [m.requires_grad_(True) for m in ms]
    base = torch.from_numpy(case["base"]).to(cuda).requires_grad_(True) if with_base else None
    f = ops.image_pool(v, _matrix() if matrix is None else matrix, ms, base=base)
    out = {"feats": f.detach().cpu().numpy()}
    if backward:
        f.backward(torch.from_numpy(case["grad_out"]).to(cuda))
        out["grad_maps"] = [m.grad.cpu().numpy() for m in ms]
        out["grad_verts"] = v.grad.cpu().numpy()
        if with_base:
            out["grad_base"] = base.grad.cpu().numpy()
    return out


def _block_max(case):
    """max |grad_out| over the vertices of a sample and the channels of a channel block, per map as (B, C, 1, 1)."""
    g = np.abs(case["grad_out"].astype(np.float64))
    B, out, off = g.shape[0], [], 0
    for m in case["maps"]:
        _, C, H, W = m.shape
        cb = channel_block(B, C, H, W)
        mx = np.empty((B, C))
        for c0 in range(0, C, cb):
            mx[:, c0:c0 + cb] = g[:, :, off + c0:off + min(c0 + cb, C)].max(axis=(1, 2))[:, None]
        out.append(mx[:, :, None, None])
        off += C
    return out


def _ratio(dev, ref, bound, what, mask=None):
    """Asserts |dev - ref| <= bound for EVERY element (of the mask) and returns the largest err / bound."""
    err = np.abs(dev.astype(np.float64) - ref)
    ok = err <= bound
    if mask is not None:
        ok = ok | ~mask
        err, bound = np.where(mask, err, 0.0), np.where(mask, bound, 0.0)
    worst = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    if not ok.all():
        i = np.unravel_index(np.argmax(np.where(ok, 0.0, err)), err.shape)
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} elements out of bound; worst err/bound {worst:.3g}; at {i} "
                             f"device {dev[i]!r} reference {ref[i]!r} bound {bound[i]!r}")
    return worst


def _check(name, case, dev, ref, with_base, masks=None):
    """Features (with or without base), map gradients and vertex gradient of one evaluation against the reference."""
    masks = masks or {}
    N = case["verts"].shape[1]
    r = {"feats": _ratio(dev["feats"], ref["feats"], K_F * U * ref["abs_feats"], f"{name}: feats (base={with_base})")}
    if "grad_maps" in dev:
        r["maps"] = 0.0
        for k, bm in enumerate(_block_max(case)):
            bound = K_M * U * ref["abs_grad_maps"][k] + N * 2.0 ** -40 * bm
            r["maps"] = max(r["maps"], _ratio(dev["grad_maps"][k], ref["grad_maps"][k], bound, f"{name}: grad_maps[{k}]",
                                              masks.get(("maps", k))))
        r["verts"] = _ratio(dev["grad_verts"], ref["grad_verts"], K_V * U * ref["abs_grad_verts"], f"{name}: grad_verts",
                            masks.get("verts"))
    print(f"POOL err/bound {name} base={int(with_base)}: " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    return r


def _run_case(name, case, cuda, inexact_rows=()):
    pl.assert_geometry_exact(case["verts"], case["sizes"], inexact_quotient_rows=inexact_rows)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = pool_reference(case["maps"], case["verts"], pl.IDENTITY, grad_out=case["grad_out"], f32_quotients=True)
    dev = _device(case, cuda)
    _check(name, case, dev, ref, False)
    # the sum with `base` in the pooling's own pass: the same fp32 add, so base + pooled bit for bit, and within the bound
    # of the reference with base; the gradient of base is the output gradient itself, the others do not change
    devb = _device(case, cuda, with_base=True)
    base = case["base"].astype(np.float64)
    _check(name, case, {"feats": devb["feats"]}, {"feats": base + ref["feats"], "abs_feats": np.abs(base) + ref["abs_feats"]}, True)
    assert np.array_equal(devb["feats"], case["base"] + dev["feats"])
    assert np.array_equal(devb["grad_base"], case["grad_out"])
    assert np.array_equal(devb["grad_verts"], dev["grad_verts"])
    assert all(np.array_equal(a, b) for a, b in zip(devb["grad_maps"], dev["grad_maps"]))
    return dev, ref


@pytest.mark.parametrize("name", list(CASES))
def test_lattice_case(cuda, name):
    """Forward, forward with base and backward of one case against pool_reference under the bounds of the module docstring,
    no element left out.  What each case reaches:
      pyramid         the default maps, with the pixel-hit and patch vertices
      nonsquare       H != W, a 1-wide and a 1-high map, four maps, a last channel block narrower than the others (8 + 4)
      two_per_trip    m = 70007 > 65536: the second vertex of a trip, a second grid-stride trip whose second vertex is off
      fallback        516 channels: pool_fwd_kernel / pool_bwd_verts_kernel, their second channel pass, their grid stride
      fallback_small  the same kernels in one trip
      one_map         one lane of 64 busy
      cb12            channel block 12: 3 lanes per vertex, 85 vertices in flight, thread 255 idle
      cb_split        channel block 8 of 12 channels: the last block 4 wide
      lds_full        H W CB = 8192: the largest LDS image (65536 B of dynamic LDS)."""
    B, N, shapes = CASES[name]
    blocks = [channel_block(B, *s) for s in shapes]
    if name == "nonsquare":
        assert blocks[1] == 8 and len(shapes) == 4
    if name == "two_per_trip":
        assert B * N > 65536 + 4 and B * N < 65536 + 32768
    if name.startswith("fallback"):
        assert sum(s[0] for s in shapes) > 512 and (name != "fallback" or B * N > 32768)
    if name in ("cb12", "cb_split"):
        assert blocks == [12 if name == "cb12" else 8]
    if name == "lds_full":
        assert shapes[0][1] * shapes[0][2] * blocks[0] == 8192
    case = pl.lattice_case(B, N, shapes, seed=sum(map(ord, name)))
    s = case["slots"]
    dev, ref = _run_case(name, case, cuda, inexact_rows=(s["depth"],))
    # the rows that are zero by construction
    gv, f = dev["grad_verts"].reshape(-1, 3), dev["feats"].reshape(B * N, -1)
    assert not gv[s["huge"]].any() and gv[s["depth"], 2] == 0 and gv[s["ys"], 0] == 0 and gv[s["xs"], 1] == 0
    assert not gv[s["both"]].any()
    assert gv[s["depth"], 0] != 0 and gv[s["ys"], 1] != 0 and gv[s["xs"], 0] != 0
    off = 0
    for c, h, w in shapes:
        if h > 1 and w > 1:
            assert not f[s["huge"], off:off + c].any()
        off += c


@pytest.mark.parametrize("pos", ["interior", "corner"])
def test_pile_up(cuda, pos):
    """4096 identical vertices with identical output-gradient rows: 4096 same-sign terms in each accumulator, the largest
    1e6, beside a channel of the same block that holds 1e-6.  At an interior non-integer point, and at ix = W - 1,
    iy = H - 1 (one corner in range, weight 1).  The same bounds."""
    B, N, shapes = 1, 4096, [(8, 5, 5)]
    case = pl.lattice_case(B, N, shapes, seed=77)
    case["verts"][:] = (100.25, 57.5, 1.0) if pos == "interior" else (256.0, 256.0, 1.0)
    row = case["grad_out"][0, 0].copy()
    row[2], row[5] = 1e6, 1e-6
    assert np.abs(row).max() == np.float32(1e6) and channel_block(B, *shapes[0]) == 8
    case["grad_out"][:] = row
    _run_case(f"pile_up_{pos}", case, cuda)


def test_real_camera_nonsquare_maps(cuda):
    """The camera matrix, vertices as in test_image_pool_fwd_bwd (far off-screen ones included), maps 8x5x9 and 16x13x6,
    against the float64 reference under that test's criteria (the geometry is not fp32-exact here): H and W may not be
    swapped anywhere."""
    from a3vt_amd import ops
    from oracle import gcn as og
    B, N = 3, 700
    g = torch.Generator().manual_seed(13)
    verts = (torch.rand(B, N, 3, generator=g) - 0.5) * 0.5
    verts[:, :40] *= 6.0
    maps = [torch.randn(B, 8, 5, 9, generator=g), torch.randn(B, 16, 13, 6, generator=g)]
    gout = torch.randn(B, N, 24, generator=g)
    matrix = og.projection_matrix().float()
    ref = pool_reference([m.numpy() for m in maps], verts.numpy(), matrix.numpy(), grad_out=gout.numpy())
    vd = verts.to(cuda).requires_grad_(True)
    md = [m.to(cuda).requires_grad_(True) for m in maps]
    f = ops.image_pool(vd, matrix, md)
    f.backward(gout.to(cuda))
    assert rel_err(f, torch.from_numpy(ref["feats"])) < 1e-5
    for k in range(2):
        assert rel_err(md[k].grad, torch.from_numpy(ref["grad_maps"][k])) < 1e-5
    assert_grad_close(vd.grad, torch.from_numpy(ref["grad_verts"]), "grad_verts")
    # and the reference's own statement of the same thing
    v64 = verts.double().requires_grad_(True)
    f_o = og.image_pooling([m.double() for m in maps], v64)
    (f_o * gout.double()).sum().backward()
    assert rel_err(f, f_o) < 1e-5
    assert_grad_close(vd.grad, v64.grad, "grad_verts (grid_sample)")


@pytest.mark.parametrize("name", ["two_per_trip", "fallback_small"])
def test_bits(cuda, name):
    """A second evaluation reproduces every output bit (the map gradients accumulate in fixed point), and channels-last
    maps give the same bits as contiguous ones."""
    B, N, shapes = CASES[name]
    case = pl.lattice_case(B, N, shapes, seed=sum(map(ord, name)))
    a = _device(case, cuda, with_base=True)
    for other in (_device(case, cuda, with_base=True), _device(case, cuda, with_base=True, channels_last=True)):
        assert np.array_equal(a["feats"], other["feats"]) and np.array_equal(a["grad_verts"], other["grad_verts"])
        assert all(np.array_equal(x, y) for x, y in zip(a["grad_maps"], other["grad_maps"]))
        assert np.array_equal(other["grad_base"], case["grad_out"])


@pytest.mark.parametrize("value", [float("nan"), float("inf"), 3.2e38], ids=["nan", "inf", "3.2e38"])
def test_nonfinite_output_gradient(cuda, value):
    """One element of grad_out (sample 0, last vertex — moved to an interior point —, channel 3 of the second map) is NaN,
    infinite, or finite above 3e38.  NaN / inf: every map-gradient element that is not finite in the reference is not finite
    on the device; device elements that are not finite lie in that sample and that map only (the channel block is poisoned
    as a whole, which is the documented behaviour); everything else, the other sample included, keeps its bounds; that
    vertex's gradient is not finite.  3.2e38: the reference is finite, so the device is, within the bounds (one vertex on the
    pixel with weight < 1: the sum stays below FLT_MAX).  That vertex's own position gradient (3.2e38 times a pixel
    difference) may overflow fp32 and is not compared."""
    B, N, shapes = 2, 300, [(8, 5, 5), (16, 3, 3)]
    case = pl.lattice_case(B, N, shapes, seed=31)
    case["verts"][0, N - 1] = (100.25, 57.5, 1.0)
    case["grad_out"][0, N - 1, 8 + 3] = value
    pl.assert_geometry_exact(case["verts"], case["sizes"], inexact_quotient_rows=(case["slots"]["depth"],))
    with np.errstate(invalid="ignore", over="ignore"):
        ref = pool_reference(case["maps"], case["verts"], pl.IDENTITY, grad_out=case["grad_out"], f32_quotients=True)
    dev = _device(case, cuda)
    ref_bad = [~np.isfinite(g) for g in ref["grad_maps"]]
    dev_bad = [~np.isfinite(g) for g in dev["grad_maps"]]
    vmask = np.ones((B, N, 3), dtype=bool)
    vmask[0, N - 1] = False
    if np.isfinite(value):
        assert not any(b.any() for b in ref_bad + dev_bad)
    else:
        assert ref_bad[1][0, 3].any() and not ref_bad[0].any() and not ref_bad[1][1].any()
        assert all((d | ~r).all() for r, d in zip(ref_bad, dev_bad))            # reference not finite -> device not finite
        assert not dev_bad[0].any() and not dev_bad[1][1].any()                # only that sample and that map
        assert not np.isfinite(dev["grad_verts"][0, N - 1]).all()
    assert np.isfinite(dev["grad_verts"][vmask]).all()
    masks = {("maps", k): ~(ref_bad[k] | dev_bad[k]) for k in range(2)}
    masks["verts"] = vmask
    # (the block maximum of the bounds: over the finite values; the poisoned block itself is masked out)
    bound_case = dict(case, grad_out=np.where(np.isfinite(case["grad_out"]), case["grad_out"], np.float32(0)))
    with np.errstate(invalid="ignore", over="ignore"):
        _check(f"nonfinite_{value}", bound_case, dev, ref, False, masks)


def test_refusals(cuda):
    """What the library refuses: a map too large for the backward's LDS image (its forward runs, and matches), a channel
    count that is not a multiple of 4, more than four maps."""
    from a3vt_amd import ops
    B, N, shapes = 1, 300, [(4, 46, 46)]
    assert channel_block(B, *shapes[0]) is None
    case = pl.lattice_case(B, N, shapes, seed=46)
    pl.assert_geometry_exact(case["verts"], case["sizes"], inexact_quotient_rows=(case["slots"]["depth"],))
    ref = pool_reference(case["maps"], case["verts"], pl.IDENTITY, f32_quotients=True)
    _check("refused_46x46 forward", case, _device(case, cuda, backward=False), ref, False)
    with pytest.raises(RuntimeError, match="too large for the LDS image"):
        _device(case, cuda)
    v = torch.from_numpy(case["verts"]).to(cuda)
    with pytest.raises(RuntimeError):
        ops.image_pool(v, _matrix(), [torch.zeros(B, 6, 3, 3, device=cuda)])
    with pytest.raises(RuntimeError):
        ops.image_pool(v, _matrix(), [torch.zeros(B, 4, 3, 3, device=cuda) for _ in range(5)])
