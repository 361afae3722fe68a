"""A rounding-aware float64 reference of the vertex-feature encoder (Positional_Encoder + Mask_Encoder + their sum), for the
edge tests of csrc/posenc.hip and csrc/posenc_wide.hip.  Plain torch on the CPU; it shares no code with the kernels or
with oracle/gcn.py.

    e(p)  = [sin(a_i), cos(a_i)]_{i = 0..9} ++ p,   a_i = float32(float32(f_i) * p),  f_0 = pi, f_i = 2 pi i
    feats = W3 relu(W2 relu(W1 e + b1) + b2) + b3 + Emb[clamp(trunc(mask), 0, 3)]

The ONE place where this differs from the float64 oracle: the sin / cos argument is the float32 product of the
float32-rounded frequency and the float32 position — what both kernels and the float32 original compute — and only then
widened.  At |p| = 0.3 the argument reaches 17 rad, where a float32 ulp is 1.9e-6: an oracle that forms the argument in
float64 differs from ANY float32 evaluation by that much, which is what kept the old bounds at 1e-5 / 1e-4.  The position
derivative uses the same rounded frequency: d sin(a_i)/dp = float32(f_i) cos(a_i), d cos(a_i)/dp = -float32(f_i) sin(a_i).
Everything else (products, sums, sin, cos) is float64.  `evaluate(..., dtype=torch.float32)` runs the very same formula in
float32 on the CPU: its distance from the float64 run is the yardstick the GPU bounds are taken from.

ReLU kinks.  A pre-activation within rounding of zero may land on either side of it in two correct float32 evaluations,
which switches that unit's gradient on or off: a jump, not a rounding error.  `near_kink` marks the vertices where any
first- or second-layer |pre-activation| < tau and `make_case` zeroes their upstream-gradient rows, so that such a vertex
contributes nothing to any gradient whichever side the kernel's own summation order lands on (its features are still
compared).  Every gradient comparison can then be tight and elementwise.

Numbers (measured by tests/test_posenc_ref_host.py on the CPU, which prints them; inputs from `make_case`):

  TAU = 1e-6.  The largest |pre-activation(float32 CPU) - pre-activation(reference)| is 8.2e-7 (I = 50, m = 65 557, twelve
  seeds, |p| <= 0.3 and 1.5; 7.3e-7 over the shapes the host test measures): a 63-term float32 sum whose partial sums reach 1.7.  Sixteen times
  that, 1.3e-5, would mark 1.1e-3 .. 1.7e-3 of the vertices at m = 65 557 — over the cap below — so TAU is NOT widened to
  it: 1e-6 is the smallest round figure above the measured error.  A smaller tau zeroes fewer rows and can only make a
  gradient comparison fail, never pass: were a kernel's pre-activation to land on the other side of zero at an unmarked
  vertex (its error would have to exceed 1e-6), that vertex's gradient would be off by ~1e-2, not by 1e-5.
  The host test asserts measured < TAU.
  Share of vertices marked (= upstream rows zeroed) at TAU = 1e-6, I = 50, m = 65 557: 1.4e-4 at |p| <= 0.3, 1.2e-4 at
  |p| <= 1.5.  Below m = 1000 a single marked vertex is over the cap, so the small cases have none (their seeds are chosen
  so; about 4e-6 of all pre-activations lie within 1e-6 of zero).  `make_case` asserts the share <= MAX_KINK_SHARE = 1e-3
  (a condition on the test's inputs: it fails, it does not skip) and records it in case["kink_share"]; the GPU tests print
  it per case.

  BOUNDS: 16 x the float32-CPU-versus-reference error of each tensor on that tensor's largest reference element
  (helpers.rel_err); the table is in tests/test_gpu_posenc_edges.py, the constants are below.
"""
import math

import numpy as np
import torch

NAMES = ["positional_encoder.model.0.weight", "positional_encoder.model.0.bias",
         "positional_encoder.model.2.weight", "positional_encoder.model.2.bias",
         "positional_encoder.model.4.weight", "positional_encoder.model.4.bias", "mask_encoder.model.0.weight"]
SHORT = ["dW1", "db1", "dW2", "db2", "dW3", "db3", "dEmb"]

TAU = 1e-6
MAX_KINK_SHARE = 1e-3

# the hand-written mask of the token tests: truncation toward zero and the clamp to 0..3 -> tokens 0 0 0 0 1 2 3 3 3 3
HAND_MASK = [-2.0, -0.5, 0.0, 0.9, 1.5, 2.999, 3.0, 3.7, 7.0, 1e6]

# float32-CPU-versus-reference errors (rel_err per tensor), the largest over the shapes test_posenc_ref_host.py measures,
# rounded up to two digits (the float32 evaluation uses elementwise operations only: the same figures on every CPU);
# every GPU bound is 16 x its figure
CPU_FIGURES = {
    "feats": 9.5e-8,
    "grad_verts": 5.4e-7,
    "weights": 5.0e-7,          # each of dW1, db1, dW2, db2, dW3, db3 on its own scale, m <= 2048
    "weights_large": 1.7e-6,    # the same at m > 2048 (float32 sums over up to 65 557 rows)
    "emb": 1.5e-7,              # dEmb, m <= 2048
    "emb_large": 8.5e-7,        # dEmb, m > 2048
}
BOUNDS = {k: 16 * v for k, v in CPU_FIGURES.items()}
assert BOUNDS["feats"] <= 1e-5 and max(v for k, v in BOUNDS.items() if k != "feats") <= 1e-4   # never looser than the old ones

# float32(f_i): f_0 = pi, f_i = 2 pi i (a float64 product rounded once)
FREQ32 = np.array([np.pi if i == 0 else np.pi * 2 * i for i in range(10)], dtype=np.float64).astype(np.float32)


def param_shapes(I):
    h1, h2 = I // 4, I // 2
    return [(h1, 63), (h1,), (h2, h1), (h2,), (I, h2), (I,), (4, I)]


def make_params(I, seed):
    """The seven float32 parameter tensors in state-dict order: Linear weights and biases uniform in +-1/sqrt(fan_in), the
    embedding standard normal (torch's defaults)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for shp in param_shapes(I)[:6]:
        fan_in = shp[1] if len(shp) == 2 else {I // 4: 63, I // 2: I // 4, I: I // 2}[shp[0]]
        out.append(((torch.rand(shp, generator=g, dtype=torch.float64) * 2 - 1) / math.sqrt(fan_in)).float())
    out.append(torch.randn(4, I, generator=g, dtype=torch.float64).float())
    return out


def pack(tensors):
    """Seven tensors in state-dict order -> the packed vector of a3vt_posenc_mask_fwd."""
    return torch.cat([t.reshape(-1) for t in tensors])


def unpack(vec, I):
    out, off = [], 0
    for shp in param_shapes(I):
        n = int(np.prod(shp))
        out.append(vec[off:off + n].reshape(shp))
        off += n
    assert off == vec.numel()
    return out


def tokens(mask):
    """clamp(trunc(mask), 0, 3): mask.long() for legal masks plus the clamp both kernels apply."""
    return torch.clamp(torch.trunc(mask.reshape(-1).double()), 0, 3).long()


def embed(p, dtype):
    """p (M, 3) float32 -> (e (M, 63), sin (M, 10, 3), cos (M, 10, 3)) in `dtype`; the argument is the float32 product.
    In float32 sin / cos are the float64 values rounded once (a float32 libm differs from CPU to CPU)."""
    arg = torch.from_numpy(FREQ32)[None, :, None] * p.float()[:, None, :]        # float32, rounded once
    arg = arg.double()
    s, c = torch.sin(arg).to(dtype), torch.cos(arg).to(dtype)
    e = torch.cat([torch.cat([s, c], dim=2).reshape(p.shape[0], 60), p.to(dtype)], dim=1)   # 6 i + c: sin, 6 i + 3 + c: cos
    return e, s, c


# Products.  float64: BLAS.  float32: elementwise multiplies and adds only, one rounding each and in a fixed order, so that
# the yardstick is the same number on every CPU (a float32 BLAS blocks its sums by the machine's vector width: the dW3 error
# at m = 65 557 came out as 4e-7 on one CPU and 1e-5 on another).
def _mm(a, b, bias=None):
    """a (M, K) @ b (K, N) (+ bias): in float32 the K terms are added one after the other, starting from the bias — the
    order of the scalar forward kernel."""
    if a.dtype == torch.float64:
        return a @ b if bias is None else a @ b + bias
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=a.dtype) if bias is None else bias.expand(a.shape[0], -1).clone()
    for k in range(a.shape[1]):
        acc = acc + a[:, k:k + 1] * b[k:k + 1, :]
    return acc


def _tmm(a, b, block=64):
    """a^T b, a sum over the M rows: in float32, blocks of 64 rows summed row after row, then the blocks one after the other
    (the shape of the kernels' sums: a workgroup's rows, then the slabs in order)."""
    if a.dtype == torch.float64:
        return a.t() @ b
    M, nb = a.shape[0], (a.shape[0] + block - 1) // block
    pad = nb * block - M
    a3 = torch.cat([a, a.new_zeros(pad, a.shape[1])]).reshape(nb, block, -1)
    b3 = torch.cat([b, b.new_zeros(pad, b.shape[1])]).reshape(nb, block, -1)
    acc = torch.zeros(nb, a.shape[1], b.shape[1], dtype=a.dtype)
    for r in range(block):
        acc = acc + a3[:, r, :, None] * b3[:, r, None, :]
    total = acc[0]
    for i in range(1, nb):
        total = total + acc[i]
    return total


def evaluate(verts, mask, params, gout=None, dtype=torch.float64):
    """Forward and hand-written backward in `dtype` (float64: the reference; float32: the CPU yardstick).
    verts (..., 3) float32, mask (..., 1) float32, params: seven float32 tensors, gout (..., I) or None.
    Returns a dict: feats (M, I), pre1 (M, I/4), pre2 (M, I/2) and, with gout, grad_verts (M, 3) and grad_params (list of 7)."""
    p = verts.reshape(-1, 3)
    W1, b1, W2, b2, W3, b3, Emb = [t.to(dtype) for t in params]
    tok = tokens(mask)
    e, s, c = embed(p, dtype)
    pre1 = _mm(e, W1.t(), b1)
    h1 = pre1.clamp_min(0)
    pre2 = _mm(h1, W2.t(), b2)
    h2 = pre2.clamp_min(0)
    out = {"feats": _mm(h2, W3.t(), b3) + Emb[tok], "pre1": pre1, "pre2": pre2, "tok": tok}
    if gout is None:
        return out
    g = gout.reshape(p.shape[0], -1).to(dtype)
    ones = torch.ones(p.shape[0], 1, dtype=dtype)
    onehot = torch.nn.functional.one_hot(tok, 4).to(dtype)
    d2 = _mm(g, W3) * (pre2 > 0)
    d1 = _mm(d2, W2) * (pre1 > 0)
    de = _mm(d1, W1)
    f = torch.from_numpy(FREQ32).to(dtype)[None, :, None]
    de_sc = de[:, :60].reshape(-1, 10, 6)
    terms = f * (c * de_sc[:, :, :3] - s * de_sc[:, :, 3:])
    gp = de[:, 60:]
    for i in range(10):
        gp = gp + terms[:, i]
    out["grad_verts"] = gp
    out["grad_params"] = [_tmm(d1, e), _tmm(d1, ones)[:, 0], _tmm(d2, h1), _tmm(d2, ones)[:, 0], _tmm(g, h2), _tmm(g, ones)[:, 0],
                          _tmm(onehot, g)]
    return out


def evaluate_autograd(verts, mask, params, gout):
    """The float64 reference once more, by autograd through a surrogate argument whose VALUE is the float32 product and whose
    derivative is float32(f_i): checks the hand-written backward of `evaluate`."""
    p32 = verts.reshape(-1, 3).float()
    p = p32.double().requires_grad_(True)
    ps = [t.double().requires_grad_(True) for t in params]
    f = torch.from_numpy(FREQ32).double()[None, :, None]
    arg32 = (torch.from_numpy(FREQ32)[None, :, None] * p32[:, None, :]).double()
    lin = f * p[:, None, :]
    arg = lin + (arg32 - lin).detach()
    e = torch.cat([torch.cat([torch.sin(arg), torch.cos(arg)], dim=2).reshape(-1, 60), p], dim=1)
    h = torch.relu(torch.nn.functional.linear(e, ps[0], ps[1]))
    h = torch.relu(torch.nn.functional.linear(h, ps[2], ps[3]))
    feats = torch.nn.functional.linear(h, ps[4], ps[5]) + ps[6][tokens(mask)]
    (feats * gout.reshape(feats.shape).double()).sum().backward()
    return {"feats": feats.detach(), "grad_verts": p.grad, "grad_params": [t.grad for t in ps]}


def near_kink(pre1, pre2, tau=TAU):
    """(M,) bool: vertices where any first- or second-layer |pre-activation| < tau."""
    return (pre1.abs() < tau).any(dim=1) | (pre2.abs() < tau).any(dim=1)


def make_case(B, N, I=50, ld=None, seed=0, pmax=0.3, mask=None, params=None, gscale=None, tau=TAU):
    """Seeded inputs + the float64 reference of one test case.
    verts uniform in [-pmax, pmax]; mask uniform integers 0..3 unless given ((B, N, 1) float32); gout standard normal times
    `gscale` (None, or a (B * N,) tensor of per-vertex factors), its pad columns (>= I) zero, and the rows of near-kink
    vertices zeroed.  Returns a dict of float32 inputs (verts, mask, params, packed, gout (B, N, ld)), the reference `ref`
    (see `evaluate`; from the zeroed gout), `kink` (M,) bool and `kink_share`."""
    ld = I if ld is None else ld
    g = torch.Generator().manual_seed(1000 * seed + I)
    verts = (torch.rand(B, N, 3, generator=g) * 2 - 1) * pmax
    rmask = torch.randint(0, 4, (B, N, 1), generator=g).float()
    mask = rmask if mask is None else mask.reshape(B, N, 1).float()
    params = make_params(I, seed + 17) if params is None else params
    gout = torch.zeros(B, N, ld)
    gout[..., :I] = torch.randn(B, N, I, generator=g)
    if gscale is not None:
        gout *= gscale.reshape(B, N, 1)
    fwd = evaluate(verts, mask, params)
    kink = near_kink(fwd["pre1"], fwd["pre2"], tau)
    share = kink.double().mean().item()
    assert share <= MAX_KINK_SHARE, f"{share:.2e} of the vertices lie within {tau} of a ReLU kink (cap {MAX_KINK_SHARE})"
    gout.reshape(B * N, ld)[kink] = 0
    ref = evaluate(verts, mask, params, gout[..., :I])
    return {"B": B, "N": N, "I": I, "ld": ld, "verts": verts, "mask": mask, "params": params, "packed": pack(params),
            "gout": gout, "ref": ref, "kink": kink, "kink_share": share}

