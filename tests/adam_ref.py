"""Host references of csrc/adam.hip for the tests (plain module, numpy only, no fixtures): one step of torch's ``_single_tensor_adam``
rule in float64 (step_fp64), a per-element first-order forward error bound for an fp32 evaluation of that rule (bound, margin), the
rule in numpy float32 in the kernel's order of operations, with or without fused multiply-adds and optionally deliberately wrong
(emulate_fp32, MUTANTS), and the settings and input recipes the host and the GPU tests share (SETTINGS, make_inputs).

The rule, per element (torch/optim/adam.py, amsgrad and maximize off; the clamp is this project's ``grad_clamp``):
    g' = clamp(g, -c, c)                                   (torch.clamp: +-Inf -> +-c, NaN stays NaN)
    g2 = g' + weight_decay * p                             (weight_decay != 0 only)
    m' = m + (g2 - m) * (1 - beta1)
    v' = v * beta2 + ((1 - beta2) * g2) * g2
    p' = p - step_size * (m' / (sqrt(v') / sqrt(1 - beta2^t) + eps)),   step_size = lr / (1 - beta1^t)
"""
import numpy as np

U = 2.0 ** -24                 # unit roundoff of fp32, round to nearest
DENORM = 2.0 ** -149           # the smallest fp32 denormal
F32 = np.float32

# lr, betas, eps, weight decay, step count, state (zero or prepared), clamp.  The first four are the magnitudes at which the rule's
# parts can be told apart: a first step from zero state (the bias corrections at their largest), a short resumed run with weight
# decay, a large eps with short betas (eps placement), and a long resumed run (beta^t underflows, both corrections are 1).  The
# fifth steps under the clamp with about a third of the gradients beyond it.
SETTINGS = [
    dict(name="first-step", lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1, zero_state=True, grad_clamp=None),
    dict(name="resumed-wd", lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, step=7, zero_state=False, grad_clamp=None),
    dict(name="large-eps", lr=1e-2, beta1=0.8, beta2=0.99, eps=1e-3, weight_decay=0.1, step=3, zero_state=False, grad_clamp=None),
    dict(name="step-100000", lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=100000, zero_state=False, grad_clamp=None),
    dict(name="clamped", lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, step=7, zero_state=False, grad_clamp=0.5),
]
HYPER_KEYS = ("lr", "beta1", "beta2", "eps", "weight_decay", "step", "grad_clamp")

MUTANTS = ("no_bias_correction1", "no_bias_correction2", "lerp_weight_beta1", "eps_inside_sqrt", "eps_before_bias_correction2",
           "quotient_from_old_m", "weight_decay_dropped", "clamp_written_only")
# the outputs each wrong rule corrupts (0 = p', 1 = m', 2 = v')
MUTANT_OUTPUTS = {"no_bias_correction1": (0,), "no_bias_correction2": (0,), "lerp_weight_beta1": (0, 1), "eps_inside_sqrt": (0,),
                  "eps_before_bias_correction2": (0,), "quotient_from_old_m": (0,), "weight_decay_dropped": (0, 1, 2),
                  "clamp_written_only": (0, 1, 2)}


def hyper(setting):
    """The keyword arguments of step_fp64 / bound / emulate_fp32 for one entry of SETTINGS."""
    return {k: setting[k] for k in HYPER_KEYS}


def make_inputs(rng, n, setting):
    """(p, g, m, v), each (n,) float32.  Magnitudes span many decades so that sqrt(v) lies below, at and above eps and the update
    is not hidden under the last rounding of p: g = N * 10^U(-10, 1), m = N * 10^U(-10, 0), v = (that recipe)^2, p = N * 10^U(-6, 0).
    Under a clamp the gradient is N * c / 0.9674 instead: P(|N| > 0.9674) = 1/3, a third of the elements lie beyond the clamp."""
    def spread(lo, hi):
        return rng.standard_normal(n) * 10.0 ** rng.uniform(lo, hi, n)
    p = spread(-6, 0).astype(F32)
    if setting["grad_clamp"] is None:
        g = spread(-10, 1).astype(F32)
    else:
        g = (rng.standard_normal(n) * (setting["grad_clamp"] / 0.9674)).astype(F32)
    m, v = spread(-10, 0).astype(F32), (spread(-10, 0) ** 2).astype(F32)
    if setting["zero_state"]:
        m, v = np.zeros(n, F32), np.zeros(n, F32)
    return p, g, m, v


def _f64(*xs):
    out = []
    for x in xs:
        x = np.asarray(x)
        assert x.dtype == F32, "the state is fp32"
        out.append(x.astype(np.float64))
    return out


def _clamp64(g, c):
    return g if c is None else np.where(np.isnan(g), g, np.minimum(np.maximum(g, -c), c))


def _intermediates(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_clamp):
    p, g, m, v = _f64(p, g, m, v)
    gc = _clamp64(g, grad_clamp)
    g2 = gc + weight_decay * p if weight_decay != 0 else gc
    m2 = m + (g2 - m) * (1.0 - beta1)
    a, b = v * beta2, ((1.0 - beta2) * g2) * g2
    v2 = a + b
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    step_size, bcs = lr / bc1, bc2 ** 0.5
    s = np.sqrt(v2)
    r = s / bcs
    denom = r + eps
    q = m2 / denom
    upd = step_size * q
    # Tensor.addcdiv_ evaluates p + (value * m') / denom: in that order p' is torch's own to the last bit, and one fp64 rounding from
    # the kernel's p - step_size * (m' / denom)
    return dict(p=p, g=g, m=m, v=v, gc=gc, g2=g2, m2=m2, a=a, b=b, v2=v2, step_size=step_size, bcs=bcs, s=s, r=r, denom=denom, q=q,
                upd=upd, p2=p + (-step_size * m2) / denom)


def step_fp64(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_clamp=None):
    """One step of the rule in float64 on fp32 state and double hyper-parameters -> (p', m', v', g_clamped), float64."""
    with np.errstate(all="ignore"):       # non-finite gradients are data here
        t = _intermediates(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_clamp)
    return t["p2"], t["m2"], t["v2"], t["gc"]


def bound(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_clamp=None, u=U):
    """First-order forward error bounds (bp, bm, bv), per element, for an fp32 evaluation of the rule as ``adam_one`` orders it.
    Every rounding contributes u times the magnitude of the value it rounds, propagated to the output with the exact (fp64) partial
    derivatives; products of two roundings are dropped.  Counted roundings, each a relative error of at most u = 2^-24:

      scalars rounded once on the host (8): clamp c, weight_decay, 1 - beta1, beta2, 1 - beta2, step_size, sqrt(1 - beta2^t), eps
      g2 (2 operations, weight decay only):  weight_decay * p, g' + .          -> E_g2 = |c - fl(c)| [clamped] + 2u|wd p| + u|g2|
      m' (3 operations):  d = g2 - m,  d * (1 - beta1),  m + .                 -> E_m = (1 - beta1)(E_g2 + 3u|d|) + u|m'|
      v' (4 operations):  a = v * beta2,  (1 - beta2) * g2,  . * g2 = b,  a + b
                                                                    -> E_v = 2u a + 3u b + 2(1 - beta2)|g2| E_g2 + u v'
      p' (6 operations):  s = sqrt(v'),  r = s / bcs,  denom = r + eps,  q = m' / denom,  step_size * q,  p - .
          E_s = E_v / (2 s) + u s;   E_denom = E_s / bcs + 2u r + u eps + u denom;   E_q = E_m / denom + |q| E_denom / denom + u|q|
          E_p = step_size E_q + 2u|step_size q| + u|p'|

    A fused multiply-add removes the rounding of the product it absorbs (in g2, m', v' and p'), so each sum above also bounds the
    contracted evaluation, whichever products the compiler fuses.  margin() adds what a first-order bound leaves out.
    ``u`` = 2^-53 gives the same bound for an evaluation in fp64 (the clamp is exact there): two such evaluations, fused or not,
    lie within twice that of each other."""
    with np.errstate(all="ignore"):
        t = _intermediates(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_clamp)
        e_g2 = np.zeros_like(t["p"])
        if grad_clamp is not None and u == U:
            e_g2 = e_g2 + np.where(np.abs(t["g"]) > grad_clamp, abs(grad_clamp - float(F32(grad_clamp))), 0.0)
        if weight_decay != 0:
            e_g2 = e_g2 + 2 * u * np.abs(weight_decay * t["p"]) + u * np.abs(t["g2"])
        d = t["g2"] - t["m"]
        e_m = (1.0 - beta1) * (e_g2 + 3 * u * np.abs(d)) + u * np.abs(t["m2"])
        e_v = 2 * u * t["a"] + 3 * u * t["b"] + 2 * (1.0 - beta2) * np.abs(t["g2"]) * e_g2 + u * t["v2"]
        e_s = np.where(t["s"] > 0, e_v / (2 * np.where(t["s"] > 0, t["s"], 1.0)), 0.0) + u * t["s"]
        e_den = e_s / t["bcs"] + 2 * u * t["r"] + u * eps + u * t["denom"]
        e_q = e_m / t["denom"] + np.abs(t["q"]) * e_den / t["denom"] + u * np.abs(t["q"])
        e_p = t["step_size"] * e_q + 2 * u * np.abs(t["upd"]) + u * np.abs(t["p2"])
    return e_p, e_m, e_v


def margin(b):
    """What a comparison against step_fp64 allows: twice the first-order bound (the second-order terms, and intermediates that lose
    bits as denormals or are flushed) plus one fp32 denormal absolute (an output that is itself flushed)."""
    return 2.0 * b + DENORM


def _fma(a, b, c):
    # the product of two fp32 values is exact in fp64; the sum is rounded to fp64 and then to fp32 (a double rounding that differs
    # from a true fma in about one case in 2^29: no matter for a bound)
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def emulate_fp32(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_clamp=None, contract=False, mutant=None):
    """``adam_kernel`` per element in numpy float32, in the kernel's order -> (p', m', v', g_written), float32.  ``contract`` fuses
    every multiply that feeds an add, as the device compiler may; ``mutant`` (one of MUTANTS) selects a deliberately wrong rule."""
    assert mutant is None or mutant in MUTANTS, mutant
    p, g, m, v = (np.asarray(x) for x in (p, g, m, v))
    assert all(x.dtype == F32 for x in (p, g, m, v))
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step          # in double on the host, each kernel argument rounded once
    if mutant == "no_bias_correction1":
        bc1 = 1.0
    if mutant == "no_bias_correction2":
        bc2 = 1.0
    w1 = F32(beta1 if mutant == "lerp_weight_beta1" else 1.0 - beta1)
    b2, w2, ss, bcs, eps32 = F32(beta2), F32(1.0 - beta2), F32(lr / bc1), F32(bc2 ** 0.5), F32(eps)
    wd = F32(0.0 if mutant == "weight_decay_dropped" else weight_decay)
    with np.errstate(all="ignore"):
        written = g
        if grad_clamp is not None:
            c = F32(grad_clamp)
            written = np.where(np.isnan(g), g, np.minimum(np.maximum(g, -c), c))
        gs = g if mutant == "clamp_written_only" else written
        if wd != 0:
            gs = _fma(wd, p, gs) if contract else gs + wd * p
        d = gs - m
        m2 = _fma(d, w1, m) if contract else m + d * w1
        t = w2 * gs
        v2 = _fma(v, b2, t * gs) if contract else v * b2 + t * gs
        if mutant == "eps_inside_sqrt":
            denom = np.sqrt(v2 + eps32) / bcs
        elif mutant == "eps_before_bias_correction2":
            denom = (np.sqrt(v2) + eps32) / bcs
        else:
            denom = np.sqrt(v2) / bcs + eps32
        q = (m if mutant == "quotient_from_old_m" else m2) / denom
        p2 = _fma(-ss, q, p) if contract else p - ss * q
    for x in (p2, m2, v2, written):
        assert x.dtype == F32
    return p2, m2, v2, written
