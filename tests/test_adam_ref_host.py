"""CPU tests of tests/adam_ref.py, the yardstick test_gpu_adam.py judges the kernel by: the fp32 emulation of the rule, with and
without fused multiply-adds, stays inside 1 x the derived bound of the fp64 rule at every setting (the bound is safe); every wrong
rule in adam_ref.MUTANTS leaves 2 x the bound at some setting on a tenth of the elements or more (the bound has teeth); and the fp64
rule is torch's own, not this project's reading of it."""
import numpy as np
import pytest
import torch

import adam_ref as ar

N = 50000


def _case(si):
    setting = ar.SETTINGS[si]
    p, g, m, v = ar.make_inputs(np.random.default_rng(100 + si), N, setting)
    h = ar.hyper(setting)
    return (p, g, m, v), h, ar.step_fp64(p, g, m, v, **h)[:3], ar.bound(p, g, m, v, **h)


@pytest.fixture(scope="module")
def cases():
    return [_case(si) for si in range(len(ar.SETTINGS))]


@pytest.mark.parametrize("contract", [False, True])
@pytest.mark.parametrize("si", range(len(ar.SETTINGS)))
def test_fp32_emulation_stays_inside_the_bound(cases, si, contract):
    state, h, want, bnd = cases[si]
    got = ar.emulate_fp32(*state, **h, contract=contract)
    for name, x, w, b in zip(("p", "m", "v"), got, want, bnd):
        assert np.isfinite(b).all() and (b >= 0).all()
        err = np.abs(x.astype(np.float64) - w)
        ratio = np.where(err > 0, err / np.where(b > 0, b, 1.0), 0.0)
        assert (err <= b).all(), f"{ar.SETTINGS[si]['name']} {name}': error / bound up to {ratio.max():.3f} at element {int(ratio.argmax())}"
    clamped = ar.step_fp64(*state, **h)[3]
    assert np.array_equal(got[3].astype(np.float64), clamped)          # the written gradient is exact


def _violating_share(state, h, want, bnd, mutant, contract):
    got = ar.emulate_fp32(*state, **h, contract=contract, mutant=mutant)
    return [float((np.abs(x.astype(np.float64) - w) > ar.margin(b)).mean()) for x, w, b in zip(got, want, bnd)]


@pytest.mark.parametrize("mutant", ar.MUTANTS)
def test_every_wrong_rule_leaves_the_margin_somewhere(cases, mutant):
    shares = {}
    for si, (state, h, want, bnd) in enumerate(cases):
        # the weaker of the two contraction variants, per output: the mutant has to show whichever way the compiler fuses
        both = [_violating_share(state, h, want, bnd, mutant, c) for c in (False, True)]
        shares[ar.SETTINGS[si]["name"]] = [min(a, b) for a, b in zip(*both)]
    print(mutant, {k: [round(x, 3) for x in s] for k, s in shares.items()})
    for out in ar.MUTANT_OUTPUTS[mutant]:
        assert max(s[out] for s in shares.values()) >= 0.10, (mutant, ("p", "m", "v")[out], shares)


def test_bias_correction_mutants_cannot_show_at_step_100000(cases):
    """Both corrections are exactly 1 there (beta^t underflows): the small step counts carry those two mutants."""
    state, h, want, bnd = cases[3]
    for mutant in ("no_bias_correction1", "no_bias_correction2"):
        assert _violating_share(state, h, want, bnd, mutant, False) == [0.0, 0.0, 0.0]


def test_inputs_reach_below_eps_and_beyond_the_clamp(cases):
    """What the eps mutants and the clamp mutant need from the inputs."""
    (p, g, m, v), h, want, _ = cases[2]
    share = float((np.sqrt(want[2]) <= h["eps"]).mean())
    assert h["eps"] == 1e-3 and share > 0.05, share
    (p, g, m, v), h, _, _ = cases[4]
    assert 0.28 < float((np.abs(g) > h["grad_clamp"]).mean()) < 0.38


def test_the_clamp_follows_torch_clamp():
    g = np.array([np.nan, np.inf, -np.inf, 2.0, -2.0, 0.25, -0.0], np.float32)
    z = np.zeros_like(g)
    got = ar.step_fp64(z, g, z, z, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, grad_clamp=1.0)[3]
    want = torch.clamp(torch.from_numpy(g), -1.0, 1.0).numpy()
    assert np.array_equal(got, want.astype(np.float64), equal_nan=True) and np.isnan(got[0]) and np.signbit(got[6])
    written = ar.emulate_fp32(z, g, z, z, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, grad_clamp=1.0)[3]
    assert np.array_equal(written, want, equal_nan=True)


@pytest.mark.parametrize("si", range(len(ar.SETTINGS)))
def test_step_fp64_is_torch_adam_in_float64(si):
    """Against ``torch.optim.Adam(foreach=False)`` on CPU float64 tensors.  torch's CPU kernels fuse the multiply-adds of
    ``add(alpha=)``, ``lerp_`` and ``addcmul_`` (measured: g2, m' and v' are the fused evaluations to the last bit) and numpy does
    not, so the two fp64 evaluations differ by an fp64 rounding of an operand.  Where g + wd * p, g2 - m or p - update cancels, that
    rounding is tiny against what was subtracted and large against the result: relative to the result the largest differences over
    these inputs are 2.3e-13 for p', 8.9e-15 for m' and 1.8e-14 for v', and 1e-14 holds for all but a handful of the 4000 elements
    (asserted: 99.5 %).  Every element is held to what two fp64 evaluations of the rule can differ by: twice adam_ref.bound at
    u = 2^-53, which is below 1e-14 of the result wherever nothing cancels."""
    setting = ar.SETTINGS[si]
    h = ar.hyper(setting)
    p, g, m, v = ar.make_inputs(np.random.default_rng(200 + si), 4000, setting)
    want = ar.step_fp64(p, g, m, v, **h)
    tp = torch.nn.Parameter(torch.from_numpy(p).double())
    tp.grad = torch.from_numpy(g).double()
    if h["grad_clamp"] is not None:
        tp.grad.clamp_(-h["grad_clamp"], h["grad_clamp"])
    opt = torch.optim.Adam([tp], lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], weight_decay=h["weight_decay"], foreach=False)
    opt.state[tp] = {"step": torch.tensor(float(h["step"] - 1)), "exp_avg": torch.from_numpy(m).double(),
                     "exp_avg_sq": torch.from_numpy(v).double()}
    opt.step()
    assert float(opt.state[tp]["step"]) == h["step"]
    got = (tp.detach().numpy(), opt.state[tp]["exp_avg"].numpy(), opt.state[tp]["exp_avg_sq"].numpy(), tp.grad.numpy())
    assert np.array_equal(got[3], want[3])
    bnd = ar.bound(p, g, m, v, **h, u=2.0 ** -53)
    for name, x, w, b in zip(("p", "m", "v"), got, want, bnd):
        err = np.abs(x - w)
        rel = err / np.abs(w)
        print(f"{setting['name']} {name}': vs torch fp64, error / fp64 bound {(err / b).max():.2f}, relative to the result {rel.max():.1e}, "
              f"{int((rel > 1e-14).sum())} of {rel.size} elements above 1e-14")
        assert (err <= 2 * b).all(), (setting["name"], name, float((err / b).max()))
        assert float((rel <= 1e-14).mean()) >= 0.995 and float(np.median(b / np.abs(w))) < 1e-15, (setting["name"], name)
