"""CPU tests of tests/posenc_ref.py, the float64 reference the encoder edge tests (test_gpu_posenc_edges.py) compare against:
it agrees with the float64 oracle up to the argument rounding it models, its hand-written backward agrees with autograd, its
token rule and near-kink marking do what they say, and the float32-CPU-versus-reference errors from which the GPU bounds are
taken are measured, printed (run with -s) and asserted to stay below the figures posenc_ref.CPU_FIGURES records."""
import pytest
import torch

import posenc_ref as R
from helpers import rel_err

# (I, m, |p| max): the shapes the GPU file's bounds are taken from
MEASURE = [(50, 1551, 0.3), (50, 1551, 1.5), (50, 65557, 0.3), (50, 65557, 1.5),
           (16, 300, 1.5), (24, 300, 1.5), (496, 300, 1.5), (496, 300, 0.3)]


def _oracle(case):
    from oracle import gcn as og
    I = case["I"]
    st = {k: t.double().requires_grad_(True) for k, t in zip(R.NAMES, case["params"])}
    v = case["verts"].double().requires_grad_(True)
    f = og.positional_encoder(v, st) + og.mask_encoder(case["mask"], st)
    (f * case["gout"][..., :I].double()).sum().backward()
    return f.detach().reshape(-1, I), v.grad.reshape(-1, 3), [st[k].grad for k in R.NAMES]


# Measured here at |p| <= 0.3, m = 1551 (seed 1): features 3.7e-8 / 3.9e-8 / 2.8e-8 of the largest feature at I = 50 / 16 / 448
# (1.7e-7 / 2.3e-7 / 1.2e-7 at |p| <= 1.5), gradients up to 5.1e-7 (grad_verts at 448; dW1, which sees the argument rounding
# directly, 3.9e-7); the bias and embedding gradients, which do not depend on the argument, agree exactly.  x 16:
ORACLE_FEATS, ORACLE_GRADS = 16 * 3.9e-8, 16 * 5.1e-7


@pytest.mark.parametrize("I", [50, 16, 448])
def test_reference_agrees_with_the_float64_oracle_up_to_the_argument_rounding(I):
    case = R.make_case(1, 1551, I, seed=1, pmax=0.3)
    f, gv, gp = _oracle(case)
    ref = case["ref"]
    errs = {"feats": rel_err(ref["feats"], f), "grad_verts": rel_err(ref["grad_verts"], gv)}
    errs.update({n: rel_err(a, b) for n, a, b in zip(R.SHORT, ref["grad_params"], gp)})
    print(f"\nI={I} reference vs oracle.gcn (|p| <= 0.3): " + "  ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    assert 0 < errs["feats"] < ORACLE_FEATS          # (0 would mean the rounding is not modelled at all)
    assert max(v for k, v in errs.items() if k != "feats") < ORACLE_GRADS
    # at |p| <= 1.5 the arguments are five times larger and so is the distance (printed)
    far = R.make_case(1, 1551, I, seed=4, pmax=1.5)
    print(f"I={I} |p| <= 1.5: feats {rel_err(far['ref']['feats'], _oracle(far)[0]):.1e}")


@pytest.mark.parametrize("I,m", [(50, 300), (16, 37), (496, 40)])
def test_hand_backward_agrees_with_autograd_through_the_surrogate_argument(I, m):
    case = R.make_case(1, m, I, seed=4, pmax=1.5)
    ref = case["ref"]
    ag = R.evaluate_autograd(case["verts"], case["mask"], case["params"], case["gout"][..., :I])
    assert rel_err(ref["feats"], ag["feats"]) < 1e-14
    assert rel_err(ref["grad_verts"], ag["grad_verts"]) < 1e-13
    for n, a, b in zip(R.SHORT, ref["grad_params"], ag["grad_params"]):
        assert a.shape == b.shape and rel_err(a, b) < 1e-13, n


def test_argument_is_the_float32_product_of_the_float32_frequency():
    import numpy as np
    assert R.FREQ32.dtype == np.float32 and R.FREQ32[0] == np.float32(np.pi) and R.FREQ32[9] == np.float32(np.pi * 18)
    p = torch.tensor([[0.3, -1.5, 0.123456789]])
    e, s, c = R.embed(p, torch.float64)
    for i in range(10):
        for ax in range(3):
            arg = float(np.float32(R.FREQ32[i] * np.float32(p[0, ax].item())))      # one float32 rounding of the product
            assert e[0, 6 * i + ax].item() == pytest.approx(np.sin(arg), abs=1e-15)
            assert e[0, 6 * i + 3 + ax].item() == pytest.approx(np.cos(arg), abs=1e-15)
    assert torch.equal(e[0, 60:], p[0].double())
    # and it is NOT the float64 product: at 18 pi x 1.5 they differ by up to an ulp of 85 (7.6e-6)
    assert abs(float(np.float32(R.FREQ32[9] * np.float32(-1.5))) - np.pi * 18 * -1.5) > 1e-7


def test_tokens_truncate_and_clamp():
    mask = torch.tensor(R.HAND_MASK)
    assert R.tokens(mask).tolist() == [0, 0, 0, 0, 1, 2, 3, 3, 3, 3]
    legal = torch.tensor([0.0, 1.0, 2.0, 3.0, 0.5, 1.999])
    assert torch.equal(R.tokens(legal), legal.long())             # mask.long() for legal masks
    # the token picks the embedding row, in the features and in the gradient
    case = R.make_case(1, 10, 50, seed=1, mask=mask)
    emb = case["params"][6].double()
    base = R.evaluate(case["verts"], torch.zeros(10), case["params"])["feats"] - emb[0]
    assert torch.allclose(case["ref"]["feats"] - base, emb[R.tokens(mask)], atol=1e-14)
    g = case["gout"].reshape(10, 50).double()
    for t, rows in ((0, [0, 1, 2, 3]), (1, [4]), (2, [5]), (3, [6, 7, 8, 9])):
        assert torch.allclose(case["ref"]["grad_params"][6][t], g[rows].sum(0), atol=1e-14)


def test_near_kink_marks_an_exact_zero_and_the_builder_zeroes_its_row():
    pre1 = torch.tensor([[0.5, -0.5], [0.5, 0.0], [2e-6, -2e-6], [0.5, 0.5], [0.5, 0.5]], dtype=torch.float64)
    pre2 = torch.tensor([[1.0], [1.0], [1.0], [-9e-7], [1e-6]], dtype=torch.float64)
    assert R.near_kink(pre1, pre2, 1e-6).tolist() == [False, True, False, True, False]
    # constructed case: a zero first layer makes every first-layer pre-activation exactly 0 -> every vertex is marked; the
    # builder refuses (cap), and with the cap lifted zeroes every row
    params = R.make_params(50, 3)
    params[0].zero_()
    params[1].zero_()
    with pytest.raises(AssertionError, match="ReLU kink"):
        R.make_case(1, 40, 50, seed=1, params=params)
    # one vertex steered onto a kink: b1[0] := -(W1[0] . e(v_7)) makes unit 0 of vertex 7 vanish to rounding
    case = R.make_case(1, 2000, 50, seed=1)
    assert not case["kink"][7]
    params = [t.clone() for t in case["params"]]
    e, _, _ = R.embed(case["verts"].reshape(-1, 3), torch.float64)
    params[1][0] = -(e[7] @ params[0][0].double()).float()
    steered = R.make_case(1, 2000, 50, seed=1, params=params)
    assert steered["kink"][7] and abs(steered["ref"]["pre1"][7, 0].item()) < 1e-6
    assert steered["gout"].reshape(2000, 50)[7].abs().max() == 0 and steered["kink_share"] <= R.MAX_KINK_SHARE
    assert steered["ref"]["grad_verts"][7].abs().max() == 0          # a zeroed row contributes nothing


def test_float32_cpu_errors_stay_below_the_figures_the_gpu_bounds_cite():
    """The yardstick: the same formula in float32 on the CPU against the reference, every tensor on its own scale.  The GPU
    bounds are 16 x posenc_ref.CPU_FIGURES; this test keeps those figures honest (measured <= figure) and prints them."""
    worst = {k: 0.0 for k in R.CPU_FIGURES}
    worst_pre = 0.0
    print()
    for I, m, pmax in MEASURE:
        case = R.make_case(1, m, I, seed=1, pmax=pmax)
        ref = case["ref"]
        f32 = R.evaluate(case["verts"], case["mask"], case["params"], case["gout"][..., :I], dtype=torch.float32)
        pre = max((f32["pre1"].double() - ref["pre1"]).abs().max().item(), (f32["pre2"].double() - ref["pre2"]).abs().max().item())
        errs = {"feats": rel_err(f32["feats"], ref["feats"]), "grad_verts": rel_err(f32["grad_verts"], ref["grad_verts"])}
        per = {n: rel_err(a, b) for n, a, b in zip(R.SHORT, f32["grad_params"], ref["grad_params"])}
        size = "" if m <= 2048 else "_large"
        errs["weights" + size] = max(v for n, v in per.items() if n != "dEmb")
        errs["emb" + size] = per["dEmb"]
        print(f"I={I:3d} m={m:5d} |p|<={pmax}: kink share {case['kink_share']:.1e}  |pre32 - pre64| {pre:.1e}  feats {errs['feats']:.1e}"
              f"  grad_verts {errs['grad_verts']:.1e}  " + "  ".join(f"{n} {v:.1e}" for n, v in per.items()))
        worst_pre = max(worst_pre, pre)
        for k, v in errs.items():
            worst[k] = max(worst[k], v)
    print("worst float32-CPU figures:", {k: f"{v:.2e}" for k, v in worst.items()}, f"pre-activations {worst_pre:.1e}")
    print("figures the bounds cite:  ", {k: f"{v:.1e}" for k, v in R.CPU_FIGURES.items()}, f"TAU {R.TAU:.1e}")
    for k, v in worst.items():
        assert 0.25 * R.CPU_FIGURES[k] < v <= R.CPU_FIGURES[k], (k, v)      # neither exceeded nor padded
        assert R.BOUNDS[k] == 16 * R.CPU_FIGURES[k]
    assert worst_pre < R.TAU


def test_pack_and_unpack_follow_the_state_dict_order():
    params = R.make_params(50, 0)
    vec = R.pack(params)
    assert vec.numel() == 12 * 63 + 12 + 25 * 12 + 25 + 50 * 25 + 50 + 200
    assert all(torch.equal(a, b) for a, b in zip(R.unpack(vec, 50), params))
    assert [tuple(t.shape) for t in params] == R.param_shapes(50)
