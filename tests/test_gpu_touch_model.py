"""GPU tests of the touch chart predictor (reconstruction/touch/model.py) against the fixture the real reference wrote
(``g17_touch_encoder.npz``): eval mode with the fused stem (csrc/conv5f.hip) and without, train mode on torch's modules, and
``policies.scoring.touch_slots``.

Caps: the reference's own fp32 result differs from the same module in fp64 by ``e_stem`` (block 3's output) / ``e_out`` (forward);
two equally valid fp32 evaluations with different summation orders get 4 x that.  Train-mode caps are 4 x the reference's own
fp32-versus-fp64 figure of each quantity, computed here from the stored pair.

Observed on an MI355X: fused stem 1.14 e_stem / 1.39 e_out, torch path 1.05 / 1.09, fused against torch 1.72 / 1.57; train-mode
predict_verts 3.4e-6 (cap 1.7e-5), gradients 0.2-0.5 of their caps; touch_slots against the per-sample forward 0.33 e_out."""
import pytest
import torch

import golden_util as gu
import touch_util as tu
from helpers import assert_grad_close, rel_err, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    return gu.load(tu.FIXTURE)


def inputs(z, dev):
    x = torch.from_numpy(z["img"]).float().to(dev) / 255.0
    ref = {"rot": torch.from_numpy(z["rot"]).to(dev), "pos": torch.from_numpy(z["pos"]).to(dev)}
    verts = torch.from_numpy(z["template"]).to(dev).unsqueeze(0).repeat(x.shape[0], 1, 1)
    return x, ref, verts


def eval_outputs(z, dev, fused):
    from a3vt_amd import ops
    net = tu.load_encoder(z, dev, fused_stem=fused)
    x, ref, verts = inputs(z, dev)
    before = ops.STATS.get("conv5f", 0)
    with torch.no_grad():
        stem = net.stem(x)
        out = net(x, ref, verts)
    launches = ops.STATS.get("conv5f", 0) - before
    assert launches == (18 if fused else 0), f"fused_stem={fused}: {launches} conv5f launches in two passes over the stem"
    assert tuple(stem.shape) == (2, 32, 16, 16)
    return stem.double().cpu(), out.double().cpu()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "torch"])
def test_eval_against_fp64(cuda, z, fused):
    stem, out = eval_outputs(z, cuda, fused)
    e_stem, e_out = float(z["e_stem"]), float(z["e_out"])
    d_stem = (stem - torch.from_numpy(z["eval64:stem"])).abs().max().item()
    d_out = (out - torch.from_numpy(z["eval64:out"])).abs().max().item()
    print(f"fused_stem={fused}: stem {d_stem:.3e} = {d_stem / e_stem:.2f} e_stem, forward {d_out:.3e} = {d_out / e_out:.2f} e_out")
    assert d_stem <= 4 * e_stem, f"block 3's output: {d_stem:.3e} > 4 x {e_stem:.3e}"
    assert d_out <= 4 * e_out, f"forward: {d_out:.3e} > 4 x {e_out:.3e}"


def test_fused_against_torch(cuda, z):
    stem_f, out_f = eval_outputs(z, cuda, True)
    stem_t, out_t = eval_outputs(z, cuda, False)
    d_stem, d_out = (stem_f - stem_t).abs().max().item(), (out_f - out_t).abs().max().item()
    print(f"fused vs torch: stem {d_stem / float(z['e_stem']):.2f} e_stem, forward {d_out / float(z['e_out']):.2f} e_out")
    assert d_stem <= 4 * float(z["e_stem"]) and d_out <= 4 * float(z["e_out"])


def test_fold_follows_the_parameters(cuda, z):
    """The cached BatchNorm fold and weight image are rebuilt when a tensor they were made from changes."""
    net = tu.load_encoder(z, cuda, fused_stem=True)
    x, _, _ = inputs(z, cuda)
    with torch.no_grad():
        a = net.stem(x).clone()
        assert torch.equal(net.stem(x), a)
        net.CNN_layers[1].double_conv[4].running_var.mul_(4.0)
        net.CNN_layers[2].double_conv[6].weight.mul_(-1.0)
        b = net.stem(x)
        net.fused_stem = False
        want = net.stem(x)
    assert not torch.equal(a, b)
    assert (b - want).abs().max().item() <= 4 * float(z["e_stem"]) * max(1.0, want.abs().max().item() / 6.0)


def test_train_mode_against_fp64(cuda, z):
    from a3vt_amd import ops
    net = tu.load_encoder(z, cuda, fused_stem=True).train()
    x, _, _ = inputs(z, cuda)
    before = ops.STATS.get("conv5f", 0)
    pred = net.predict_verts(x)
    (pred * torch.from_numpy(z["R"]).to(cuda)).sum().backward()
    assert ops.STATS.get("conv5f", 0) == before, "the forward-only kernels ran in train mode"
    p32, p64 = torch.from_numpy(z["train32:pred"]), torch.from_numpy(z["train64:pred"])
    cap = 4 * rel_err(p32, p64)
    print(f"train predict_verts: rel err {rel_err(pred, p64):.3e}, cap {cap:.3e}")
    assert rel_err(pred, p64) <= cap
    params = dict(net.named_parameters())
    for k in tu.GRAD_NAMES:
        g32, g64 = torch.from_numpy(z[f"train32:g:{k}"]), torch.from_numpy(z[f"train64:g:{k}"])
        tol, l2 = 4 * rel_err(g32, g64), 4 * rel_l2(g32, g64)
        print(f"grad {k}: rel err {rel_err(params[k].grad, g64):.3e} (cap {tol:.3e}), rel l2 {rel_l2(params[k].grad, g64):.3e} (cap {l2:.3e})")
        assert_grad_close(params[k].grad, g64, what=k, tol=tol, l2_tol=l2)


def test_fused_path_not_taken_when_it_must_not_be(cuda, z):
    from a3vt_amd import ops
    net = tu.load_encoder(z, cuda, fused_stem=True)
    x, _, _ = inputs(z, cuda)
    count = lambda: ops.STATS.get("conv5f", 0)      # noqa: E731
    n0 = count()
    net.eval()
    net.predict_verts(x)                            # eval mode, gradients enabled
    assert count() == n0
    net.train()
    with torch.no_grad():
        net.predict_verts(x)                        # train mode, gradients disabled
    assert count() == n0
    net.eval()
    with torch.no_grad():
        net.predict_verts(x)
    assert count() == n0 + 9
    net.fused_stem = False
    with torch.no_grad():
        net.predict_verts(x)
    assert count() == n0 + 9
    cpu = tu.load_encoder(z, "cpu", fused_stem=True)
    with torch.no_grad():
        cpu.predict_verts(x.cpu())
    assert count() == n0 + 9


def test_touch_slots(cuda, z):
    from a3vt_amd.pterotactyl.policies import scoring
    net = tu.load_encoder(z, cuda, fused_stem=True)
    lead = (2, 3, 4)                                # candidates x environments x fingers
    n = 24
    touch = (tu.images(n, 11).float() / 255.0).to(cuda).view(*lead, 3, 121, 121)
    rot, pos = tu.frames(n, 12)
    ref = {"rot": rot.to(cuda).view(*lead, 3, 3), "pos": pos.to(cuda).view(*lead, 3)}
    names = ["touch", "no_touch", "no_contact"]
    status = [[[names[(5 * k + 2 * e + f) % 3] for f in range(4)] for e in range(3)] for k in range(2)]
    template = torch.from_numpy(z["template"]).to(cuda)
    charts, masks = scoring.touch_slots(net, touch, ref, status, template)
    assert tuple(charts.shape) == lead + (25, 3) and tuple(masks.shape) == lead + (25, 1)
    # the forward over the same 24 samples: a "touch" slot holds ITS sample's row of it, bit for bit; and that row is the forward
    # of the sample alone up to fp32 summation order (blocks 4-6 and the linear layers run torch's kernels, which are picked by the
    # batch size: the cap is the one of two equally valid fp32 evaluations, 4 e_out)
    with torch.no_grad():
        whole = net(touch.reshape(n, 3, 121, 121), {"rot": ref["rot"].reshape(n, 3, 3), "pos": ref["pos"].reshape(n, 3)},
                    template[None].repeat(n, 1, 1)).view(*lead, 25, 3)
    cap, worst = 4 * float(z["e_out"]), 0.0
    seen = set()
    for k in range(2):
        for e in range(3):
            for f in range(4):
                st = status[k][e][f]
                seen.add(st)
                if st == "touch":
                    with torch.no_grad():
                        one = net(touch[k, e, f][None], {"rot": ref["rot"][k, e, f][None], "pos": ref["pos"][k, e, f][None]}, template[None])
                    assert torch.equal(charts[k, e, f], whole[k, e, f]), "the slot does not hold its own sample's prediction"
                    d = (charts[k, e, f] - one[0]).abs().max().item()
                    worst = max(worst, d)
                    assert d <= cap, f"a chart differs from its sample's own forward by {d:.3e} > 4 e_out = {cap:.3e}"
                    assert (masks[k, e, f] == 2).all()
                elif st == "no_touch":
                    assert torch.equal(charts[k, e, f], ref["pos"][k, e, f].view(1, 3).expand(25, 3))
                    assert (masks[k, e, f] == 1).all()
                else:
                    assert (charts[k, e, f] == 0).all() and (masks[k, e, f] == 0).all()
    assert seen == set(names)
    # a mix-up between samples cannot hide under the cap: any two samples' charts are apart by orders of magnitude more
    flat = whole.reshape(n, -1)
    apart = (flat[:, None] - flat[None]).abs().amax(dim=-1) + torch.eye(n, device=cuda)
    assert apart.min().item() > 1000 * cap, f"two samples' charts are only {apart.min().item():.3e} apart"
    print(f"touch_slots: batched against per-sample forward, worst {worst:.3e} = {worst / float(z['e_out']):.2f} e_out")
