"""-m gpu: the DDQN learner on the device (ISSUE: fused Q-network input layer + TD kernel + clamp inside the optimizer launch).

* ``a3vt_ddqn_td`` against the reference's update rule written out in torch fp64 here;
* ``ops.qnet_input`` (features + layer 0 of ``Graph_Model`` without the feature rows) against the unfused model with the same
  weights, against an fp64 restatement of the formulas (``ddqn_util.layer0_restated``), and through ``g10_graph_model.npz``
  against the reference; its launch counter, repeatability, batch invariance and allocator peak;
* cases (a) and (b) of ``g16_ddqn_update.npz`` (reference runs of one ``update_parameters``) end to end, knob on and off;
* ``get_action`` and the device-resident replay memory.

The upstream gradient of the fp64 comparison is plain ``randn``: ``test_ddqn_host.py`` checks on the CPU that the unfused fp32
formulation stays inside ``assert_grad_close``'s caps against fp64 under it."""
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ddqn_util as du
from golden_util import load, state_sha256
from helpers import assert_grad_close, make_args, rel_err

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


# ---- the TD kernel -----------------------------------------------------------------------------------------------------------------
def _td_ref(q_cur, q_no, q_nt, mask, actions, rewards, denom, budget, gamma):
    """ddqn.py:88-115 in fp64 (the Python loop over the batch written as a where)."""
    q_cur, q_no, q_nt, mask, rewards = (t.double() for t in (q_cur, q_no, q_nt, mask, rewards))
    not_done = mask.sum(dim=1) < budget - 1
    if denom is not None:
        rewards = rewards / denom.double()
    q = q_cur.gather(1, actions.long()[:, None]).squeeze(1)
    pen = q_no.clone()
    pen[mask > 0] = -1e10
    best = (pen == pen.max(dim=1, keepdim=True)[0]).float().argmax(dim=1)        # the lowest index of the maximum
    nxt = torch.where(not_done, q_nt.gather(1, best[:, None]).squeeze(1), torch.zeros_like(q))
    target = gamma * nxt + rewards
    return ((q - target) ** 2).mean(), best, target, q - target


def _td_inputs(B, A, rows, seed):
    g = torch.Generator().manual_seed(seed)
    q_cur, q_no, q_nt = (torch.randn(B, A, generator=g) for _ in range(3))
    budget = 5
    touched = {"done": torch.full((B,), 4), "open": torch.randint(0, 4, (B,), generator=g),
               "mixed": torch.randint(0, 6, (B,), generator=g)}[rows]
    if rows == "mixed":
        touched[0], touched[1] = 4, 1
    mask = torch.zeros(B, A)
    for b in range(B):
        mask[b, torch.randperm(A, generator=g)[:int(touched[b])]] = 1
    # row 0: a tie between two free columns (the lower index must win); row 1: the unpenalised maximum sits on a penalised column
    free = torch.nonzero(mask[0] == 0).flatten()
    q_no[0, free[1]] = q_no[0, free[-1]] = 7.0
    if mask[1].sum() == 0:
        mask[1, A // 2] = 1
    q_no[1, torch.nonzero(mask[1] > 0).flatten()[0]] = 9.0
    actions = torch.randint(0, A, (B,), generator=g).float()
    rewards = torch.rand(B, generator=g)
    first = 1.0 + torch.rand(B, generator=g)
    score = first * (0.5 + 0.5 * torch.rand(B, generator=g))
    return q_cur, q_no, q_nt, mask, actions, rewards, first, score, budget, int(free[1])


@pytest.mark.parametrize("A", [7, 50])
@pytest.mark.parametrize("B", [2, 16, 67, 300])
def test_td_kernel_against_the_rule_in_fp64(cuda, B, A):
    from a3vt_amd import ops
    for rows in ("done", "open", "mixed"):
        q_cur, q_no, q_nt, mask, actions, rewards, first, score, budget, tie = _td_inputs(B, A, rows, 100 * B + A)
        dev = [t.to(cuda) for t in (q_cur, q_no, q_nt, mask, actions, rewards)]
        for gamma in (0.0, 0.9):
            for norm, denom in (("none", None), ("first", first), ("current", score)):
                qc = dev[0].clone().requires_grad_(True)
                loss, best, target = ops.ddqn_td(qc, *dev[1:], None if denom is None else denom.to(cuda), budget, gamma)
                r_loss, r_best, r_target, r_diff = _td_ref(q_cur, q_no, q_nt, mask, actions, rewards, denom, budget, gamma)
                what = f"B={B} A={A} rows={rows} gamma={gamma} norm={norm}"
                assert best.dtype == torch.int32 and torch.equal(best.cpu().long(), r_best), what
                assert int(best[0]) == tie and mask[1, int(best[1])] == 0, what
                assert rel_err(target, r_target) < 4 * EPS, what
                err = abs(loss.item() - r_loss.item()) / r_loss.item()
                (3.0 * loss).backward()
                want = torch.zeros(B, A, dtype=torch.float64)
                want[torch.arange(B), actions.long()] = 3.0 * 2.0 * r_diff / B
                dq = qc.grad.double().cpu()
                dq_err = ((dq - want).abs().max() / want.abs().max()).item()
                print(f"\n{what}: loss rel {err:.2e} (bound {(B + 8) * EPS:.2e})  dq {dq_err:.2e}")
                assert err <= (B + 8) * EPS, what
                assert dq_err <= 8 * EPS, what
                off = torch.ones(B, A, dtype=torch.bool)
                off[torch.arange(B), actions.long()] = False
                assert (dq[off] == 0).all(), what
                if rows == "done":
                    assert rel_err(target, (rewards / denom if denom is not None else rewards)) < 4 * EPS, what
                again = ops.ddqn_td(dev[0], *dev[1:], None if denom is None else denom.to(cuda), budget, gamma)
                assert torch.equal(again[0], loss.detach()) and torch.equal(again[1], best) and torch.equal(again[2], target), what


def test_td_kernel_refuses_what_it_does_not_cover(cuda):
    from a3vt_amd import ops
    z = lambda *s: torch.zeros(*s, device=cuda)  # noqa: E731
    with pytest.raises(RuntimeError):
        ops.ddqn_td(z(2, 305), z(2, 305), z(2, 305), z(2, 305), z(2), z(2), None, 5, 0.9)
    with pytest.raises(RuntimeError):
        ops.ddqn_td(z(2, 50), z(2, 50), z(2, 50), z(2, 49), z(2), z(2), None, 5, 0.9)


# ---- the fused input layer ---------------------------------------------------------------------------------------------------------
def _tp_info():
    from a3vt_amd.pterotactyl.utility import utils
    return utils.load_mesh_vision(make_args(use_touch=True, num_grasps=5, finger=True), "vision_charts")[0]


def _ico_info(cuda):
    from a3vt_amd import mesh as amesh
    from a3vt_amd.pterotactyl.utility import utils
    _, faces = amesh.icosphere(1)
    return {"adj": utils.normalize_adj(utils.calc_adj(torch.from_numpy(faces))).to(cuda)}


def _pair(info, cuda, seed=0, **kw):
    """Two graph models with the same weights: knob on / knob off."""
    from a3vt_amd.pterotactyl.policies.DDQN import model as dm
    nets = []
    for fused in (True, False):
        torch.manual_seed(seed)
        nets.append(dm.Graph_Model(du.case_args("a", fused_q_input=fused, **kw), info).to(cuda))
    assert all(torch.equal(a, b) for a, b in zip(nets[0].state_dict().values(), nets[1].state_dict().values()))
    return nets


SHAPES = [("t_p", 3, 200, 3), ("t_p", 2, 100, 3), ("t_p", 2, 300, 3), ("ico", 1, 200, 3), ("ico", 5, 200, 2), ("t_p", 2, 200, 1), ("ico", 5, 200, 1)]


@pytest.mark.parametrize("graph,B,hidden,layers", SHAPES)
def test_fused_input_layer_against_the_unfused_model(cuda, graph, B, hidden, layers):
    """Same weights, knob on vs off: Q values, every parameter gradient, and which path ran (launch counters).  t_p has hub rows;
    B = 3 gives 5847 rows (a multiple of no tile size); hidden 200 cuts at 66 columns (not a multiple of 4); hidden 300 takes the
    wide instantiation; ``layers = 1`` aggregates all 50 output columns (50 is no multiple of 4)."""
    from a3vt_amd import ops
    info = _tp_info() if graph == "t_p" else _ico_info(cuda)
    n = 1949 if graph == "t_p" else 42
    fused, plain = _pair(info, cuda, hidden_dim=hidden, layers=layers)
    obs = du.random_obs(B, n, 11, empty_sample=B - 1)
    assert sorted(obs["mesh"][..., 3].unique().tolist()) == [0.0, 1.0, 2.0, 3.0]
    gq = torch.randn(B, 50, generator=torch.Generator().manual_seed(2)).to(cuda)
    ops.path_counts(reset=True)
    q_plain = plain(obs)
    (q_plain * gq).sum().backward()
    counts = ops.path_counts(reset=True)
    assert counts["qnet_input_fwd"] == 0 and counts["qnet_input_bwd"] == 0
    q_fused = fused(obs)
    (q_fused * gq).sum().backward()
    counts = ops.path_counts()
    assert counts["qnet_input_fwd"] == 1 and counts["qnet_input_bwd"] == 1
    print(f"\n{graph} B={B} h={hidden} L={layers}: Q rel_err {rel_err(q_fused, q_plain):.3e}")
    assert rel_err(q_fused, q_plain) < 1e-4
    for (k, a), b in zip(fused.named_parameters(), plain.parameters()):
        assert a.grad is not None and b.grad is not None, k
        assert_grad_close(a.grad, b.grad, k)
    with torch.no_grad():                       # forward only (get_action): the same values, no backward scratch needed
        assert torch.equal(fused(obs), q_fused.detach())
    moved = {"mesh": obs["mesh"].to(cuda).requires_grad_(True), "mask": obs["mask"]}
    ops.path_counts(reset=True)
    fused(moved)                                # observations that want a gradient take the unfused path
    assert ops.path_counts()["qnet_input_fwd"] == 0


@pytest.mark.parametrize("graph,B,hidden,cut_all", [("t_p", 3, 200, False), ("t_p", 2, 300, False), ("ico", 5, 100, False), ("ico", 5, 50, True)])
def test_fused_input_layer_against_fp64(cuda, graph, B, hidden, cut_all):
    """Layer 0 alone against ``ddqn_util.layer0_restated`` in fp64: the fused output's error may be at most twice the unfused torch +
    library path's (both measured here, floor 1e-6 relative: the composites are rounded once more); every gradient the kernel or its
    composites produce through ``assert_grad_close`` under a random upstream gradient."""
    from a3vt_amd import ops
    from a3vt_amd.pterotactyl.reconstruction.vision.model import _csr_of
    if graph == "t_p":
        info, adj, n = _tp_info(), du.tp_dense_adjacency(), 1949
    else:
        info, n = _ico_info(cuda), 42
        adj = info["adj"].cpu()
    layers = 1 if cut_all else 3
    fused, plain = _pair(info, cuda, seed=3, hidden_dim=hidden, layers=layers, num_actions=hidden if cut_all else 50)
    obs = du.random_obs(B, n, 13, empty_sample=0)
    mesh = obs["mesh"].to(cuda)
    cut = hidden if cut_all else round(hidden * 0.33)
    gy = du.random_gy((B, n, hidden))
    action0 = plain.action_model(obs["mask"].to(cuda)).detach()
    y64, g64 = du.layer0_run({k: t.cpu() for k, t in du.layer0_params(plain).items()}, obs["mesh"], action0.cpu(), adj, cut, gy, torch.float64)
    csr = _csr_of(info, "adj")

    def run(net, is_fused):
        net.zero_grad(set_to_none=True)
        action = action0.clone().requires_grad_(True)
        if is_fused:
            y = ops.qnet_input(mesh, action, net.positional_embedding, net.mask_embedding.model[0].weight, net.layers[0].weight[0],
                               net.layers[0].bias, csr, cut)
        else:
            feats = torch.cat((action.unsqueeze(1).expand(-1, n, -1), net.positional_embedding(mesh[..., :3]),
                               net.mask_embedding(mesh[..., 3:])), dim=-1)
            y = net.layers[0](feats, csr, F.relu)
        y.backward(gy.float().to(cuda))
        return y.detach(), {**{k: t.grad for k, t in du.layer0_params(net).items()}, "action": action.grad}

    y_f, g_f = run(fused, True)
    y_u, g_u = run(plain, False)
    e_f, e_u = rel_err(y_f, y64), rel_err(y_u, y64)
    print(f"\n{graph} B={B} h={hidden} cut={cut}: output error vs fp64: fused {e_f:.3e}  unfused {e_u:.3e}")
    assert e_f <= max(2.0 * e_u, 1e-6)
    for k in g64:
        a, b = g_f[k].double().cpu().reshape(g64[k].shape), g64[k]
        print(f"  {k}: fused max {((a - b).abs().max() / b.abs().max()).item():.3e} l2 {((a - b).norm() / b.norm()).item():.3e}"
              f"   unfused l2 {((g_u[k].double().cpu().reshape(b.shape) - b).norm() / b.norm()).item():.3e}")
    for k in g64:
        assert_grad_close(g_f[k].reshape(g64[k].shape), g64[k], k)


def test_g10_ddqn_graph_model_fused(cuda):
    """``test_g10_ddqn_graph_model`` with ``fused_q_input=True``: the fused path against the reference's Graph_Model."""
    from a3vt_amd import ops
    from a3vt_amd.pterotactyl.policies.DDQN import model as dm
    z = load("g10_graph_model.npz")
    args = make_args(use_touch=True, num_grasps=5, finger=True, layers=3, hidden_dim=200, num_actions=50, fused_q_input=True)
    torch.manual_seed(0)
    net = dm.Graph_Model(args, _tp_info())
    assert np.array_equal(state_sha256(net.state_dict()), z["weight_sha256"]), "init differs from the reference"
    net = net.to(cuda)
    obs = {"mesh": torch.from_numpy(z["mesh"]), "mask": torch.from_numpy(z["mask"])}
    ops.path_counts(reset=True)
    q = net(obs)
    assert q.shape == (3, 50)
    assert rel_err(q, torch.from_numpy(z["q"])) < 1e-4
    (q * torch.from_numpy(z["gq"]).to(cuda)).sum().backward()
    counts = ops.path_counts()
    assert counts["qnet_input_fwd"] == 1 and counts["qnet_input_bwd"] == 1
    params = dict(net.named_parameters())
    for key in [k for k in z.files if k.startswith("g:")]:
        gk = params[key[2:]].grad
        got = gk[..., ::3, ::5] if key == "g:layers.0.weight" else gk
        assert_grad_close(got, torch.from_numpy(z[key]), key)


def _qnet_call(net, csr, mesh, action, gy):
    from a3vt_amd import ops
    net.zero_grad(set_to_none=True)
    action = action.clone().requires_grad_(True)
    y = ops.qnet_input(mesh, action, net.positional_embedding, net.mask_embedding.model[0].weight, net.layers[0].weight[0], net.layers[0].bias,
                       csr, 66)
    y.backward(gy)
    return [y.detach().clone(), action.grad.clone()] + [t.grad.clone() for t in du.layer0_params(net).values()]


def test_fused_input_layer_repeatable_and_batch_invariant(cuda):
    from a3vt_amd.pterotactyl.reconstruction.vision.model import _csr_of
    info = _tp_info()
    fused, _ = _pair(info, cuda, seed=5)
    csr = _csr_of(info, "adj")
    obs = du.random_obs(4, 1949, 17, empty_sample=2)
    mesh = obs["mesh"].to(cuda)
    action = fused.action_model(obs["mask"].to(cuda)).detach()
    gy = du.random_gy((4, 1949, 200)).float().to(cuda)
    first, second = _qnet_call(fused, csr, mesh, action, gy), _qnet_call(fused, csr, mesh, action, gy)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    alone = _qnet_call(fused, csr, mesh[2:3].contiguous(), action[2:3], gy[2:3].contiguous())     # the same S row: action[2]
    assert torch.equal(alone[0][0], first[0][2])


def test_fused_input_layer_relu_keeps_nan(cuda):
    """The kernel's own ReLUs (the encoder's two and the one on the passed-through columns) keep a NaN, as ``torch.relu`` in the
    unfused composition (``layer0_restated`` in fp32): a NaN position makes its row NaN, a NaN action embedding its whole sample, and
    the other samples keep the bits of the clean run.  Compared on the columns from ``cut`` on: the aggregated columns leave through
    the GCN stack's aggregation epilogue, which maps NaN to 0 by its documented choice."""
    from a3vt_amd import ops
    from a3vt_amd.pterotactyl.reconstruction.vision.model import _csr_of
    info, n, B, hidden, cut = _ico_info(cuda), 42, 5, 100, 33
    fused, plain = _pair(info, cuda, seed=3, hidden_dim=hidden, layers=3)
    obs = du.random_obs(B, n, 13, empty_sample=0)
    action = plain.action_model(obs["mask"].to(cuda)).detach()
    csr, adj = _csr_of(info, "adj"), info["adj"].cpu()
    params = {k: t.detach().cpu() for k, t in du.layer0_params(plain).items()}

    def run(mesh, act):
        with torch.no_grad():
            y = ops.qnet_input(mesh.to(cuda), act, fused.positional_embedding, fused.mask_embedding.model[0].weight,
                               fused.layers[0].weight[0], fused.layers[0].bias, csr, cut)
            return y, du.layer0_restated(params, mesh, act.cpu(), adj, cut)

    clean, clean_t = run(obs["mesh"], action)
    assert torch.isfinite(clean).all() and torch.isfinite(clean_t).all()
    others = [0, 1, 3, 4]
    mesh = obs["mesh"].clone()
    mesh[2, 7, 1] = float("nan")
    y, y_t = run(mesh, action)
    want = torch.isnan(y_t[..., cut:])
    assert want[2, 7].all() and want.sum() == hidden - cut
    assert torch.equal(torch.isnan(y[..., cut:]).cpu(), want)
    assert torch.equal(y[others], clean[others])
    assert torch.equal(y[2, :, cut:][~want[2].to(cuda)], clean[2, :, cut:][~want[2].to(cuda)])
    act = action.clone()
    act[2, 0] = float("nan")
    y, y_t = run(obs["mesh"], act)
    want = torch.isnan(y_t[..., cut:])
    assert want[2].all() and not want[others].any()
    assert torch.equal(torch.isnan(y[..., cut:]).cpu(), want)
    assert torch.equal(y[others], clean[others])


def test_fused_input_layer_allocator_peak(cuda):
    """No (B N) x 300 feature rows and none of the encoder's intermediates: over layer 0's forward + backward at B = 16 on t_p the
    allocator's peak grows by at most half of what the unfused path needs (both measured here, workspaces warmed up first)."""
    from a3vt_amd import ops
    from a3vt_amd.pterotactyl.reconstruction.vision.model import _csr_of
    info = _tp_info()
    fused, plain = _pair(info, cuda, seed=6)
    csr = _csr_of(info, "adj")
    obs = du.random_obs(16, 1949, 19)
    mesh = obs["mesh"].to(cuda)
    action0 = fused.action_model(obs["mask"].to(cuda)).detach()
    gy = torch.ones(16, 1949, 200, device=cuda)

    def step(net, is_fused):
        net.zero_grad(set_to_none=True)
        action = action0.clone().requires_grad_(True)
        if is_fused:
            y = ops.qnet_input(mesh, action, net.positional_embedding, net.mask_embedding.model[0].weight, net.layers[0].weight[0],
                               net.layers[0].bias, csr, 66)
        else:
            feats = torch.cat((action.unsqueeze(1).expand(-1, 1949, -1), net.positional_embedding(mesh[..., :3]),
                               net.mask_embedding(mesh[..., 3:])), dim=-1)
            y = net.layers[0](feats, csr, F.relu)
        y.backward(gy)

    growth = {}
    for name, net, is_fused in (("fused", fused, True), ("unfused", plain, False)):
        step(net, is_fused)                      # warm-up: the library's workspaces, torch's caches
        net.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(net, is_fused)
        torch.cuda.synchronize()
        growth[name] = torch.cuda.max_memory_allocated() - base
    print(f"\npeak growth over forward + backward: fused {growth['fused'] / 2 ** 20:.1f} MiB, unfused {growth['unfused'] / 2 ** 20:.1f} MiB")
    assert growth["fused"] <= 0.5 * growth["unfused"]


# ---- the learner, end to end ---------------------------------------------------------------------------------------------------------
def _learner(case, cuda, fused=True, device_replay=False):
    from a3vt_amd.pterotactyl.policies import replay
    from a3vt_amd.pterotactyl.policies.DDQN import ddqn
    args = du.case_args(case, fused_q_input=fused)
    torch.manual_seed(0)
    memory = replay.ReplayMemory(args, device=cuda if device_replay else None)
    info = _tp_info()
    learner = ddqn.DDQN(args, info, memory)
    target = du.perturbed_copy(learner, info)
    return learner.to(cuda), target.to(cuda), memory


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("case", ["a", "b"])
def test_update_matches_the_reference(cuda, case, fused):
    """One ``update_parameters`` of cases (a) / (b) against the reference's run: loss, q_cur, best_next, target, post-clamp
    gradients; in (b) the clamp bites and leaves max|grad| = 1 exactly; the weights afterwards are ``torch.optim.Adam``'s on the
    same clamped gradients (the bound ``test_gpu_adam.py`` uses for the fused step)."""
    from a3vt_amd import ops
    z = load("g16_ddqn_update.npz")
    learner, target, memory = _learner(case, cuda, fused)
    assert np.array_equal(state_sha256({k: v.cpu() for k, v in learner.model.state_dict().items()}), z[f"{case}:weight_sha256"])
    assert learner.model.fused_q_input is fused
    learner.add_experience(*du.transitions(z, case))
    before = [p.detach().clone().requires_grad_(True) for p in learner.model.parameters()]
    ops.path_counts(reset=True)
    np.random.seed(5)
    loss = learner.update_parameters(target)
    counts = ops.path_counts()
    assert (counts["qnet_input_fwd"], counts["qnet_input_bwd"]) == ((3, 1) if fused else (0, 0))     # online-current, online-next, target-next
    assert learner.optimizer.library_steps == 1
    assert np.array_equal(memory.last_indices, z[f"{case}:indices"])
    ref_loss = float(z[f"{case}:loss"])
    print(f"\ncase {case} fused={fused}: loss {loss:.6f} (reference {ref_loss:.6f})")
    assert abs(loss - ref_loss) / ref_loss < 1e-4
    q_cur = learner.last_q.gather(1, torch.from_numpy(z["actions"][z[f"{case}:indices"]]).long().to(cuda)[:, None]).squeeze(1)
    assert rel_err(q_cur, torch.from_numpy(z[f"{case}:q_cur"])) < 1e-4
    assert rel_err(learner.last_q, torch.from_numpy(z[f"{case}:q_all"])) < 1e-4
    assert np.array_equal(learner.last_best_next.cpu().numpy(), z[f"{case}:best_next"])
    assert rel_err(learner.last_target, torch.from_numpy(z[f"{case}:target"])) < 1e-4
    params = dict(learner.model.named_parameters())
    for key in [k for k in z.files if k.startswith(f"{case}:g:")]:
        name = key[4:]
        got = params[name].grad[..., ::3, ::5] if name == "layers.0.weight" else params[name].grad
        assert_grad_close(got, torch.from_numpy(z[key]), key)
    top = max(p.grad.abs().max().item() for p in params.values())
    if case == "b":
        assert top == 1.0
        share = (params["layers.2.weight"].grad.abs() == 1.0).float().mean().item()
        assert 0.0 < share < 1.0
    else:
        assert top < 1.0
    # the step: torch's Adam on the weights from before the update and the clamped gradients the update left behind
    for p, q in zip(before, learner.model.parameters()):
        p.grad = q.grad.clone()
    torch.optim.Adam(before, lr=learner.args.lr).step()
    for p, (k, q) in zip(before, learner.model.named_parameters()):
        torch.testing.assert_close(q.detach(), p.detach(), rtol=5e-7, atol=1e-8, msg=lambda m, k=k: f"{k}: {m}")


def test_get_action(cuda):
    z = load("g16_ddqn_update.npz")
    learner, _, _ = _learner("a", cuda)
    _, obs, _, _ = du.transitions(z, "a")
    with torch.no_grad():
        q = learner.model(obs)
    want = q.masked_fill(obs["mask"].to(cuda) > 0, -1e10).argmax(dim=1).cpu().numpy()
    got = learner.get_action(obs, 0.0)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    assert (z["mask"][np.arange(6), got] == 0).all()
    # an observation whose best unpenalised action has been taken already
    taken = {"mesh": obs["mesh"], "mask": torch.zeros(6, 50)}
    taken["mask"][np.arange(6), q.argmax(dim=1).cpu().numpy()] = 1
    assert (taken["mask"].numpy()[np.arange(6), learner.get_action(taken, 0.0)] == 0).all()
    from a3vt_amd.pterotactyl.policies.baselines import baselines
    random.seed(9)
    got = [learner.get_action(obs, 1.0) for _ in range(3)]
    random.seed(9)
    sampler = baselines.random_sampler(learner.args)
    for a in got:
        random.random()                          # get_action's own draw against eps
        assert np.array_equal(a, sampler.get_action(obs["mask"]))
        assert (z["mask"][np.arange(6), a] == 0).all()
    assert np.array_equal(learner.get_action(obs, 0.0, give_random=True).shape, (6,))


def test_device_replay(cuda):
    """A replay memory built with ``device=``: the same samples as the host one under the same seed, on the device; the update
    gives the same loss bits with either."""
    z = load("g16_ddqn_update.npz")
    losses = []
    batches = []
    for device_replay in (False, True):
        learner, target, memory = _learner("b", cuda, device_replay=device_replay)
        learner.add_experience(*du.transitions(z, "b"))
        assert memory.mesh.is_cuda is device_replay
        np.random.seed(5)
        batches.append(memory.sample())
        np.random.seed(5)
        losses.append(learner.update_parameters(target))
    host, dev = batches
    assert set(host) == set(dev)
    for k in host:
        assert dev[k].is_cuda and not host[k].is_cuda and torch.equal(dev[k].cpu(), host[k]), k
    assert losses[0] == losses[1]
