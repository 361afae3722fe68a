"""-m gpu: DDQN's ``Latent_Model`` on ``ops.ddqn_latent_q`` / ``ops.ddqn_latent_update`` (csrc/ddqn_latent.hip).

* every output of the three-launch update is BIT-IDENTICAL to the composition of the existing entry points on the same operands
  (``latent_policy_fwd`` x 3, ``a3vt_ddqn_td``, ``a3vt_ddqn_td_bwd`` under a unit gradient, ``latent_policy_bwd(accumulate=False)``):
  the kernels share their device code (csrc/policy_dev.h), so ``torch.equal`` is the bound;
* repeatability, row permutation, the action choice against ``masked_fill(mask > 0, -1e10).argmax(1)``;
* one fused ``update_parameters`` of case (c) of ``g16_ddqn_update.npz`` (a reference run) within the bounds ``test_ddqn_host.py``
  applies to that case on the CPU, with host and device replay;
* launch counters, and that a target copy / an optimizer step is seen by the next call without a table rebuild.
"""
import ctypes

import numpy as np
import pytest
import torch

import ddqn_util as du
from golden_util import load, state_sha256
from helpers import assert_grad_close, rel_err

pytestmark = pytest.mark.gpu

BUDGET = 5
# (layer sizes (in, out, relu), concat_at): g16 case (c) — A 50, latent 200, hidden 100, 3 layers — and a table with no width a multiple
# of 4 (A 7, latent 10, hidden 37, 2 layers; the embedding 7 -> 13 -> 9 -> 10), so every layer takes the scalar-load path
TABLES = {
    "g16c": ([(50, 200, 1), (200, 100, 1), (100, 200, 0), (600, 100, 1), (100, 100, 1), (100, 50, 0)], 3),
    "odd": ([(7, 13, 1), (13, 9, 1), (9, 10, 0), (30, 37, 1), (37, 7, 0)], 3),
}


def _table(name, seed, dev):
    from a3vt_amd import ops
    dims, concat_at = TABLES[name]
    g = torch.Generator().manual_seed(seed)
    layers = []
    for n_in, n_out, relu in dims:
        bound = 1.0 / np.sqrt(n_in)                                       # torch's Linear init range
        layers.append((((torch.rand(n_out, n_in, generator=g) * 2 - 1) * bound).to(dev),
                       ((torch.rand(n_out, generator=g) * 2 - 1) * bound).to(dev), relu))
    return ops.PolicyTable(layers, concat_at, None)


def _batch(table, B, seed, dev):
    """Replay rows of every kind, cycling with the row index: one action taken (not done), budget - 1 taken (done), every action
    taken, a stored action outside [0, A), nothing taken."""
    A, ls = table.num_actions, table.latent_size
    g = torch.Generator().manual_seed(seed)
    mask, actions = torch.zeros(B, A), torch.zeros(B)
    for b in range(B):
        kind = (b + B) % 5
        taken = {0: 1, 1: min(BUDGET - 1, A), 2: A, 3: 2, 4: 0}[kind]
        mask[b, torch.randperm(A, generator=g)[:taken]] = 1
        actions[b] = float(torch.randint(0, A, (1,), generator=g))
        if kind == 3:
            actions[b] = -3.0 if b % 2 else float(A + 5)
    mask_n = mask.clone()
    inside = (actions >= 0) & (actions < A)
    mask_n[inside, actions[inside].long()] = 1
    d = dict(mask=mask, mask_n=mask_n, latent=torch.randn(B, ls, generator=g), latent_n=torch.randn(B, ls, generator=g),
             first_latent=torch.randn(B, ls, generator=g), actions=actions, rewards=torch.rand(B, generator=g),
             denom=1.0 + torch.rand(B, generator=g))
    return {k: v.to(dev) for k, v in d.items()}


def _zero_grads(table):
    return [(torch.zeros_like(w), torch.zeros_like(b)) for w, b, _ in table.layers]


def _composed(online, target, d, denom, gamma):
    """The existing entry points, one after another, on the same operands."""
    from a3vt_amd import lib, ops
    L = lib.load()
    B, A = d["mask"].shape[0], online.num_actions
    dev = d["mask"].device
    q_cur, _, stash = ops.latent_policy_fwd(online, d["mask"], d["latent"], d["first_latent"], None, stash=True)
    q_no, _, _ = ops.latent_policy_fwd(online, d["mask_n"], d["latent_n"], d["first_latent"])
    q_nt, _, _ = ops.latent_policy_fwd(target, d["mask_n"], d["latent_n"], d["first_latent"])
    loss = torch.empty((), device=dev)
    diff, tgt, best = torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.check(L.a3vt_ddqn_td(lib.ptr(q_cur), lib.ptr(q_no), lib.ptr(q_nt), lib.ptr(d["mask"]), lib.ptr(d["actions"]), lib.ptr(d["rewards"]),
                             lib.ptr(denom), B, A, BUDGET, float(gamma), lib.ptr(loss), lib.ptr(diff), lib.ptr(best), lib.ptr(tgt), s), "td")
    one, dq = torch.ones((), device=dev), torch.empty(B, A, device=dev)
    lib.check(L.a3vt_ddqn_td_bwd(lib.ptr(diff), lib.ptr(d["actions"]), lib.ptr(one), B, A, lib.ptr(dq), s), "td_bwd")
    grads = _zero_grads(online)
    ops.latent_policy_bwd(online, d["mask"], d["latent"], d["first_latent"], dq, stash, grads, accumulate=False)
    return dict(loss=loss, q_cur=q_cur, best=best, target=tgt, diff=diff), grads


def _fused(online, target, d, denom, gamma, grads=None):
    from a3vt_amd import ops
    grads = _zero_grads(online) if grads is None else grads
    for dw, db in grads:                                   # the op overwrites: whatever the tensors held must not show
        dw.fill_(7.0)
        db.fill_(-7.0)
    loss, q_cur, best, tgt, diff = ops.ddqn_latent_update(online, target, grads, d["mask"], d["mask_n"], d["latent"], d["latent_n"],
                                                          d["first_latent"], d["actions"], d["rewards"], denom, BUDGET, gamma)
    return dict(loss=loss, q_cur=q_cur, best=best, target=tgt, diff=diff), grads


@pytest.mark.parametrize("gamma", [0.0, 0.9])
@pytest.mark.parametrize("B", [1, 5, 16, 67])
@pytest.mark.parametrize("name", ["g16c", "odd"])
def test_update_is_bit_identical_to_the_composed_entry_points(cuda, name, B, gamma):
    from a3vt_amd import ops
    online, target = _table(name, 0, cuda), _table(name, 1, cuda)
    assert ops.ddqn_latent_supported(online, torch.zeros(B, online.in_width, device=cuda))
    d = _batch(online, B, 10 * B + 1, cuda)
    for denom in (None, d["denom"]):
        want, want_g = _composed(online, target, d, denom, gamma)
        ops.ddqn_latent_launches(reset=True)
        ops.policy_launches(reset=True)
        got, got_g = _fused(online, target, d, denom, gamma)
        assert ops.ddqn_latent_launches() == {"q": 0, "update": 3} and sum(ops.policy_launches().values()) == 0
        for k in want:
            assert torch.equal(got[k], want[k]), (k, denom is None)
        for l, ((dw, db), (rw, rb)) in enumerate(zip(got_g, want_g)):
            assert torch.equal(dw, rw) and torch.equal(db, rb), (l, denom is None)
        assert torch.isfinite(got["loss"]) and got["q_cur"].shape == (B, online.num_actions)
        # the kinds of rows the batch was built from did occur
        done = d["mask"].sum(1) >= BUDGET - 1
        if B >= 5:
            assert done.any() and (~done).any() and (d["mask"].sum(1) == online.num_actions).any()
            assert ((d["actions"] < 0) | (d["actions"] >= online.num_actions)).any()
        if gamma == 0.0:
            r = d["rewards"] if denom is None else d["rewards"] / denom
            assert torch.equal(got["target"], r + 0.0)


def test_repeated_call_and_row_permutation(cuda):
    online, target = _table("g16c", 2, cuda), _table("g16c", 3, cuda)
    d = _batch(online, 16, 5, cuda)
    a, ga = _fused(online, target, d, d["denom"], 0.9)
    a = {k: v.clone() for k, v in a.items()}
    ga = [(dw.clone(), db.clone()) for dw, db in ga]
    b, gb = _fused(online, target, d, d["denom"], 0.9)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for (dw, db), (rw, rb) in zip(ga, gb):
        assert torch.equal(dw, rw) and torch.equal(db, rb)
    perm = torch.randperm(16, generator=torch.Generator().manual_seed(4)).to(cuda)
    p, _ = _fused(online, target, {k: v[perm].contiguous() for k, v in d.items()}, d["denom"][perm].contiguous(), 0.9)
    for k in ("q_cur", "best", "target", "diff"):                  # per-row outputs travel with their rows, bit for bit
        assert torch.equal(p[k], a[k][perm]), k


def test_q_and_action_choice(cuda):
    from a3vt_amd import ops
    for name in TABLES:
        table = _table(name, 6, cuda)
        A = table.num_actions
        w, b, _ = table.layers[-1]
        with torch.no_grad():                                      # values half a unit apart: a gap far above 1e-2 relative
            w.mul_(0.001)
            b.copy_((torch.randperm(A, generator=torch.Generator().manual_seed(7)).float() * 0.5).to(cuda))
        d = _batch(table, 16, 8, cuda)
        want_q, _, _ = ops.latent_policy_fwd(table, d["mask"], d["latent"], d["first_latent"])
        ops.ddqn_latent_launches(reset=True)
        q, action = ops.ddqn_latent_q(table, d["mask"], d["latent"], d["first_latent"], d["mask"])
        q_only, none = ops.ddqn_latent_q(table, d["mask"], d["latent"], d["first_latent"])
        assert ops.ddqn_latent_launches() == {"q": 2, "update": 0}
        assert none is None and torch.equal(q, want_q) and torch.equal(q_only, want_q)
        pen = q.masked_fill(d["mask"] > 0, -1e10)
        top = pen.topk(2, dim=1).values
        open_rows = (d["mask"] == 0).sum(1) >= 2
        gap = ((top[:, 0] - top[:, 1]) / top[:, 0].abs().clamp_min(1e-30))[open_rows].min().item()
        print(f"\n{name}: smallest relative gap between the two best open values {gap:.3e}")
        assert gap > 1e-2
        assert action.dtype == torch.int32 and torch.equal(action.long(), pen.argmax(1))
        full = d["mask"].sum(1) == A
        assert full.any() and (action[full] == 0).all()            # every action taken: index 0, as ddqn_td_kernel's rule gives


# ---- the learner ------------------------------------------------------------------------------------------------------------------
def _learner(tmp_path, cuda, fused=True, device_replay=False, **kw):
    from a3vt_amd.pterotactyl.policies import replay
    from a3vt_amd.pterotactyl.policies.DDQN import ddqn
    args = du.case_args("c", du.write_auto_config(str(tmp_path)), fused_q_latent=fused, **kw)
    torch.manual_seed(0)
    memory = replay.ReplayMemory(args, device=cuda if device_replay else None)
    learner = ddqn.DDQN(args, None, memory)
    target = du.perturbed_copy(learner)
    return learner.to(cuda), target.to(cuda), memory


@pytest.mark.parametrize("device_replay", [False, True])
def test_fused_update_matches_the_reference(cuda, tmp_path, device_replay):
    """Case (c) of g16: one fused ``update_parameters`` on the GPU against the reference's run, within the bounds
    ``test_ddqn_host.py::test_latent_update_matches_the_reference`` applies on the CPU (loss, target 1e-4 relative; best_next equal;
    gradients by ``assert_grad_close``), ``q_all`` within the same 1e-4, and the step = torch's Adam on the clamped gradients.
    Measured on an MI355X, host and device replay alike: loss equal to the printed digits, ``q_all`` 1.7e-7, target 7.7e-8."""
    from a3vt_amd import ops
    from a3vt_amd.pterotactyl.policies.DDQN import model
    z = load("g16_ddqn_update.npz")
    learner, target, memory = _learner(tmp_path, cuda, device_replay=device_replay)
    assert isinstance(learner.model, model.Latent_Model) and learner.model.fused_q_latent
    assert np.array_equal(state_sha256({k: v.cpu() for k, v in learner.model.state_dict().items()}), z["c:weight_sha256"])
    learner.add_experience(*du.transitions(z, "c"))
    before = [p.detach().clone().requires_grad_(True) for p in learner.model.parameters()]
    ops.ddqn_latent_launches(reset=True)
    ops.policy_launches(reset=True)
    np.random.seed(5)
    loss = learner.update_parameters(target)
    assert ops.ddqn_latent_launches() == {"q": 0, "update": 3} and sum(ops.policy_launches().values()) == 0
    assert learner.optimizer.library_steps == 1
    assert np.array_equal(memory.last_indices, z["c:indices"])
    ref_loss = float(z["c:loss"])
    errs = dict(loss=abs(loss - ref_loss) / ref_loss, q_all=rel_err(learner.last_q, torch.from_numpy(z["c:q_all"])),
                target=rel_err(learner.last_target, torch.from_numpy(z["c:target"])))
    print(f"\ncase c fused, device_replay={device_replay}: loss {loss:.6f} (reference {ref_loss:.6f}); relative errors {errs}")
    assert all(e < 1e-4 for e in errs.values()), errs
    assert np.array_equal(learner.last_best_next.cpu().numpy(), z["c:best_next"])
    params = dict(learner.model.named_parameters())
    for key in [k for k in z.files if k.startswith("c:g:")]:
        name = key[4:]
        got = params[name].grad[::3, ::5] if name == "model.0.0.weight" else params[name].grad
        assert_grad_close(got, torch.from_numpy(z[key]), key)
    for p, q in zip(before, learner.model.parameters()):
        p.grad = q.grad.clone()
    torch.optim.Adam(before, lr=learner.args.lr).step()
    for p, (k, q) in zip(before, learner.model.named_parameters()):
        torch.testing.assert_close(q.detach(), p.detach(), rtol=5e-7, atol=1e-8, msg=lambda m, k=k: f"{k}: {m}")
    # the gradient tensors are the learner's own and are written in place by the next update
    owned = [p.grad for p in learner.model.parameters()]
    np.random.seed(6)
    learner.update_parameters(target)
    assert all(p.grad is g for p, g in zip(learner.model.parameters(), owned)) and learner.optimizer.library_steps == 2


def test_get_action_is_one_launch_and_one_copy_of_E_integers(cuda, tmp_path):
    from a3vt_amd import ops
    z = load("g16_ddqn_update.npz")
    learner, _, _ = _learner(tmp_path, cuda)
    plain, _, _ = _learner(tmp_path, cuda, fused=False)
    _, obs, _, _ = du.transitions(z, "c")
    with torch.no_grad():
        q = plain.model(obs)
    pen = q.masked_fill(obs["mask"].to(cuda) > 0, -1e10)
    top = pen.topk(2, dim=1).values
    assert ((top[:, 0] - top[:, 1]) / top[:, 0].abs()).min().item() > 1e-4      # (fp32 module values against the kernel's: ~1e-6)
    # counted as test_gpu_supervised.py::test_one_host_tensor_of_E_integers_leaves_a_model_call counts: whatever brings a device
    # tensor to the host (or waits for one) while the choice runs
    copies = []
    originals = {name: getattr(torch.Tensor, name) for name in ("cpu", "item", "tolist", "numpy", "__bool__", "__int__", "__float__")}

    def counted(name):
        def method(self, *a, **k):
            if self.is_cuda:
                copies.append((name, tuple(self.shape), self.dtype))
            return originals[name](self, *a, **k)
        return method

    ops.ddqn_latent_launches(reset=True)
    for name in originals:
        setattr(torch.Tensor, name, counted(name))
    try:
        got = learner.get_action(obs, eps_threshold=-1)
    finally:
        for name, fn in originals.items():
            setattr(torch.Tensor, name, fn)
    assert ops.ddqn_latent_launches() == {"q": 1, "update": 0}
    assert copies == [("cpu", (6,), torch.int32)] and learner.copied == [((6,), torch.int32)]
    assert isinstance(got, np.ndarray) and np.array_equal(got, pen.argmax(1).cpu().numpy())
    assert np.array_equal(got, plain.get_action(obs, eps_threshold=-1)) and plain.copied == []
    assert ops.ddqn_latent_launches() == {"q": 1, "update": 0}                   # the knob-off learner stays on the modules


def test_the_next_call_sees_a_target_copy_and_an_optimizer_step(cuda, tmp_path):
    from a3vt_amd import ops
    z = load("g16_ddqn_update.npz")
    learner, target, _ = _learner(tmp_path, cuda)
    learner.add_experience(*du.transitions(z, "c"))
    _, obs, _, _ = du.transitions(z, "c")
    net = learner.model
    mask, latent, first = net.inputs(obs)
    table, ttable = net.table(), target.model.table()
    structs = (ctypes.addressof(table.struct()), ctypes.addressof(ttable.struct()))
    q0, _ = ops.ddqn_latent_q(table, mask, latent, first)
    np.random.seed(5)
    learner.update_parameters(target)
    t0 = learner.last_target.clone()
    q1, _ = ops.ddqn_latent_q(net.table(), mask, latent, first)
    with torch.no_grad():
        want = net(obs)
    assert not torch.equal(q1, q0) and rel_err(q1, want) < 1e-5                   # the step moved the weights the kernel reads
    target.load_state_dict(learner.state_dict())                                 # in place: the same tensors, the same table
    assert target.model.table() is ttable and net.table() is table
    assert (ctypes.addressof(table.struct()), ctypes.addressof(ttable.struct())) == structs
    grads = _zero_grads(table)
    b = {k: v.to(cuda) for k, v in learner.replay.sample().items()}
    args = (grads, b["mask"], b["mask_n"], b["latent"], b["latent_n"], b["first_latent"], b["actions"], b["rewards"], None, 5, 0.9)
    with_copy = ops.ddqn_latent_update(table, ttable, *args)
    with_self = ops.ddqn_latent_update(table, table, *args)
    for a, c in zip(with_copy, with_self):
        assert torch.equal(a, c)
    assert t0.shape == with_copy[3].shape
