"""CPU tests of the DDQN learner's host side: replay memory, action samplers, the learner's bookkeeping, the latent-model update
(case (c) of ``g16_ddqn_update.npz``, a reference run) end to end, the torch-op flavour of ``ops.ddqn_td`` and the argument checks
of the new C entry points (fake device pointers that must never be dereferenced)."""
import ctypes
import random

import numpy as np
import pytest
import torch

import ddqn_util as du
from golden_util import load, state_sha256
from helpers import assert_grad_close, rel_err


@pytest.fixture(scope="module")
def z():
    return load("g16_ddqn_update.npz")


def _modules():
    from a3vt_amd.pterotactyl.policies import replay
    from a3vt_amd.pterotactyl.policies.baselines import baselines
    from a3vt_amd.pterotactyl.policies.DDQN import ddqn
    return replay, baselines, ddqn


def _latent_args(tmp_path, **kw):
    return du.case_args("c", du.write_auto_config(str(tmp_path)), **kw)


def _push(memory, n, start=0):
    obs = {"score": np.arange(start, start + n) + 0.5, "first_score": np.ones(n), "mask": torch.zeros(n, 50),
           "latent": torch.arange(start, start + n).float()[:, None].expand(n, 200), "first_latent": torch.zeros(n, 200)}
    nxt = {"score": np.zeros(n), "mask": torch.ones(n, 50), "latent": torch.zeros(n, 200)}
    memory.push(np.arange(start, start + n), obs, nxt, np.arange(start, start + n) * 0.1)


def test_facade_registers_the_policy_modules():
    import subprocess
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); import a3vt_amd; a3vt_amd.install_as_pterotactyl();"
            "import pterotactyl.policies.DDQN.ddqn as d, pterotactyl.policies.replay as r, pterotactyl.policies.baselines.baselines as b;"
            "assert d.DDQN.__module__.startswith('a3vt_amd') and hasattr(r, 'ReplayMemory') and hasattr(b, 'even_sampler'); print('ok')") % root
    assert subprocess.run([sys.executable, "-c", code], capture_output=True, text=True).stdout.strip() == "ok"


def test_replay_ring_wraps_and_waits_for_burn_in(tmp_path):
    replay, _, _ = _modules()
    args = _latent_args(tmp_path, mem_capacity=5, burn_in=4, train_batch_size=2)
    memory = replay.ReplayMemory(args)
    for name in ("mask", "mask_n", "actions", "rewards", "score", "score_n", "first_score", "latent", "latent_n", "first_latent"):
        assert getattr(memory, name).shape[0] == 5, name
    assert not hasattr(memory, "mesh")
    _push(memory, 3)
    assert memory.sample() is None and (memory.position, memory.count_seen) == (3, 3)     # below burn_in
    _push(memory, 4, start=3)
    assert (memory.position, memory.count_seen) == (2, 7)
    assert memory.actions.tolist() == [5.0, 6.0, 2.0, 3.0, 4.0]                          # the two oldest were overwritten
    assert memory.latent[:, 0].tolist() == [5.0, 6.0, 2.0, 3.0, 4.0] and torch.allclose(memory.score, memory.actions + 0.5)
    batch = memory.sample()
    assert batch["mask"].shape == (2, 50) and set(batch) == {"mask", "mask_n", "actions", "rewards", "score", "score_n", "first_score",
                                                              "latent", "latent_n", "first_latent"}
    args2 = _latent_args(tmp_path, mem_capacity=5, burn_in=0, train_batch_size=4)
    memory = replay.ReplayMemory(args2)
    _push(memory, 3)
    assert memory.sample() is None                                                        # fewer than a batch


def test_replay_mesh_width(tmp_path):
    replay, _, _ = _modules()
    for finger, grasps, n in ((True, 5, 1949), (False, 5, 2324), (False, 1, 1924)):
        memory = replay.ReplayMemory(du.case_args("a", mem_capacity=2, finger=finger, num_grasps=grasps))
        assert memory.mesh.shape == (2, n, 4) and memory.mesh_n.shape == (2, n, 4)


@pytest.mark.parametrize("case", du.CASES)
def test_replay_seeded_indices_are_the_references(z, tmp_path, case):
    replay, _, _ = _modules()
    memory = replay.ReplayMemory(du.case_args(case, du.write_auto_config(str(tmp_path))))
    memory.push(*du.transitions(z, case))
    np.random.seed(5)
    batch = memory.sample()
    assert np.array_equal(memory.last_indices, z[f"{case}:indices"])
    assert torch.equal(batch["mask"], torch.from_numpy(z["mask"][z[f"{case}:indices"]]))
    assert torch.equal(batch["score_n"], torch.from_numpy(z["score_n"][z[f"{case}:indices"]]))


def test_replay_save_load_and_reference_key_set(tmp_path):
    replay, _, _ = _modules()
    args = _latent_args(tmp_path, mem_capacity=5)
    memory = replay.ReplayMemory(args)
    _push(memory, 7)
    stem = str(tmp_path / "run")
    memory.save(stem)
    assert not (tmp_path / "run_replay_buffer_temp.pt").exists()
    data = torch.load(stem + "_replay_buffer.pt")
    assert set(data) == {"mask", "mask_n", "actions", "rewards", "score", "first_score", "position", "count_seen", "latent", "latent_n",
                         "first_latent"}                                                  # the reference's keys: no score_n
    assert all(not v.is_cuda for v in data.values() if isinstance(v, torch.Tensor))
    other = replay.ReplayMemory(args)
    other.load(stem)
    for name in data:
        a, b = getattr(other, name), getattr(memory, name)
        assert torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b, name
    # a file as the reference writes it (its dict, its order) loads
    ref_file = {"mask": torch.ones(5, 50), "mask_n": torch.zeros(5, 50), "actions": torch.arange(5.0), "rewards": torch.ones(5),
                "score": torch.ones(5), "first_score": torch.ones(5), "position": 3, "count_seen": 13,
                "latent": torch.ones(5, 200), "latent_n": torch.ones(5, 200), "first_latent": torch.ones(5, 200)}
    torch.save(ref_file, str(tmp_path / "ref_replay_buffer.pt"))
    other.load(str(tmp_path / "ref"))
    assert (other.position, other.count_seen) == (3, 13) and other.actions.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]


def test_random_sampler_avoids_the_mask_and_follows_the_reference(z):
    _, baselines, _ = _modules()
    sampler = baselines.random_sampler(du.case_args("a"))
    random.seed(7)
    got = np.stack([sampler.get_action(z["mask"]) for _ in range(3)])
    assert np.array_equal(got, z["sampler_actions"])
    assert np.array_equal(sampler.get_action(torch.from_numpy(z["mask"])).shape, (6,))
    g = np.random.default_rng(0)
    mask = (g.random((40, 50)) < 0.9).astype(np.float32)
    mask[:, 17] = 0                                           # at least one free action per row
    for _ in range(5):
        picked = sampler.get_action(mask)
        assert (mask[np.arange(40), picked] == 0).all()


def test_even_sampler_spreads_the_grasps():
    _, baselines, _ = _modules()
    args = du.case_args("a", env_batch_size=3)
    random.seed(3)
    sampler = baselines.even_sampler(args)
    random.seed(3)
    offsets = [random.choice(range(50)) for _ in range(3)]
    for step in range(5):
        assert sampler.get_action(np.zeros((3, 50))).tolist() == [(10 * step + o) % 50 for o in offsets]
    sampler.reset()
    assert all(len(a) == 5 for a in sampler.angles)


def test_get_model_pretrained_table_and_knob(tmp_path):
    _, _, ddqn = _modules()
    table = {(True, True, True): (300, 5), (True, True, False): (300, 5), (True, False, True): (300, 5), (True, False, False): (300, 2),
             (False, True, True): (100, 5), (False, True, False): (100, 5), (False, False, True): (100, 5), (False, False, False): (100, 2)}
    for (latent, img, finger), (hidden, layers) in table.items():
        args = du.case_args("c" if latent else "a", du.write_auto_config(str(tmp_path)), pretrained=True, use_img=img, finger=finger,
                            use_latent=latent, use_recon=not latent, hidden_dim=7, layers=9)
        learner = ddqn.DDQN(args, {"adj": torch.eye(4)}, None)
        assert (args.hidden_dim, args.layers) == (hidden, layers)
        assert args.fused_q_input is ddqn.FUSED_Q_INPUT_DEFAULT          # args did not carry the knob: get_model set it
        if not latent:
            assert learner.model.fused_q_input is ddqn.FUSED_Q_INPUT_DEFAULT and len(learner.model.layers) == layers and learner.model.layers[0].weight.shape[-1] == hidden
    for knob in (False, True):
        args = du.case_args("a", fused_q_input=knob)
        assert ddqn.DDQN(args, {"adj": torch.eye(4)}, None).model.fused_q_input is knob
    args = du.case_args("a", use_recon=False)
    with pytest.raises(SystemExit):
        ddqn.DDQN(args, {"adj": torch.eye(4)}, None)


def test_update_epsilon(tmp_path):
    _, _, ddqn = _modules()
    args = _latent_args(tmp_path)
    learner = ddqn.DDQN(args, None, None)
    assert learner.update_epsilon(1.0, args) == pytest.approx(0.9)
    assert learner.update_epsilon(0.05, args) == 0.05 and learner.update_epsilon(0.01, args) == 0.05


def test_latent_update_matches_the_reference(z, tmp_path):
    """Case (c): one ``update_parameters`` of the latent model on the CPU against the reference's run."""
    replay, _, ddqn = _modules()
    args = _latent_args(tmp_path)
    torch.manual_seed(0)
    memory = replay.ReplayMemory(args)
    learner = ddqn.DDQN(args, None, memory)
    assert np.array_equal(state_sha256(learner.model.state_dict()), z["c:weight_sha256"]), "init differs from the reference"
    target = du.perturbed_copy(learner)
    assert learner.update_parameters(target) is None                    # nothing to sample yet
    learner.add_experience(*du.transitions(z, "c"))
    before = {k: p.detach().clone() for k, p in learner.model.named_parameters()}
    np.random.seed(5)
    loss = learner.update_parameters(target)
    assert abs(loss - float(z["c:loss"])) / float(z["c:loss"]) < 1e-4
    assert np.array_equal(learner.last_best_next.numpy(), z["c:best_next"])
    assert rel_err(learner.last_target, torch.from_numpy(z["c:target"])) < 1e-4
    params = dict(learner.model.named_parameters())
    for key in [k for k in z.files if k.startswith("c:g:")]:
        name = key[4:]
        got = params[name].grad[::3, ::5] if name == "model.0.0.weight" else params[name].grad
        assert_grad_close(got, torch.from_numpy(z[key]), key)
    assert all(not torch.equal(before[k], p) for k, p in params.items())    # the step moved every tensor


def test_ddqn_td_on_torch_ops_matches_the_fixture(z):
    """The torch-op flavour of the rule on the fixture's recorded Q values.  The next-state values are BUILT here so that the
    penalised argmax and the gathered target values are the recorded ones: this covers the penalty, the not-done rule, the
    normalisation, the loss and its gradient, not the network values behind ``best_next`` (those come from real forwards in
    ``test_latent_update_matches_the_reference`` and in the GPU cases).  Both flavours keep an action outside the table inside
    the row."""
    from a3vt_amd import ops
    for case in ("a", "b"):
        idx = z[f"{case}:indices"]
        q_all = torch.from_numpy(z[f"{case}:q_all"]).requires_grad_(True)
        # any next-state values whose penalised argmax / gathered values are the recorded ones
        g = torch.Generator().manual_seed(3)
        q_no = torch.rand(4, 50, generator=g)
        q_nt = torch.rand(4, 50, generator=g)
        mask = torch.from_numpy(z["mask"][idx])
        best = torch.from_numpy(z[f"{case}:best_next"]).long()
        q_no[torch.arange(4), best] = 2.0
        q_no[mask > 0] = 5.0                                      # larger still, but penalised
        rewards = torch.from_numpy((z["rewards_b"] if case == "b" else z["rewards"])[idx])
        denom = torch.from_numpy(z["first_score"][idx]) if case == "a" else None
        norm = rewards / denom if denom is not None else rewards
        nxt = (torch.from_numpy(z[f"{case}:target"]) - norm) / 0.9
        q_nt[torch.arange(4), best] = nxt
        loss, got_best, target = ops.ddqn_td(q_all, q_no, q_nt, mask, torch.from_numpy(z["actions"][idx]).float(), rewards, denom, 5, 0.9)
        assert got_best.dtype == torch.int32 and np.array_equal(got_best.numpy(), z[f"{case}:best_next"])
        assert rel_err(target, torch.from_numpy(z[f"{case}:target"])) < 1e-5
        assert np.array_equal((target - norm == 0).numpy(), ~z[f"{case}:not_done"])        # done rows: the reward alone
        assert abs(loss.item() - float(z[f"{case}:loss"])) / float(z[f"{case}:loss"]) < 1e-4
        loss.backward()
        col = torch.from_numpy(z["actions"][idx]).long()
        want = torch.zeros(4, 50)
        want[torch.arange(4), col] = 2 * (torch.from_numpy(z[f"{case}:q_cur"]) - torch.from_numpy(z[f"{case}:target"])) / 4
        assert rel_err(q_all.grad, want) < 1e-5
    q = torch.arange(6.0).reshape(2, 3)
    loss, _, target = ops.ddqn_td(q, q, q, torch.zeros(2, 3), torch.tensor([-1.0, 7.0]), torch.zeros(2), None, 5, 0.0)
    assert loss.item() == (0.0 ** 2 + 5.0 ** 2) / 2          # columns 0 and 2: what the kernel's clamp picks


def test_unfused_fp32_layer0_stays_inside_the_gradient_caps():
    """What ``test_gpu_ddqn.py`` relies on for its fp64 comparison: layer 0 of the graph model restated on torch ops in fp32 stays
    inside ``assert_grad_close``'s caps against the same formulas in fp64 under the RANDOM upstream gradient those tests use (t_p,
    B = 3, hidden 200, every gradient the fused kernel or its composites produce)."""
    from a3vt_amd.pterotactyl.policies.DDQN import model as dm
    adj = du.tp_dense_adjacency()
    torch.manual_seed(0)
    net = dm.Graph_Model(du.case_args("a"), {"adj": adj})
    obs = du.random_obs(3, adj.shape[0], 7, empty_sample=1)
    assert sorted(obs["mesh"][..., 3].unique().tolist()) == [0.0, 1.0, 2.0, 3.0]
    action = net.action_model(obs["mask"])
    gy = du.random_gy((3, adj.shape[0], 200))
    p = du.layer0_params(net)
    y32, g32 = du.layer0_run(p, obs["mesh"], action, adj, 66, gy, torch.float32)
    y64, g64 = du.layer0_run(p, obs["mesh"], action, adj, 66, gy, torch.float64)
    assert rel_err(y32, y64) < 1e-5
    for k in g64:
        assert_grad_close(g32[k], g64[k], k)


# ---- argument checks of the new C entry points -----------------------------------------------------------------------------------
FAKE = ctypes.c_void_p(0x7F0000001000)       # a "device pointer": 16-byte aligned, never mapped on the host
FAKE_ODD = ctypes.c_void_p(0x7F0000001008)


@pytest.fixture(scope="module")
def L():
    from a3vt_amd import lib
    return lib.load()


def _err(L):
    return L.a3vt_last_error().decode()


def _td(L, batch=4, actions=50, **kw):
    a = dict(q_cur=FAKE, q_no=FAKE, q_nt=FAKE, mask=FAKE, act=FAKE, rew=FAKE, denom=None, loss=FAKE, diff=FAKE, best=FAKE, target=FAKE)
    a.update(kw)
    return L.a3vt_ddqn_td(a["q_cur"], a["q_no"], a["q_nt"], a["mask"], a["act"], a["rew"], a["denom"], batch, actions, 5, 0.9, a["loss"],
                          a["diff"], a["best"], a["target"], None)


def test_td_entry_points_refuse_bad_arguments(L):
    for bad in (dict(batch=0), dict(batch=4097), dict(actions=0), dict(actions=305), dict(q_cur=None), dict(q_no=None), dict(q_nt=None),
                dict(mask=None), dict(act=None), dict(rew=None), dict(loss=None), dict(diff=None), dict(best=None), dict(target=None)):
        assert _td(L, **bad) != 0, bad
        assert "argument check failed" in _err(L), bad
    for bad in ((None, FAKE, FAKE, 4, 50, FAKE), (FAKE, None, FAKE, 4, 50, FAKE), (FAKE, FAKE, None, 4, 50, FAKE), (FAKE, FAKE, FAKE, 4, 50, None),
                (FAKE, FAKE, FAKE, 0, 50, FAKE), (FAKE, FAKE, FAKE, 4097, 50, FAKE), (FAKE, FAKE, FAKE, 4, 305, FAKE)):
        assert L.a3vt_ddqn_td_bwd(*bad, None) != 0, bad


def _qnet(L, bwd=False, hidden=200, cut=66, n_vert=100, batch=2, ld=200, **kw):
    a = dict(mesh=FAKE, w1=FAKE, b1=FAKE, w2=FAKE, b2=FAKE, s=FAKE, t=FAKE, c=FAKE, bias=FAKE, rowptr=FAKE, col=FAKE, val=FAKE, y=FAKE,
             scratch=FAKE, gy=FAKE, out=FAKE)
    a.update(kw)
    if not bwd:
        return L.a3vt_qnet_input_fwd(a["mesh"], a["w1"], a["b1"], a["w2"], a["b2"], a["s"], a["t"], a["c"], a["bias"], hidden, cut, a["rowptr"],
                                     a["col"], a["val"], 6, n_vert, batch, a["y"], ld, a["scratch"], None)
    return L.a3vt_qnet_input_bwd(a["mesh"], a["w1"], a["b1"], a["w2"], a["b2"], a["c"], hidden, cut, a["rowptr"], a["col"], a["val"], 6, n_vert,
                                 batch, a["y"], ld, a["gy"], ld, a["out"], FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, a["bias"], a["scratch"], None)


def test_qnet_input_entry_points_refuse_bad_arguments(L):
    for bwd in (False, True):
        for bad in (dict(hidden=305, ld=308), dict(hidden=0), dict(cut=-1), dict(cut=201), dict(n_vert=0), dict(batch=0), dict(mesh=None),
                    dict(w1=None), dict(b2=None), dict(c=None), dict(bias=None), dict(rowptr=None), dict(val=None), dict(y=None),
                    dict(scratch=None), dict(ld=196), dict(mesh=FAKE_ODD), dict(c=FAKE_ODD), dict(scratch=FAKE_ODD)):
            assert _qnet(L, bwd, **bad) != 0, (bwd, bad)
            assert _err(L), (bwd, bad)
    assert _qnet(L, False, s=None) != 0 and _qnet(L, False, t=FAKE_ODD) != 0 and _qnet(L, False, ld=202) != 0
    assert _qnet(L, True, gy=None) != 0 and _qnet(L, True, out=None) != 0
    assert "hidden=305" in (_qnet(L, False, hidden=305, ld=308), _err(L))[1]
    assert L.a3vt_qnet_input_scratch_bytes(2, 100, 305, 66, 1) == 0
    fwd, both = L.a3vt_qnet_input_scratch_bytes(16, 2324, 200, 66, 0), L.a3vt_qnet_input_scratch_bytes(16, 2324, 200, 66, 1)
    assert 0 < fwd < both


def test_adam_step_clamp_refuses_bad_arguments(L):
    ok = (FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 3, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    assert L.a3vt_adam_step_clamp(*ok, 0.0, None) != 0 and "argument check failed" in _err(L)       # the clamp must be positive
    assert L.a3vt_adam_step_clamp(*ok, -1.0, None) != 0
    assert L.a3vt_adam_step_clamp(FAKE, None, *ok[2:], 1.0, None) != 0
    assert L.a3vt_adam_step_clamp(*ok[:13], 0, 1.0, None) != 0                                       # step counts from 1
    assert L.a3vt_adam_step_clamp(*ok[:7], 0, *ok[8:], 1.0, None) == 0                               # no chunks: nothing is launched


def test_adam_grad_clamp_on_parameters_the_kernel_does_not_take():
    """CPU parameters: torch's clamp, then torch's own step — the same numbers as clamping by hand in front of ``torch.optim.Adam``."""
    from a3vt_amd.optim import Adam
    torch.manual_seed(0)
    p, q = (torch.nn.Parameter(torch.randn(7, 5)) for _ in range(2))
    q.data.copy_(p.data)
    g = 3.0 * torch.randn(7, 5)
    p.grad, q.grad = g.clone(), g.clone().clamp_(-1, 1)
    Adam([p], lr=1e-2, grad_clamp=1.0).step()
    torch.optim.Adam([q], lr=1e-2).step()
    assert torch.equal(p.grad, q.grad) and p.grad.abs().max() == 1.0 and torch.equal(p.data, q.data)
    with pytest.raises(ValueError):
        Adam([p], grad_clamp=0.0)


def test_adam_grad_clamp_host_fallback_keeps_a_nan_gradient():
    """The kernel's clamp and this one are pinned to the same rule (``torch.clamp``, test_gpu_adam.py::test_non_finite_gradients):
    +-Inf become +-c, a NaN gradient stays NaN and makes that element of the parameter and of both moments NaN."""
    from a3vt_amd.optim import Adam
    torch.manual_seed(1)
    p = torch.nn.Parameter(torch.randn(9))
    before = p.detach().clone()
    p.grad = torch.tensor([float("nan"), float("inf"), float("-inf"), 3.0, -3.0, 0.25, float("nan"), -0.5, 0.0])
    opt = Adam([p], lr=1e-2, grad_clamp=1.0)
    opt.step()
    nan = torch.tensor([True, False, False, False, False, False, True, False, False])
    assert torch.equal(torch.isnan(p.grad), nan)
    assert p.grad[~nan].tolist() == [1.0, -1.0, 1.0, -1.0, 0.25, -0.5, 0.0]
    for t in (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]):
        assert torch.equal(torch.isnan(t), nan) and bool(torch.isfinite(t[~nan]).all())
    # the first step from zero state moves a finite element by lr against its gradient's sign: +-Inf stepped as +-1
    assert torch.allclose((before - p.detach())[1:5], 1e-2 * torch.tensor([1.0, -1.0, 1.0, -1.0]), rtol=1e-5, atol=0)
