"""Shared by the DDQN tests and ``golden/make_golden_ddqn.py``: the argument sets of the three cases of ``g16_ddqn_update.npz``
and how a case's transitions are rebuilt from what the fixture stores."""
import json
import os

import numpy as np
import torch

from helpers import make_args

N_VISION = 1824
CASES = ("a", "b", "c")


def case_args(case, auto_location=None, **kw):
    """(a) graph model, rewards / first_score; (b) the same with raw rewards of order 5-10 (the clamp bites); (c) latent model."""
    d = dict(use_touch=True, num_grasps=5, finger=True, layers=3, hidden_dim=200, num_actions=50, mem_capacity=8, burn_in=0,
             train_batch_size=4, pretrained=False, lr=1e-3, gamma=0.9, budget=5, use_recon=case != "c", use_latent=case == "c",
             normalization="none" if case == "b" else "first", auto_location=auto_location, epsilon_end=0.05, epsilon_decay=0.9)
    if case == "c":
        d.update(hidden_dim=100)
    d.update(kw)
    return make_args(**d)


def write_auto_config(directory, encoding_size=200):
    """The ``config.json`` the latent model and the replay memory read their latent size from."""
    with open(os.path.join(directory, "config.json"), "w") as f:
        json.dump({"encoding_size": encoding_size, "check_point": directory}, f)
    return directory


def next_mesh(mesh, touch_n):
    """The next-state meshes of cases (a) / (b): the vision charts grown by 1 % (one fp32 product per element, the same bits
    wherever it runs), the touch-chart rows as stored."""
    out = np.array(mesh, dtype=np.float32, copy=True)
    out[:, :N_VISION, :3] = out[:, :N_VISION, :3] * np.float32(1.01)
    out[:, N_VISION:] = touch_n
    return out


def transitions(z, case):
    """(action, observation, next_observation, reward) of a case as ``ReplayMemory.push`` takes them."""
    t = lambda k: torch.from_numpy(np.asarray(z[k]))  # noqa: E731
    obs = {"score": t("score"), "first_score": t("first_score"), "mask": t("mask")}
    nxt = {"score": t("score_n"), "mask": t("mask_n")}
    if case == "c":
        obs.update(latent=t("latent"), first_latent=t("first_latent"))
        nxt.update(latent=t("latent_n"))
    else:
        obs["mesh"] = t("mesh")
        nxt["mesh"] = torch.from_numpy(next_mesh(z["mesh"], z["mesh_n_touch"]))
    return z["actions"], obs, nxt, t("rewards_b" if case == "b" else "rewards")


def perturbed_copy(learner, adj_info=None):
    """The target network of the cases: a second learner with the first one's weights (as the reference trainer builds it,
    DDQN/train.py:49-51) whose parameters then move by 0.01 * randn under seed 1 (CPU generator, parameter order)."""
    target = type(learner)(learner.args, adj_info, None)
    target.load_state_dict(learner.state_dict())
    torch.manual_seed(1)
    with torch.no_grad():
        for p in target.parameters():
            p.add_(0.01 * torch.randn(p.shape))
    return target


# ---- layer 0 of the graph model restated from its formulas (any dtype, any device): what the fused kernel is compared with --------
NERF_FREQS = [np.pi if i == 0 else np.pi * 2 * i for i in range(10)]


def layer0_params(net):
    """The tensors layer 0 of a ``Graph_Model`` reads, by the names ``layer0_restated`` uses."""
    pe = net.positional_embedding.model
    return {"w1": pe[0].weight, "b1": pe[0].bias, "w2": pe[2].weight, "b2": pe[2].bias, "w3": pe[4].weight, "b3": pe[4].bias,
            "table": net.mask_embedding.model[0].weight, "w0": net.layers[0].weight, "b0": net.layers[0].bias}


def layer0_restated(p, mesh, action, adj, cut_len):
    """relu(layer0([action | PE(xyz) | table[token]])) in the dtype of ``p``: nerf embedding with the reference's ten frequencies
    (each rounded to fp32 first, as every fp32 implementation has them), 63 -> 25 -> 50 -> 100 with two ReLUs, the 300 x h
    product, the first ``cut_len`` columns aggregated with the dense ``adj`` + bias, the rest passed through, ReLU."""
    dt = p["w0"].dtype
    xyz, tok = mesh[..., :3].to(dt), mesh[..., 3].long()
    f = torch.tensor(NERF_FREQS, dtype=torch.float32, device=xyz.device).to(dt)
    ang = xyz[..., None, :] * f[:, None]                                                     # (B, N, 10, 3)
    e = torch.cat((torch.stack((torch.sin(ang), torch.cos(ang)), dim=-2).flatten(-3), xyz), dim=-1)     # (B, N, 63)
    h1 = torch.relu(e @ p["w1"].t() + p["b1"])
    h2 = torch.relu(h1 @ p["w2"].t() + p["b2"])
    pos = h2 @ p["w3"].t() + p["b3"]
    feats = torch.cat((action[:, None, :].expand(-1, mesh.shape[1], -1), pos, p["table"][tok]), dim=-1)
    z = feats @ p["w0"].reshape(300, -1)
    z = torch.cat((adj @ z[..., :cut_len] + p["b0"][:cut_len], z[..., cut_len:]), dim=-1)
    return torch.relu(z)


def random_gy(shape, seed=1):
    """The upstream gradient of the fp64 comparisons: plain randn (fp64).  ``test_ddqn_host.py`` checks on the CPU that the unfused
    fp32 formulation stays inside ``assert_grad_close``'s caps against fp64 under it, so no smoother one is needed."""
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def tp_dense_adjacency():
    """The row-normalised dense adjacency of t_p (atlas + 5 finger charts, N = 1949) built on the host."""
    from a3vt_amd import mesh as amesh
    v, f = amesh.load_asset("vision_charts")
    sv, sf = amesh.load_asset("touch_chart")
    r, c, n, _ = amesh.fused_pairs(v, f, sf, 5, True, sv.shape[0])
    return torch.from_numpy(amesh.CSRAdjacency.from_pairs(r, c, n).to_dense())


def layer0_run(p, mesh, action, adj, cut_len, gy, dtype):
    """Forward + backward of the restated layer in ``dtype`` on detached copies -> (y, {name: gradient})."""
    q = {k: t.detach().to(dtype).requires_grad_(True) for k, t in p.items()}
    act = action.detach().to(dtype).requires_grad_(True)
    y = layer0_restated(q, mesh, act, adj.to(dtype), cut_len)
    y.backward(gy.to(dtype))
    return y.detach(), {**{k: t.grad for k, t in q.items()}, "action": act.grad}


def random_obs(batch, n_vert, seed, empty_sample=None):
    """Observations as the environment hands them over: perturbed vision charts with token 3, touch-chart rows with tokens 0..2
    (all four tokens present), ``empty_sample``: a sample whose touch slots are all empty (token 0, zero positions)."""
    from a3vt_amd import mesh as amesh
    g = torch.Generator().manual_seed(seed)
    mesh = torch.zeros(batch, n_vert, 4)
    if n_vert > N_VISION:
        verts = torch.from_numpy(amesh.load_asset("vision_charts")[0])
        mesh[:, :N_VISION, :3] = verts + 0.01 * torch.randn(batch, N_VISION, 3, generator=g)
        mesh[:, :N_VISION, 3] = 3
        nt = n_vert - N_VISION
        mesh[:, N_VISION:, :3] = (torch.rand(batch, nt, 3, generator=g) - 0.5) * 0.3
        mesh[:, N_VISION:, 3] = torch.randint(0, 3, (batch, nt), generator=g).float()
        mesh[:, N_VISION:N_VISION + 3, 3] = torch.tensor([0.0, 1.0, 2.0])
    else:
        mesh[..., :3] = (torch.rand(batch, n_vert, 3, generator=g) - 0.5) * 0.3
        mesh[..., 3] = torch.randint(0, 4, (batch, n_vert), generator=g).float()
        mesh[:, :4, 3] = torch.tensor([0.0, 1.0, 2.0, 3.0])
    if empty_sample is not None and n_vert > N_VISION:
        mesh[empty_sample, N_VISION:] = 0
    mask = (torch.rand(batch, 50, generator=g) < 0.1).float()
    return {"mesh": mesh, "mask": mask}
