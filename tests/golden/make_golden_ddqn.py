#!/usr/bin/env python
"""Generate ``g16_ddqn_update.npz`` by running the REAL reference's DDQN learner and replay memory on the CPU
(``python tests/golden/make_golden_ddqn.py``, build container only; see ``make_golden.py`` and ``oracle.ref_shim``).

Three cases, each ONE ``update_parameters`` from seed 0 (``tests/ddqn_util.py`` holds the argument sets): weights from
``torch.manual_seed(0)``, the target net a copy perturbed by ``0.01 * randn`` under seed 1, ``np.random.seed(5)`` in front of
the update.  6 transitions are pushed in one call (masks with 0..4 earlier touches: done and not-done rows), 4 are sampled.
  (a) graph model on t_p (3 layers, 200 wide), rewards / first_score: every gradient stays inside the clamp
  (b) the same model, raw rewards of order 5-10: the clamp bites on part of the gradients (asserted below)
  (c) latent model (encoding_size 200 from a config.json in a temporary directory)
Per case (keys prefixed ``a:`` / ``b:`` / ``c:``): checksum of the initial weights, sampled indices, loss, q_cur / best_next /
target (recomputed with the reference's own forward calls), post-clamp gradients of selected tensors.  Shared: the pushed
observations, and ``sampler_actions`` — the reference ``random_sampler`` under ``random.seed(7)`` on the pushed masks, 3 rounds."""
import importlib
import os
import random
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import OBJ, ref, save, state_checksum  # noqa: E402  (installs the import shim; defines no fixture when imported)
import ddqn_util as du  # noqa: E402

GRAPH_GRADS = ("layers.0.bias", "layers.1.weight", "layers.2.weight", "layers.2.bias", "action_model.2.0.bias",
               "positional_embedding.model.4.bias", "mask_embedding.model.0.weight", "positional_embedding.model.0.weight",
               "positional_embedding.model.2.weight")
LATENT_GRADS = ("model.1.0.weight", "model.2.0.weight", "model.2.0.bias", "action_model.2.0.bias", "action_model.0.0.bias")


def observations():
    g = torch.Generator().manual_seed(41)
    n = 6
    info, verts = ref.utils.load_mesh_vision(du.case_args("a"), OBJ)
    nv = info["adj"].shape[0]
    mesh = torch.zeros(n, nv, 4)
    mesh[:, :du.N_VISION, :3] = verts + 0.01 * torch.randn(n, du.N_VISION, 3, generator=g)
    mesh[:, :du.N_VISION, 3] = 3
    touch = lambda: torch.cat(((torch.rand(n, nv - du.N_VISION, 3, generator=g) - 0.5) * 0.3,  # noqa: E731
                               torch.randint(0, 3, (n, nv - du.N_VISION, 1), generator=g).float()), dim=-1)
    mesh[:, du.N_VISION:] = touch()
    mesh[0, du.N_VISION:, 3] = 0          # one sample whose touch slots are all empty
    touch_n = touch()
    touches = [0, 1, 2, 3, 4, 4]          # earlier touches per transition: budget 5 -> the last two rows are done
    mask = torch.zeros(n, 50)
    for i, k in enumerate(touches):
        mask[i, torch.randperm(50, generator=g)[:k]] = 1
    actions = np.array([int(torch.nonzero(mask[i] == 0)[int(torch.randint(0, 50 - k, (1,), generator=g))]) for i, k in enumerate(touches)])
    mask_n = mask.clone()
    mask_n[torch.arange(n), torch.from_numpy(actions)] = 1
    first = 1.0 + torch.rand(n, generator=g)
    score = first * (0.5 + 0.5 * torch.rand(n, generator=g))
    rewards = score * 0.3 * torch.rand(n, generator=g)
    return {"mesh": mesh.numpy(), "mesh_n_touch": touch_n.numpy(), "mask": mask.numpy(), "mask_n": mask_n.numpy(), "actions": actions,
            "score": score.numpy(), "score_n": (score - rewards).numpy(), "first_score": first.numpy(), "rewards": rewards.numpy(),
            "rewards_b": (5.0 + 5.0 * torch.rand(n, generator=g)).numpy(),
            "latent": torch.randn(n, 200, generator=g).numpy(), "latent_n": torch.randn(n, 200, generator=g).numpy(),
            "first_latent": torch.randn(n, 200, generator=g).numpy()}, info


def run_case(case, z, info, auto_location):
    ddqn = importlib.import_module("pterotactyl.policies.DDQN.ddqn")
    replay = importlib.import_module("pterotactyl.policies.replay")
    args = du.case_args(case, auto_location)
    torch.manual_seed(0)
    memory = replay.ReplayMemory(args)
    learner = ddqn.DDQN(args, info, memory)
    out = {"weight_sha256": state_checksum(learner.model.state_dict())}
    target = du.perturbed_copy(learner, info)
    learner.add_experience(*du.transitions(z, case))
    np.random.seed(5)
    batch = memory.sample()
    with torch.no_grad():     # the reference's own forward calls, ddqn.py:101-113, before the update moves the weights
        q_all = learner.forward(batch, penalize=False)
        out["q_cur"] = q_all.gather(1, batch["actions"].unsqueeze(1).long()).squeeze(1).numpy()
        out["q_all"] = q_all.numpy()
        best = learner.forward(batch, next=True).max(1)[1]
        nxt = target.forward(batch, next=True, penalize=False)
        not_done = batch["mask"].sum(dim=1) < args.budget - 1
        rewards = batch["rewards"] / batch["first_score"] if args.normalization == "first" else batch["rewards"]
        out["best_next"] = best.numpy().astype(np.int32)
        out["target"] = (args.gamma * torch.where(not_done, nxt[torch.arange(4), best], torch.zeros(4)) + rewards).numpy()
        out["not_done"] = not_done.numpy()
    np.random.seed(5)
    state = np.random.get_state()
    out["indices"] = np.random.choice(min(memory.count_seen, args.mem_capacity), args.train_batch_size)
    np.random.set_state(state)
    out["loss"] = np.float64(learner.update_parameters(target))
    params = dict(learner.model.named_parameters())
    names = LATENT_GRADS if case == "c" else GRAPH_GRADS
    for k in names:
        out["g:" + k] = params[k].grad.numpy()
    if case == "c":
        out["g:model.0.0.weight"] = params["model.0.0.weight"].grad.numpy()[::3, ::5]
    else:
        out["g:layers.0.weight"] = params["layers.0.weight"].grad.numpy()[..., ::3, ::5]
        share = {k: float((p.grad.abs() >= 1.0).float().mean()) for k, p in params.items()}
        print(f"case {case}: loss {out['loss']:.4f}  max|grad| {max(float(p.grad.abs().max()) for p in params.values()):.3f}  "
              f"clamped share layers.2.weight {share['layers.2.weight']:.3f}  not_done {out['not_done'].tolist()}")
        if case == "a":
            assert max(share.values()) == 0.0, "case (a) is the clamp-inactive baseline"
        else:
            assert 0.0 < share["layers.2.weight"] < 1.0, "case (b) must clamp part of layers.2.weight"
    assert abs(float(((torch.from_numpy(out["q_cur"]) - torch.from_numpy(out["target"])) ** 2).mean()) - out["loss"]) < 1e-5 * max(1.0, out["loss"])
    return {f"{case}:{k}": v for k, v in out.items()}


def main():
    baselines = importlib.import_module("pterotactyl.policies.baselines.baselines")
    z, info = observations()
    out = dict(z)
    with tempfile.TemporaryDirectory() as auto:
        du.write_auto_config(auto)
        for case in du.CASES:
            out.update(run_case(case, z, info, auto))
    random.seed(7)
    sampler = baselines.random_sampler(du.case_args("a"))
    out["sampler_actions"] = np.stack([sampler.get_action(z["mask"]) for _ in range(3)])
    save("g16_ddqn_update.npz", **out)


if __name__ == "__main__":
    main()
