#!/usr/bin/env python
"""The DDQN learner over auto-encoder latents (``Latent_Model``) — ``fused_q_latent`` on against off, the two forms ALTERNATING in
one process (``tools/ab_protocol.py``, both clocks), at two sizes: the reference's defaults (4 x 200) and the published
``l_*`` checkpoints' (5 x 300); batch 16, 50 actions, latent 200, a host replay memory of 300 transitions, ``gamma`` 0.9,
rewards / first_score.

1. update       one ``DDQN.update_parameters`` from the replay draw to the loss on the host:
                  fused:   ``ops.ddqn_latent_update`` (three launches: the three forwards side by side, TD and deltas, gradients
                           and loss) into gradient tensors the learner owns, then the one-launch ``optim.Adam(grad_clamp=1)``;
                  modules: the knob-off path, unchanged by the knob's existence — three evaluations of the torch modules, ``ops.ddqn_td``
                           (one launch), autograd's backward, the same one-launch Adam.
2. get_action   one greedy ``DDQN.get_action`` at E = 3, from host observations to host integers:
                  fused:   ``ops.ddqn_latent_q`` (one launch: values and the penalised argmax) and one copy of E int32;
                  modules: the torch modules, the ``-1e10`` masking op, ``argmax`` and the copy.

Per form: device events and the host wall clock around each call, median / p10 / p90 over ``--calls`` calls per round, ``--rounds``
rounds in turn after ``--warmup`` calls of each; the fused update's launches from the library's own counters.  The verdict applies
the project's rule for a knob's default: ``FUSED_Q_LATENT_DEFAULT`` is on only if the fused update's p90 lies below the modules'
p10 (host wall: the forms differ in launches and host work, which only the host clock sees) at BOTH sizes.

    python tools/ddqn_latent_bench.py --out profiles/ddqn_latent_ab.txt"""
import argparse
import json
import os
import sys
import tempfile
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ab_protocol as ab  # noqa: E402  (tools/ is this script's directory)

ap = argparse.ArgumentParser()
ab.add_arguments(ap, calls=100, rounds=5, warmup=20)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--env", type=int, default=3)
ap.add_argument("--num_actions", type=int, default=50)
ap.add_argument("--latent", type=int, default=200)
ap.add_argument("--sizes", type=str, default="4x200,5x300", help="layers x hidden_dim of the Q network, comma-separated")
a = ab.parse(ap)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from a3vt_amd import ops  # noqa: E402
from a3vt_amd.pterotactyl.policies import replay  # noqa: E402
from a3vt_amd.pterotactyl.policies.DDQN import ddqn  # noqa: E402

ab.require_gpu("ddqn_latent_bench")
dev = torch.device("cuda", 0)
E, A, B = a.env, a.num_actions, a.batch


def alternate(forms):
    """Both clocks; the forms end with their result on the host, so the host clock stops before the closing synchronise."""
    return ab.alternate(forms, a.calls, a.rounds, a.warmup)


def report(title, res, lines):
    return ab.report(title, res, "fused", "modules", lines, clock="host")


root = tempfile.mkdtemp(prefix="ddqn_latent_bench_")
with open(os.path.join(root, "config.json"), "w") as f:
    json.dump({"encoding_size": a.latent, "check_point": root}, f)


def learner_pair(layers, hidden, fused):
    args = SimpleNamespace(auto_location=root + "/", num_actions=A, hidden_dim=hidden, layers=layers, use_latent=True, use_recon=False,
                           use_img=False, finger=True, pretrained=False, lr=0.0003, gamma=0.9, budget=5, normalization="first",
                           mem_capacity=300, train_batch_size=B, burn_in=20, fused_q_latent=fused)
    torch.manual_seed(0)
    memory = replay.ReplayMemory(args)                                       # on the host, as the reference's
    learner = ddqn.DDQN(args, None, memory)
    target = ddqn.DDQN(args, None, None)
    target.load_state_dict(learner.state_dict())
    torch.manual_seed(1)
    with torch.no_grad():
        for p in target.parameters():
            p.add_(0.01 * torch.randn(p.shape))
    g = torch.Generator().manual_seed(2)
    for _ in range(args.mem_capacity // E):                                  # episodes of random touches fill the memory
        mask = torch.zeros(E, A)
        for e in range(E):
            mask[e, torch.randperm(A, generator=g)[:int(torch.randint(0, 5, (1,), generator=g))]] = 1
        action = np.array([int(torch.nonzero(mask[e] == 0)[int(torch.randint(0, int((mask[e] == 0).sum()), (1,), generator=g))]) for e in range(E)])
        nxt = mask.clone()
        nxt[torch.arange(E), torch.from_numpy(action)] = 1
        first = 1.0 + torch.rand(E, generator=g)
        score = first * (0.5 + 0.5 * torch.rand(E, generator=g))
        reward = score * 0.3 * torch.rand(E, generator=g)
        obs = {"mask": mask, "score": score, "first_score": first, "latent": torch.randn(E, a.latent, generator=g),
               "first_latent": torch.randn(E, a.latent, generator=g)}
        learner.add_experience(action, obs, {"mask": nxt, "score": score - reward, "latent": torch.randn(E, a.latent, generator=g)}, reward)
    return learner.to(dev), target.to(dev).eval(), obs


lines, result = [], {"batch": B, "env": E, "num_actions": A, "latent": a.latent, "calls": a.calls * a.rounds, "warmup": a.warmup,
                     "device": torch.cuda.get_device_name(0), "sizes": {}}
lines.append(f"# DDQN's latent Q-network, fused_q_latent on vs off (the torch-module path); ms per call; {result['device']}")
lines.append(f"# batch {B}, {A} actions, latent {a.latent}, host replay of 300; get_action at E = {E}; {a.calls * a.rounds} calls per form in "
             f"{a.rounds} alternating rounds after {a.warmup} warm-up calls")
verdicts = []
for size in a.sizes.split(","):
    layers, hidden = (int(x) for x in size.split("x"))
    fused, fused_target, obs = learner_pair(layers, hidden, True)
    plain, plain_target, _ = learner_pair(layers, hidden, False)
    assert fused.model.fused_q_latent and not plain.model.fused_q_latent
    one = {}

    def update(learner, target):
        def run():
            return learner.update_parameters(target)
        return run

    def choose(learner):
        def run():
            return learner.get_action(obs, eps_threshold=-1)
        return run

    np.random.seed(3)
    first_fused = update(fused, fused_target)()
    np.random.seed(3)
    first_plain = update(plain, plain_target)()
    ops.ddqn_latent_launches(reset=True)
    steps = fused.optimizer.library_steps
    update(fused, fused_target)()
    launches = ops.ddqn_latent_launches()["update"] + (fused.optimizer.library_steps - steps)
    same = bool(np.array_equal(choose(fused)(), choose(plain)()))             # (after one equal-seeded update each: nearly equal weights)
    one["first_update_loss"] = {"fused": first_fused, "modules": first_plain}
    one["fused_launches_per_update"] = launches
    one["same_actions"] = same
    lines.append(f"# ---- Q network {layers} x {hidden} ----")
    one["update"] = alternate({"fused": update(fused, fused_target), "modules": update(plain, plain_target)})
    wins = report(f"1. one update_parameters (first losses: fused {first_fused:.6g}, modules {first_plain:.6g}; fused launches per update, "
                  f"Adam included: {launches})", one["update"], lines)
    one["get_action"] = alternate({"fused": choose(fused), "modules": choose(plain)})
    report(f"2. one greedy get_action at E = {E} (same actions: {same})", one["get_action"], lines)
    verdicts.append(wins)
    result["sizes"][size] = one
result["fused_q_latent_default"] = bool(all(verdicts))
lines.append(f"# -> FUSED_Q_LATENT_DEFAULT = {result['fused_q_latent_default']} (the fused update's p90 below the modules' p10 at every size: {verdicts})")
lines.append(json.dumps(result))
ab.emit(lines, a.out)
