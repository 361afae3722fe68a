#!/usr/bin/env python
"""The supervised latent policy at the reference's ``t_p`` defaults — E = 3 elements, 50 actions, latent size 200, a value network
of 4 x 200 — three A/B measurements, the two forms of each ALTERNATING in one process (``tools/ab_protocol.py``, both clocks):

1. evaluation   one ``Latent_Model`` evaluation with the action choice at step 4 (four actions performed per element), from host
                observations to host integers:
                  fused:   ``Latent_Model.evaluate`` with ``fused_policy`` (``ops.latent_policy``: one launch) and one copy of E int32;
                  modules: the torch modules, then the reference's masking loop (``policies/supervised/train.py:119-128``:
                           ``values[e][act] = 1e10`` element by element over the earlier steps' device action tensors) and ``argmin``.
2. update       one policy update on 5 x E random actions, ending when the loss is on the host:
                  fused:   ``train.FusedUpdate`` (forward with stash, loss, two backward launches, one-launch Adam: five launches);
                  modules: the reference's lines on torch ops (:131-159: the Python double loop of ``all_pred_values[j, a]`` picks,
                           ``stack``, the loss, ``backward`` without ``zero_grad``, ``torch.optim.Adam.step``).
3. iteration    one whole ``Engine.train`` iteration (``reset``, five random action lists scored, one update) on an ``ActiveTouch``
                over seeded models (20 GCN layers x 300, ``--points`` surface points, a ``RecordedSampler`` over synthetic records:
                no simulator time):
                  batched:    ``batched_targets`` on (one ``env.score_candidates`` call for the five lists);
                  check_step: off (the reference's five ``check_step`` calls).

Per form: device events and the host wall clock around each call, median / p10 / p90 over ``--calls`` calls per round,
``--rounds`` rounds in turn after ``--warmup`` calls of each.  The verdict lines apply the project's rule for a knob's default:
on only if the new form's p90 lies below the old form's p10 (host wall: the forms differ in synchronisations, which only the
host clock sees) — ``FUSED_POLICY_DEFAULT`` needs it of both 1 and 2, ``BATCHED_TARGETS_DEFAULT`` of 3.

    python tools/supervised_bench.py --out profiles/supervised_step_ab.txt"""
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
ab.add_arguments(ap, calls=100, rounds=5, warmup=20, what="form (measurements 1 and 2)")
ap.add_argument("--iterations", type=int, default=8, help="timed train iterations per round and form (measurement 3)")
ap.add_argument("--iteration_warmup", type=int, default=3)
ap.add_argument("--env", type=int, default=3)
ap.add_argument("--num_actions", type=int, default=50)
ap.add_argument("--latent", type=int, default=200)
ap.add_argument("--layers", type=int, default=4)
ap.add_argument("--hidden_dim", type=int, default=200)
ap.add_argument("--taken", type=int, default=4, help="actions already performed per element (the mask of step 4)")
ap.add_argument("--points", type=int, default=30000, help="surface points and cloud size of measurement 3")
ap.add_argument("--gcn_layers", type=int, default=20)
ap.add_argument("--skip_iteration", action="store_true", help="measurements 1 and 2 only")
a = ab.parse(ap)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from a3vt_amd import optim as a3vt_optim  # noqa: E402
from a3vt_amd.pterotactyl.policies.supervised import model as sm  # noqa: E402
from a3vt_amd.pterotactyl.policies.supervised import train as st  # noqa: E402

ab.require_gpu("supervised_bench")
dev = torch.device("cuda", 0)
E, A = a.env, a.num_actions
# ab.alternate at its defaults: both clocks; every form ends with its result on the host, so the host clock stops before the
# closing synchronise.  The verdicts read the host clock (ab.report's default).
alternate, report = ab.alternate, ab.report


root = tempfile.mkdtemp(prefix="supervised_bench_")
auto_dir = os.path.join(root, "auto_config")
os.makedirs(auto_dir)
with open(os.path.join(auto_dir, "config.json"), "w") as f:
    json.dump({"encoding_size": a.latent, "check_point": auto_dir}, f)
policy_args = dict(auto_location=auto_dir + "/", num_actions=A, hidden_dim=a.hidden_dim, layers=a.layers, normalize=0, use_img=False)
g = np.random.default_rng(0)
obs = {"mask": torch.zeros(E, A), "latent": torch.from_numpy(g.standard_normal((E, a.latent)).astype(np.float32)),
       "first_latent": torch.from_numpy(g.standard_normal((E, a.latent)).astype(np.float32))}           # host tensors, as the environment's
cur_actions = []                                      # the reference's list: one device tensor of E actions per earlier step
for _ in range(a.taken):
    acts = [int(g.choice(np.where(obs["mask"][e].numpy() == 0)[0])) for e in range(E)]
    for e, act in enumerate(acts):
        obs["mask"][e, act] = 1
    cur_actions.append(torch.tensor(acts, device=dev))

torch.manual_seed(0)
fused_model = sm.Latent_Model(SimpleNamespace(fused_policy=True, **policy_args)).to(dev)
plain_model = sm.Latent_Model(SimpleNamespace(fused_policy=False, **policy_args)).to(dev)
plain_model.load_state_dict(fused_model.state_dict())
lines, result = [], {"env": E, "num_actions": A, "latent": a.latent, "layers": a.layers, "hidden_dim": a.hidden_dim, "taken": a.taken,
                     "calls": a.calls * a.rounds, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}

# ---- 1. evaluation with action choice -----------------------------------------------------------------------------------------


def evaluate_fused():
    with torch.no_grad():
        _, action = fused_model.evaluate(obs)
        return action.cpu().tolist()


def evaluate_modules():
    with torch.no_grad():
        values = plain_model(obs)
        for acts in cur_actions:                      # train.py:122-124
            for e, act in enumerate(acts):
                values[e][act] = 1e10
        return torch.argmin(values, dim=1).cpu().tolist()


chosen = (evaluate_fused(), evaluate_modules())
result["same_actions"] = chosen[0] == chosen[1]
res = alternate({"fused": evaluate_fused, "modules": evaluate_modules}, a.calls, a.rounds, a.warmup)
result["evaluation"] = res
lines.append(f"# the supervised latent policy, fused kernels vs torch ops; ms per call; {result['device']}")
lines.append(f"# E = {E}, {A} actions, latent {a.latent}, value network {a.layers} x {a.hidden_dim}, {a.taken} actions taken per element; "
             f"{a.calls * a.rounds} calls per form in {a.rounds} alternating rounds after {a.warmup} warm-up calls")
eval_wins = report(f"1. one evaluation with action choice (same actions: {result['same_actions']})", res, "fused", "modules", lines)

# ---- 2. one policy update ---------------------------------------------------------------------------------------------------------
random_actions = g.integers(0, A, (st.TRAINING_ACTIONS, E))
target = torch.from_numpy(g.standard_normal((st.TRAINING_ACTIONS, E)).astype(np.float32) * 20)
fused_model.train()
plain_model.train()
fused_update = st.FusedUpdate(fused_model, a3vt_optim.Adam(list(fused_model.parameters()), lr=0.001, weight_decay=0), accumulate=True)
plain_optimizer = torch.optim.Adam(list(plain_model.parameters()), lr=0.001, weight_decay=0)


def update_fused():
    loss, _ = fused_update(obs, random_actions, target)
    return loss.item()


def update_modules():
    all_pred_values = plain_model(obs)
    pred_values = []
    for actions in random_actions:                    # train.py:139-154 without the check_step calls
        cur_pred_values = []
        for j, act in enumerate(actions):
            cur_pred_values.append(all_pred_values[j, act])
        pred_values.append(torch.stack(cur_pred_values))
    tgt = target.cuda()
    pred_values = torch.stack(pred_values)
    loss = ((tgt - pred_values) ** 2).mean()
    loss.backward()
    plain_optimizer.step()
    return loss.item()


first = (update_fused(), update_modules())
result["first_update_loss"] = {"fused": first[0], "modules": first[1]}
res = alternate({"fused": update_fused, "modules": update_modules}, a.calls, a.rounds, a.warmup)
result["update"] = res
update_wins = report(f"2. one policy update (first losses: fused {first[0]:.6g}, modules {first[1]:.6g})", res, "fused", "modules", lines)
result["fused_policy_default"] = bool(eval_wins and update_wins and result["same_actions"])
lines.append(f"#   -> FUSED_POLICY_DEFAULT = {result['fused_policy_default']}")

# ---- 3. one whole train iteration ---------------------------------------------------------------------------------------------------
if not a.skip_iteration:
    from a3vt_amd.pterotactyl.policies import environment, recorded
    from a3vt_amd.pterotactyl.reconstruction.autoencoder import model as auto_model
    from a3vt_amd.pterotactyl.reconstruction.touch import model as touch_model
    from a3vt_amd.pterotactyl.reconstruction.vision import model as vision_model
    from a3vt_amd.pterotactyl.utility import utils
    from a3vt_amd.synthetic import gt_cloud
    from env_bench import synthetic_records, write_checkpoint   # (tools/ is this script's directory)

    config = dict(use_img=False, use_touch=True, finger=True, num_grasps=5, num_GCN_layers=a.gcn_layers, hidden_GCN_size=300, cut=0.33)
    info, verts = utils.load_mesh_vision(SimpleNamespace(**config), "vision_charts")
    torch.manual_seed(0)
    deform = vision_model.Deformation(info, verts, SimpleNamespace(**config))
    with torch.no_grad():
        for gcn in (deform.mesh_deform_1, deform.mesh_deform_2):
            gcn.layers[-1].weight.mul_(0.02)
            gcn.layers[-1].bias.mul_(0.02)
    auto_config = dict(config, num_GCN_layers=3, encoding_size=a.latent)
    torch.manual_seed(1)
    auto = auto_model.AutoEncoder(info, verts, SimpleNamespace(**auto_config), only_encode=True)
    torch.manual_seed(0)
    locations = {"vision_location": write_checkpoint(os.path.join(root, "vision"), config, deform),
                 "touch_location": write_checkpoint(os.path.join(root, "touch"), {}, touch_model.Encoder()),
                 "auto_location": write_checkpoint(os.path.join(root, "auto"), auto_config, auto)}
    args = SimpleNamespace(seed=0, eval=False, pretrained_recon=False, use_img=False, use_touch=True, finger=True, num_grasps=5,
                           use_latent=True, use_recon=False, num_actions=A, budget=5, env_batch_size=E, number_points=a.points,
                           loss_coeff=9000.0, exp_type="bench", exp_id="supervised", pretrained=False, visualize=False,
                           hidden_dim=a.hidden_dim, layers=a.layers, normalize=0, lr=0.001, patience=25, epoch=1, train_steps=1,
                           fused_policy=result["fused_policy_default"], batched_targets=True, **locations)
    objects = [f"object{e}" for e in range(E)]

    class Environment(environment.ActiveTouch):
        def get_loaders(self):                                       # no dataset: the batch below is synthetic
            pass

    os.chdir(root)                                                   # (the engine makes results/ and experiments/ where it runs)
    engine = st.Engine(args, sampler=recorded.RecordedSampler(synthetic_records(objects, A, 1)))
    engine.env = Environment(args, sampler=engine.sampler)
    gen = torch.Generator().manual_seed(2)
    engine.env.score_samples = (torch.randint(0, info["faces"].shape[0], (3, E, a.points), generator=gen).to(torch.int32),
                                torch.rand(3, E, a.points, generator=gen), torch.rand(3, E, a.points, generator=gen))
    batch = {"names": ["/data/object_info/" + o for o in objects], "gt_points": gt_cloud(E, a.points, 3), "img": torch.zeros(E, 1)}
    torch.manual_seed(0)
    engine.models = engine.make_models()
    engine.step = 0
    engine.start_step()
    targets = {}

    def iteration(batched):
        def run():
            args.batched_targets = batched
            np.random.seed(5)                                         # the same five action lists for both forms
            engine.train([batch])                                     # (ends with the loss on the host)
            targets[batched] = engine.last["target"].clone()
        return run

    res = alternate({"batched": iteration(True), "check_step": iteration(False)}, a.iterations, a.rounds, a.iteration_warmup)
    result["iteration"] = res
    diff = float((targets[True] - targets[False]).abs().max() / targets[False].abs().max())
    result["target_rel_diff"] = diff
    lines.append(f"#   (measurement 3: {a.iterations * a.rounds} iterations per form after {a.iteration_warmup} warm-up, {a.points} points, "
                 f"{a.gcn_layers} GCN layers, finger charts, fused_policy={args.fused_policy}; targets of the two forms differ by {diff:.2e} relative)")
    result["batched_targets_default"] = bool(report("3. one whole train iteration (reset, five action lists scored, one update)", res,
                                                    "batched", "check_step", lines))
    lines.append(f"#   -> BATCHED_TARGETS_DEFAULT = {result['batched_targets_default']}")

lines.append(json.dumps(result))
ab.emit(lines, a.out)
if not result["same_actions"]:
    raise SystemExit(f"supervised_bench: the two forms chose different actions: {chosen}")
