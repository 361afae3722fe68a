#!/usr/bin/env python
"""Generate ``g18_active_touch.npz`` by running the REAL reference's ``ActiveTouch`` (``policies/environment.py``) on the CPU
(``python tests/golden/make_golden_env.py``, build container only; see ``make_golden.py`` and ``oracle.ref_shim``).

How the reference is set up (recipe shared with the tests: ``tests/env_util.py``):
* the simulator modules it imports (``pterotactyl.simulator.scene.sampler``, ``...physics.grasping``) are stubs put into
  ``sys.modules``; the stub ``Sampler`` replays the seeded records of ``env_util.records``;
* ``get_loaders`` is a no-op (no dataset);
* ``setup_recon`` loads ``config.json`` + ``model`` from temporary directories written from seeded constructions of the
  reference's own ``Encoder`` (BatchNorm from ``touch_util.seed_batchnorm``), ``Deformation`` and ``AutoEncoder``;
* ``utils.chamfer_distance`` is the injected-sample form the other fixtures use (``make_golden.ref_chamfer_injected``).

Two cases (``env_util.CASES``; E = 2, 3 GCN layers x 300, 700 surface points, 900-point clouds, loss_coeff 9000, 5 grasps):
  a  finger, no latent, 4 actions, budget 2, full search:                      reset, best_step x 2
  b  four fingers, latent (3 layers, 200 wide), 6 actions, budget 3, greedy_checks 3, random.seed(0): reset, best_step x 2, step

Stored per case ``<c>``: (weights and images are NOT stored: the tests rebuild them from the seeds and check the checksums)
  <c>:sha:<kind>                 checksum of the touch (non-BatchNorm tensors) / vision / auto state dict
  <c>:status                     (E, num_actions, 4) int8 codes into env_util.STATUS
  <c>:gt, <c>:face_idx|u|v       ground-truth clouds, injected surface draws (3, E, 700)
  <c>:<i>:score|mask|reward|done|latent|actions   the reference's outputs of call i (0 = reset)
  <c>:<i>:mesh_sub               obs["mesh"][:, ::16] of call i;  <c>:mesh = obs["mesh"] of the final call
  <c>:<i>:table, <c>:<i>:cands   per best_step: the (K, E) candidate scores and the (K, E) candidate actions
  bn:<key>                       every BatchNorm tensor of the touch encoder (shared by the cases)
At every greedy decision the relative gap between the lowest and the second-lowest eligible score of each element must exceed
1e-2 (one hundred times the tests' score tolerance); asserted, and the smallest gap printed."""
import contextlib
import importlib
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import injected, ref, ref_chamfer_injected, save, state_checksum  # noqa: E402  (installs the import shim)
import env_util as eu  # noqa: E402
import touch_util as tu  # noqa: E402

MIN_GAP = 1e-2


class StubSampler:
    """Replays ``env_util.records`` with the reference sampler's interface (``simulator/scene/sampler.py``)."""
    records = None
    log = None

    def __init__(self, grasp, bs=1, vision=False):
        self.bs = bs

    def load_objects(self, batch, from_dataset=True, scale=3.1):
        self.ids = [os.path.basename(n) for n in batch]

    def sample(self, actions, touch_point_cloud=False):
        StubSampler.log.append([int(a) for a in actions])
        recs = [StubSampler.records[(o, int(a))] for o, a in zip(self.ids, actions)]
        return {"touch_status": [list(r["status"]) for r in recs], "touch_signal": torch.stack([r["touch"] for r in recs]),
                "finger_transfrom_pos": torch.stack([r["pos"] for r in recs]),
                "finger_transform_rot_M": torch.stack([r["rot"] for r in recs])}

    def disconnect(self):
        pass


def install_simulator_stubs():
    for name in ("pterotactyl.simulator", "pterotactyl.simulator.scene", "pterotactyl.simulator.physics"):
        if name not in sys.modules:
            mod = types.ModuleType(name)
            mod.__path__ = []
            sys.modules[name] = mod
    s = types.ModuleType("pterotactyl.simulator.scene.sampler")
    s.Sampler = StubSampler
    g = types.ModuleType("pterotactyl.simulator.physics.grasping")
    g.Agnostic_Grasp = object
    sys.modules[s.__name__], sys.modules[g.__name__] = s, g
    sys.modules["pterotactyl.simulator.scene"].sampler = s
    sys.modules["pterotactyl.simulator.physics"].grasping = g


@contextlib.contextmanager
def workdir(models):
    """A temporary working directory with ``env_util.write_models``' checkpoints in it -> (root, locations)."""
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as root:
        os.chdir(root)
        try:
            yield root, eu.write_models(root, models)
        finally:
            os.chdir(cwd)


@contextlib.contextmanager
def reference_setup(case, tables=None, records=None):
    """The opening the generators of the policy fixtures (g19 - g22) share, in the order that fixes the key order of their
    files: the simulator stubs and ``get_loaders`` a no-op; the reference's seeded models of ``env_util``'s ``case``; ``out`` with
    the ``bn:`` and ``sha:`` entries, ``status:<batch>`` of ``tables`` and the injected draws ``face_idx|u|v``; ``records`` for
    the ``StubSampler``; ``utils.chamfer_distance`` on those draws (put back on leaving).  Yields a namespace: ``env_mod``
    (``policies.environment``), ``models``, ``out``, ``samples`` and ``workdir``, which enters a fresh temporary working
    directory with the models' checkpoints -> (root, locations); a generator that re-seeds takes one per attempt, so that no
    attempt finds the files of the one before."""
    install_simulator_stubs()
    env_mod = importlib.import_module("pterotactyl.policies.environment")
    env_mod.ActiveTouch.get_loaders = lambda self: None
    tm = importlib.import_module("pterotactyl.reconstruction.touch.model")
    am = importlib.import_module("pterotactyl.reconstruction.autoencoder.model")
    models = eu.build_models(case, tm, ref.model, am, ref.utils, os.path.join(ref.objects_dir, "vision_charts.obj"))
    out = {"pytorch3d_restated": np.bool_(True)}
    enc = models["touch"][1]
    for k, v in enc.state_dict().items():
        if tu.is_bn_key(k):
            out["bn:" + k] = v.numpy().copy()
    out["sha:touch"] = state_checksum(tu.non_bn_state(enc.state_dict()))
    out["sha:vision"] = state_checksum(models["vision"][1].state_dict())
    out["sha:auto"] = state_checksum(models["auto"][1].state_dict())
    for name, t in (tables or {}).items():
        out["status:" + name] = t
    StubSampler.records, StubSampler.log = records, []
    faces = models["vision"][1].adj_info["faces"]
    samples = injected(eu.E, faces.shape[0], 700, eu.CASES[case]["sample_seed"])
    out.update({"face_idx": torch.stack([s[0] for s in samples]).numpy().astype(np.int16),
                "u": torch.stack([s[1] for s in samples]).numpy(), "v": torch.stack([s[2] for s in samples]).numpy()})
    chamfer = ref.utils.chamfer_distance
    ref.utils.chamfer_distance = lambda verts, f, g, num=1000, repeat=3: ref_chamfer_injected(verts, f, g, samples)
    try:
        yield types.SimpleNamespace(env_mod=env_mod, models=models, out=out, samples=samples, workdir=lambda: workdir(models))
    finally:
        ref.utils.chamfer_distance = chamfer


def gap_of(scores, eligible):
    s = np.sort(np.asarray(scores, dtype=np.float64)[eligible])
    return np.inf if len(s) < 2 else (s[1] - s[0]) / s[0]


def run_case(case, env_mod, out):
    c = eu.CASES[case]
    tm = importlib.import_module("pterotactyl.reconstruction.touch.model")
    am = importlib.import_module("pterotactyl.reconstruction.autoencoder.model")
    models = eu.build_models(case, tm, ref.model, am, ref.utils, os.path.join(ref.objects_dir, "vision_charts.obj"))
    enc = models["touch"][1]
    for k, v in enc.state_dict().items():
        if tu.is_bn_key(k):
            out["bn:" + k] = v.numpy().copy()
    out[f"{case}:sha:touch"] = state_checksum(tu.non_bn_state(enc.state_dict()))
    out[f"{case}:sha:vision"] = state_checksum(models["vision"][1].state_dict())
    if "auto" in models:
        out[f"{case}:sha:auto"] = state_checksum(models["auto"][1].state_dict())
    table = eu.case_table(case)
    StubSampler.records, StubSampler.log = eu.case_records(case, table), []
    gt = eu.clouds(c["cloud_seed"])
    faces = models["vision"][1].adj_info["faces"]
    samples = injected(eu.E, faces.shape[0], 700, c["sample_seed"])
    out.update({f"{case}:status": table, f"{case}:gt": gt.numpy(),
                f"{case}:face_idx": torch.stack([s[0] for s in samples]).numpy().astype(np.int16),
                f"{case}:u": torch.stack([s[1] for s in samples]).numpy(), f"{case}:v": torch.stack([s[2] for s in samples]).numpy()})
    ref.utils.chamfer_distance = lambda verts, f, g, num=1000, repeat=3: ref_chamfer_injected(verts, f, g, samples)
    smallest = np.inf
    with tempfile.TemporaryDirectory() as root:
        args = eu.env_args(case, **eu.write_models(root, models))
        env = env_mod.ActiveTouch(args)
        scored = []
        inner = env.compute_obs

        def logged(actions=None):
            obs = inner(actions)
            scored.append(obs["score"].numpy().copy())
            return obs

        env.compute_obs = logged
        random.seed(0)
        for i, call in enumerate(c["calls"]):
            del scored[:], StubSampler.log[:]
            reward = done = actions = None
            if call == "reset":
                obs = env.reset(eu.batch_of(gt))
            elif call == "best":
                taken = env.current_data["mask"].numpy().copy()
                actions, obs, reward, done = env.best_step(greedy_checks=c["greedy_checks"])
                tab, cands = np.stack(scored[:-1]), np.array(StubSampler.log[:-1])       # the last call of each is step()'s
                out[f"{case}:{i}:table"], out[f"{case}:{i}:cands"] = tab, cands.astype(np.int64)
                for e in range(eu.E):
                    ok = (taken[e][cands[:, e]] == 0) if c["greedy_checks"] is None else np.ones(len(cands), bool)
                    smallest = min(smallest, gap_of(tab[:, e], ok))
            else:
                free = [int(np.where(env.current_data["mask"][e].numpy() == 0)[0][-1]) for e in range(eu.E)]
                actions = np.array(free)                                                   # the highest untaken action of each
                obs, reward, done = env.step(actions)
            out[f"{case}:{i}:score"], out[f"{case}:{i}:mask"] = obs["score"].numpy(), obs["mask"].numpy()
            out[f"{case}:{i}:first_score"] = obs["first_score"].numpy()
            out[f"{case}:{i}:mesh_sub"] = obs["mesh"][:, ::16].numpy()
            if c["use_latent"]:
                out[f"{case}:{i}:latent"], out[f"{case}:{i}:first_latent"] = obs["latent"].numpy(), obs["first_latent"].numpy()
            if call != "reset":
                out[f"{case}:{i}:reward"], out[f"{case}:{i}:done"] = reward.numpy(), np.bool_(done)
                out[f"{case}:{i}:actions"] = np.asarray(actions).astype(np.int64)
            print(f"case {case} call {i} ({call}): score {obs['score'].tolist()} actions {None if actions is None else list(actions)}")
        out[f"{case}:mesh"] = obs["mesh"].numpy()
    print(f"case {case}: smallest relative gap between the two lowest eligible scores {smallest:.3e}")
    assert smallest > MIN_GAP, f"case {case}: score gap {smallest:.3e} <= {MIN_GAP}: choose other seeds in env_util.CASES"


def main():
    install_simulator_stubs()
    env_mod = importlib.import_module("pterotactyl.policies.environment")
    env_mod.ActiveTouch.get_loaders = lambda self: None
    out = {"pytorch3d_restated": np.bool_(True)}
    for case in eu.CASES:
        run_case(case, env_mod, out)
    save(eu.FIXTURE, **out)


if __name__ == "__main__":
    main()
