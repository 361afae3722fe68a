"""Helpers shared by the ActiveTouch tests and ``golden/make_golden_env.py``: the recipe of the fixture ``g18_active_touch.npz``
(settings of its two cases, the seeded sensor records, how the three models are written to checkpoint directories) — everything
that both the generator (which drives the REFERENCE environment) and the tests (which drive this package's) must build alike."""
import json
import os
from types import SimpleNamespace

import numpy as np
import torch

import touch_util as tu

FIXTURE = "g18_active_touch.npz"
E = 2
OBJECTS = ("obj0", "obj1")
CLOUD = 900
STATUS = ("no_intersection", "no_touch", "touch")          # codes 0, 1, 2 of the fixture's status tables
MODEL = dict(use_img=False, use_touch=True, num_grasps=5, num_GCN_layers=3, hidden_GCN_size=300, cut=0.33)
CASES = {
    # full search: reset, best_step x 2
    "a": dict(finger=True, use_latent=False, num_actions=4, budget=2, greedy_checks=None, calls=("reset", "best", "best"),
              record_seed=1814, deform_seed=0, auto_seed=None, sample_seed=1811, cloud_seed=1812),
    # limited search after random.seed(0): reset, best_step x 2, one plain step
    "b": dict(finger=False, use_latent=True, num_actions=6, budget=3, greedy_checks=3, calls=("reset", "best", "best", "step"),
              record_seed=1830, deform_seed=0, auto_seed=3, sample_seed=1821, cloud_seed=1822),
}
AUTO = dict(num_GCN_layers=3, hidden_GCN_size=300, cut=0.33, encoding_size=200)
# The output layers of the seeded Deformation are scaled by this: at its initial weights the model moves the atlas by several
# object sizes and every score exceeds 1000, the value the reference's best_step starts its search from (environment.py:170) —
# it would choose no action at all.  Damped, the model deforms by centimetres, as a trained one does.
DAMP = 0.02


def env_args(case, **kw):
    c = CASES[case]
    d = dict(seed=0, eval=True, pretrained_recon=False, use_img=False, use_touch=True, finger=c["finger"], num_grasps=5,
             use_latent=c["use_latent"], num_actions=c["num_actions"], budget=c["budget"], env_batch_size=E, number_points=700,
             loss_coeff=9000.0, limit_data=False)
    d.update(kw)
    return SimpleNamespace(**d)


def vision_args(case):
    return SimpleNamespace(finger=CASES[case]["finger"], **MODEL)


def status_table(case):
    """(E, num_actions, 4) int8 codes into ``STATUS``, seeded; re-drawn until the fingers the case reads (finger 1 alone with
    ``finger``) show all three codes and no element has two actions without any contact: those leave the mesh as it is, so
    their scores tie exactly, which the fixture's score-gap condition excludes."""
    c = CASES[case]
    g = np.random.default_rng(c["record_seed"])
    while True:
        t = g.integers(0, 3, (E, c["num_actions"], 4)).astype(np.int8)
        seen = t[:, :, 1] if c["finger"] else t
        idle = (seen.reshape(E, c["num_actions"], -1) == 0).all(axis=2).sum(axis=1)
        if len(np.unique(seen)) == 3 and idle.max() <= 1:
            return t


def records(case, table):
    """The sensor records of a case, ``{(object id, action): record}`` in ``RecordedSampler``'s format: images uniform in
    [0, 255) with fractional parts (so the finger branch's truncation through uint8 shows), frames from ``touch_util.frames``."""
    c = CASES[case]
    out = {}
    for e, obj in enumerate(OBJECTS):
        for a in range(c["num_actions"]):
            seed = c["record_seed"] + 100 * e + a
            g = torch.Generator().manual_seed(seed)
            rot, pos = tu.frames(4, seed)
            out[(obj, a)] = {"touch": torch.rand(4, 121, 121, 3, generator=g) * 255.0, "rot": rot, "pos": pos,
                             "status": [STATUS[int(s)] for s in table[e, a]]}
    return out


def clouds(case):
    """(E, 900, 3) ground-truth clouds: points on seeded ellipsoids."""
    g = torch.Generator().manual_seed(CASES[case]["cloud_seed"])
    d = torch.randn(E, CLOUD, 3, generator=g)
    return d / d.norm(dim=-1, keepdim=True) * (0.05 + 0.11 * torch.rand(E, 1, 3, generator=g))


def batch_of(gt):
    return {"names": [f"/data/object_info/{o}" for o in OBJECTS], "gt_points": gt, "img": torch.zeros(E, 1)}


def write_checkpoint(directory, config, state):
    """``config.json`` + ``model`` as ``utils.save_config`` and the trainers leave them (what ``setup_recon`` loads)."""
    os.makedirs(directory, exist_ok=True)
    config = dict(config, check_point=os.path.abspath(directory))
    with open(os.path.join(directory, "config.json"), "w") as f:
        json.dump(config, f)
    torch.save({k: v.detach().cpu() for k, v in state.items()}, os.path.join(directory, "model"))
    return directory + "/"


def build_models(case, touch_module, vision_module, auto_module, utils_module, chart_file, bn=None):
    """The three seeded models of a case from the given implementation (the reference's modules in the generator, this package's
    in the tests): the touch ``Encoder`` under ``torch.manual_seed(0)`` with ``touch_util.seed_batchnorm``'s BatchNorm tensors
    (or the stored ones in ``bn``), ``Deformation`` under ``deform_seed`` with its output layers scaled by ``DAMP``, ``AutoEncoder(only_encode=True)`` under ``auto_seed``.
    Returns {"touch" | "vision" | "auto": (config dict, module)}."""
    c = CASES[case]
    torch.manual_seed(0)
    enc = touch_module.Encoder()
    if bn is None:
        tu.seed_batchnorm(enc)
    else:
        missing, unexpected = enc.load_state_dict(bn, strict=False)
        assert not unexpected and all(not tu.is_bn_key(k) for k in missing)
    va = vision_args(case)
    info, verts = utils_module.load_mesh_vision(va, chart_file)
    torch.manual_seed(c["deform_seed"])
    deform = vision_module.Deformation(info, verts, va)
    with torch.no_grad():
        for gcn in (deform.mesh_deform_1, deform.mesh_deform_2):
            gcn.layers[-1].weight.mul_(DAMP)
            gcn.layers[-1].bias.mul_(DAMP)
    out = {"touch": ({}, enc.eval()), "vision": (vars(va), deform)}
    if c["use_latent"]:
        aa = SimpleNamespace(finger=c["finger"], use_touch=True, use_img=False, num_grasps=5, **AUTO)
        torch.manual_seed(c["auto_seed"])
        out["auto"] = (vars(aa), auto_module.AutoEncoder(info, verts, aa, only_encode=True))
    return out


def write_models(root, models):
    """Checkpoint directories of ``build_models``' result under ``root``: {"touch_location": ..., "vision_location": ...,
    "auto_location": ...}."""
    return {f"{kind}_location": write_checkpoint(os.path.join(root, kind), cfg, net.state_dict()) for kind, (cfg, net) in models.items()}
