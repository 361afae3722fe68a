"""Helpers shared by the ActiveTouch tests and ``golden/make_golden_env.py``: the recipe of the fixture ``g18_active_touch.npz``
(settings of its two cases, the seeded sensor records, how the three models are written to checkpoint directories) — everything
that both the generator (which drives the REFERENCE environment) and the tests (which drive this package's) must build alike.

The policy fixtures g19 - g22 are built on the same recipe: ``objects``, ``batch_seed``, ``status_table``, ``records``, ``clouds``
and ``batches`` are defined here once, with what the fixtures vary (seeds, the action count, the finger read, the idle rule) as
arguments; ``nn_policy_util``, ``supervised_util`` and ``tally_util`` fill in their constants.  The last three functions are the
set-up the GPU tests of g18 - g22 share."""
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


def objects(kind, b):
    """The two object ids of batch ``b`` of the ``kind`` ("train" / "valid") loader of a per-batch fixture (g19 - g22)."""
    return (f"{kind}{b}_0", f"{kind}{b}_1")


def batch_seed(base, kind, b):
    return base + (0 if kind == "train" else 50) + 7 * b


def status_table(seed, num_actions, finger=False, idle_rule=True):
    """(E, num_actions, 4) int8 codes into ``STATUS``, seeded; re-drawn until the fingers read (finger 1 alone with ``finger``)
    show all three codes and, under ``idle_rule``, no element has two actions without any contact: those leave the mesh as it is,
    so their scores tie exactly, which the fixtures' score-gap conditions exclude."""
    g = np.random.default_rng(seed)
    while True:
        t = g.integers(0, 3, (E, num_actions, 4)).astype(np.int8)
        seen = t[:, :, 1] if finger else t
        idle = (seen.reshape(E, num_actions, -1) == 0).all(axis=2).sum(axis=1)
        if len(np.unique(seen)) == 3 and (not idle_rule or idle.max() <= 1):
            return t


def records(objs, num_actions, table, seed):
    """The sensor records of one batch, ``{(object id, action): record}`` in ``RecordedSampler``'s format, record (e, a) from
    ``seed + 100 e + a``: images uniform in [0, 255) with fractional parts (so the finger branch's truncation through uint8
    shows), frames from ``touch_util.frames``."""
    out = {}
    for e, obj in enumerate(objs):
        for a in range(num_actions):
            s = seed + 100 * e + a
            g = torch.Generator().manual_seed(s)
            rot, pos = tu.frames(4, s)
            out[(obj, a)] = {"touch": torch.rand(4, 121, 121, 3, generator=g) * 255.0, "rot": rot, "pos": pos,
                             "status": [STATUS[int(code)] for code in table[e, a]]}
    return out


def clouds(seed):
    """(E, 900, 3) ground-truth clouds: points on seeded ellipsoids."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(E, CLOUD, 3, generator=g)
    return d / d.norm(dim=-1, keepdim=True) * (0.05 + 0.11 * torch.rand(E, 1, 3, generator=g))


def batch_of(gt, objs=OBJECTS):
    return {"names": [f"/data/object_info/{o}" for o in objs], "gt_points": gt, "img": torch.zeros(E, 1)}


# g18's own cases: one batch of ``OBJECTS``, table and records from the case's ``record_seed``, clouds from its ``cloud_seed``.

def case_table(case):
    c = CASES[case]
    return status_table(c["record_seed"], c["num_actions"], finger=c["finger"])


def case_records(case, table):
    return records(OBJECTS, CASES[case]["num_actions"], table, CASES[case]["record_seed"])


# The per-batch fixtures (g19 - g22): every batch of the "train" / "valid" loaders has its own two objects, status table, sensor
# records and clouds, all drawn from ``batch_seed(base, kind, b)``; ``counts`` = {"train": batches, "valid": batches}.

def status_tables(base, counts, num_actions, idle_rule=True):
    return {f"{kind}{b}": status_table(batch_seed(base, kind, b), num_actions, idle_rule=idle_rule)
            for kind, count in counts.items() for b in range(count)}


def batch_records(base, counts, num_actions, tables):
    """Every batch's sensor records in one mapping (``records`` from ``10 batch_seed``)."""
    out = {}
    for kind, count in counts.items():
        for b in range(count):
            out.update(records(objects(kind, b), num_actions, tables[f"{kind}{b}"], 10 * batch_seed(base, kind, b)))
    return out


def batches(base, kind, count):
    """The ``kind`` loader as a list of batches: names, ``clouds`` from ``batch_seed + 3``, no image."""
    return [batch_of(clouds(batch_seed(base, kind, b) + 3), objects(kind, b)) for b in range(count)]


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


# ---- what the GPU tests of g18 - g22 set up alike ---------------------------------------------------------------------------------

def package_models(case, golden, directory, prefix=""):
    """The checkpoint directories (``write_models``) under ``directory`` of this package's models built by ``build_models`` with
    the BatchNorm tensors of the golden file, after asserting their checksums against its ``{prefix}sha:<kind>`` entries."""
    from golden_util import state_sha256
    from a3vt_amd.pterotactyl.reconstruction.autoencoder import model as auto_model
    from a3vt_amd.pterotactyl.reconstruction.touch import model as touch_model
    from a3vt_amd.pterotactyl.reconstruction.vision import model as vision_model
    from a3vt_amd.pterotactyl.utility import utils
    bn = {k[3:]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith("bn:")}
    models = build_models(case, touch_model, vision_model, auto_model, utils, "vision_charts", bn=bn)
    for kind, (_, net) in models.items():
        sd = tu.non_bn_state(net.state_dict()) if kind == "touch" else net.state_dict()
        assert (state_sha256(sd) == golden[f"{prefix}sha:{kind}"]).all(), f"{prefix}the seeded {kind} model is not the fixture's"
    return write_models(str(directory), models)


def score_samples(golden, prefix=""):
    """The injected surface draws of a golden file as ``ActiveTouch.score_samples`` takes them."""
    return (torch.from_numpy(golden[prefix + "face_idx"].astype(np.int32)), torch.from_numpy(golden[prefix + "u"]),
            torch.from_numpy(golden[prefix + "v"]))


def kept_process_flags():
    """Generator body of the ``restore_process_flags`` fixtures: ``ActiveTouch.seed`` sets torch's convolution flags
    process-wide, as the reference does; other tests get them back."""
    b = torch.backends.cudnn
    kept = (b.deterministic, b.benchmark)
    yield
    b.deterministic, b.benchmark = kept
