"""Host-side parts of the supervised latent policy (no GPU): the torch forms of ``ops.latent_policy`` / ``ops.action_value_loss``
against ``supervised_util``'s fp64 restatement, ``Latent_Model``'s state dict and seeded construction, the action choice against a
literal restatement of the reference's masking loop (``policies/supervised/train.py:119-128``, ``:190-196``), the parser's
defaults, and the engine's early-stopping / per-step load and save rule with the environment stubbed out."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import supervised_util as su

from a3vt_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def auto_dir(tmp_path, encoding_size=200):
    d = tmp_path / "auto"
    d.mkdir(exist_ok=True)
    (d / "config.json").write_text(json.dumps({"encoding_size": encoding_size, "check_point": str(d)}))
    return str(d) + "/"


def model_args(tmp_path, **kw):
    d = dict(auto_location=auto_dir(tmp_path, kw.pop("encoding_size", 200)), num_actions=50, hidden_dim=200, layers=4, normalize=0, use_img=False)
    d.update(kw)
    return SimpleNamespace(**d)


def table_of(net):
    layers, concat_at, transform = net
    return ops.PolicyTable([(torch.from_numpy(W).requires_grad_(True), torch.from_numpy(b).requires_grad_(True), r) for W, b, r in layers],
                           concat_at, transform)


@pytest.mark.parametrize("shape", [(50, 200, 4, 200, 3, "plain"), (7, 5, 2, 5, 2, "normalize"), (6, 1, 1, 5, 1, "none"), (1, 5, 4, 257, 3, "use_img")],
                         ids=lambda s: "-".join(map(str, s)))
def test_torch_forms_against_the_restatement(shape):
    A, Ls, layers, hidden, rows, tr = shape
    c = su.make_case(40, rows, A, Ls, layers, hidden, su.TRANSFORMS[tr], min_choice_gap=1e-3)
    t = table_of(c["net"])
    mask, latent, first = (torch.from_numpy(c[k]) for k in ("mask", "latent", "first_latent"))
    values, action = ops.latent_policy(t, mask, latent, first, mask)                # (CPU tensors: the torch form)
    assert float(np.abs(values.detach().numpy() - c["values"]).max()) <= float(c["value_bound"].max())
    assert action.dtype == torch.int32 and np.array_equal(action.numpy(), su.choose(c["values"], c["mask"]))
    g = c["rng"]
    actions, targets = g.integers(0, A, (5, rows)), g.standard_normal((5, rows)).astype(np.float32)
    if rows > 1:
        actions[1] = actions[0]
    want_loss, want_d = su.loss(c["values"], actions, targets)
    loss, dvalues = ops.action_value_loss(values, actions, torch.from_numpy(targets))
    assert abs(float(loss.detach()) - want_loss) <= 1e-5 * abs(want_loss) + float(c["value_bound"].max()) * 4 * abs(want_loss) ** 0.5
    assert np.abs(dvalues.numpy() - want_d).max() <= 1e-5 * np.abs(want_d).max() + float(c["value_bound"].max())
    loss.backward()
    grads, bounds = su.backward(c["net"], c["mask"], c["latent"], c["first_latent"], want_d.astype(np.float32), c["stash"], c["bounds"])
    for (dW, db), (bW, bb), (w, b, _) in zip(grads, bounds, t.layers):
        slack = 1e-5 * max(np.abs(dW).max(), 1e-30)                                   # (dvalues itself is an fp32 result here)
        assert np.abs(w.grad.numpy() - dW).max() <= bW.max() + slack and np.abs(b.grad.numpy() - db).max() <= bb.max() + slack


def reference_choice(values, cur_actions):
    """train.py:119-128 / :190-196, literally: every action of every earlier step is set to 1e10, then argmin."""
    values = values.clone()
    for acts in cur_actions:
        for e, act in enumerate(acts):
            values[e][act] = 1e10
    return torch.argmin(values, dim=1)


def test_the_choice_is_the_reference_s_masking_loop():
    g = torch.Generator().manual_seed(7)
    for trial in range(20):
        E, A, steps = 3, 50, trial % 5
        values = torch.rand(E, A, generator=g) * 200 - 100
        cur_actions, mask = [], torch.zeros(E, A)
        for _ in range(steps):                                    # an episode: each step takes an action not taken before
            acts = reference_choice(torch.rand(E, A, generator=g), cur_actions)
            cur_actions.append(acts)
            for e, a in enumerate(acts):
                mask[e, a] = 1                                    # (ActiveTouch.update_masks)
        want = reference_choice(values, cur_actions)
        assert torch.equal(ops.choose_action_torch(values, mask).long(), want)
        assert np.array_equal(su.choose(values.numpy().astype(np.float64), mask.numpy()), want.numpy())
    none_open = ops.choose_action_torch(torch.zeros(2, 4), torch.tensor([[1., 1, 1, 1], [1, 0, 1, 1]]))
    assert none_open.tolist() == [-1, 1]


REFERENCE_KEYS = [f"action_model.{i}.0.{p}" for i in range(3) for p in ("weight", "bias")] + \
    [f"model.{i}.0.{p}" for i in range(4) for p in ("weight", "bias")]


def test_state_dict_has_the_reference_s_keys_and_round_trips(tmp_path):
    from a3vt_amd.pterotactyl.policies.supervised import model as sm
    torch.manual_seed(3)
    a = sm.Latent_Model(model_args(tmp_path))
    sd = a.state_dict()
    assert list(sd) == REFERENCE_KEYS
    assert [tuple(sd[k].shape) for k in REFERENCE_KEYS[::2]] == [(200, 50), (100, 200), (200, 100), (200, 600), (200, 200), (200, 200), (50, 200)]
    torch.save(sd, str(tmp_path / "model_0"))
    b = sm.Latent_Model(model_args(tmp_path, fused_policy=True))
    b.load_state_dict(torch.load(str(tmp_path / "model_0")))
    assert all(torch.equal(sd[k], v) for k, v in b.state_dict().items())
    assert not a.fused_policy and b.fused_policy                   # off in the model unless args sets it
    obs = {"mask": torch.zeros(3, 50), "latent": torch.randn(3, 200), "first_latent": torch.randn(3, 200)}
    assert torch.equal(a(obs), b(obs))                             # (CPU tensors: the knob changes nothing, the modules run)
    values, action = b.evaluate(obs)
    assert torch.equal(values, a(obs)) and torch.equal(action.long(), values.argmin(dim=1))


@pytest.mark.parametrize("kw,scale,offset", [(dict(normalize=1), 2, 1), (dict(use_img=True), 6, 3), (dict(normalize=1, use_img=True), 2, 1), ({}, 200, 100)])
def test_output_rule(tmp_path, kw, scale, offset):
    from a3vt_amd.pterotactyl.policies.supervised import model as sm
    m = sm.Latent_Model(model_args(tmp_path, encoding_size=5, hidden_dim=8, layers=2, num_actions=6, **kw))
    obs = {"mask": torch.zeros(2, 6), "latent": torch.randn(2, 5), "first_latent": torch.randn(2, 5)}
    z = m.model(torch.cat((m.action_model(obs["mask"]), obs["latent"], obs["first_latent"]), dim=-1))
    assert torch.equal(m(obs), torch.sigmoid(z) * scale - offset)
    assert m.table().transform == (scale, offset) and m.table().concat_at == 3 and m.table().latent_size == 5


def test_seeded_construction_is_the_fixture_s(tmp_path):
    from golden_util import load, state_sha256
    from a3vt_amd.pterotactyl.policies.supervised import model as sm
    golden = load(su.FIXTURE)
    args = model_args(tmp_path, num_actions=su.NUM_ACTIONS, hidden_dim=su.HIDDEN_DIM, layers=su.LAYERS)
    torch.manual_seed(int(golden["policy_seed"]))
    models = [sm.Latent_Model(args) for _ in range(su.BUDGET)]
    sd = {f"{i}.{k}": v for i, m in enumerate(models) for k, v in m.state_dict().items()}
    assert (state_sha256(sd) == golden["sha:policy"]).all()


def test_parser_defaults():
    from a3vt_amd.pterotactyl.policies.supervised import train as st
    a = st.get_parser().parse_args([])
    assert (a.number_points, a.epoch, a.seed, a.env_batch_size, a.loss_coeff, a.num_grasps, a.num_actions, a.budget, a.layers, a.patience,
            a.training_actions, a.hidden_dim, a.train_steps, a.normalize, a.lr) == \
        (30000, 3000, 0, 3, 9000.0, 5, 50, 5, 4, 25, 5, 200, 200, 0, 0.001)
    assert (a.exp_id, a.exp_type) == ("test", "test")
    assert not any((a.limit_data, a.finger, a.use_img, a.eval, a.visualize, a.pretrained_recon, a.pretrained, a.zero_grad))
    assert a.fused_policy is None and a.batched_targets is None     # (None: the engine's measured defaults decide)
    b = st.get_parser().parse_args(["--no_fused_policy", "--batched_targets", "--zero_grad"])
    assert b.fused_policy is False and b.batched_targets is True and b.zero_grad is True
    assert st.FUSED_POLICY_DEFAULT in (True, False) and st.BATCHED_TARGETS_DEFAULT in (True, False)


class StubEnv:
    def __init__(self, args, sampler=None):
        self.args = args
        self.train_data = self.valid_data = None


def scripted_engine(tmp_path, monkeypatch, validation, **kw):
    """An engine whose ``train`` does nothing and whose ``validate`` reads its score from ``validation``; every load is logged."""
    from a3vt_amd.pterotactyl.policies import environment
    from a3vt_amd.pterotactyl.policies.supervised import train as st
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(environment, "ActiveTouch", StubEnv)
    args = SimpleNamespace(**dict(dict(auto_location=auto_dir(tmp_path, 5), num_actions=6, hidden_dim=8, layers=2, normalize=0, use_img=False,
                                       finger=False, budget=2, epoch=10, patience=2, lr=0.001, eval=False, exp_type="t", exp_id="x", pretrained=False,
                                       visualize=False, env_batch_size=2, num_grasps=5, train_steps=1), **kw))
    engine = st.Engine(args, loaders=([], []))
    engine.device = "cpu"
    log, scores = [], iter(validation)

    def train(loader, writer=None):
        log.append(("train", engine.step, engine.epoch))
        with torch.no_grad():
            engine.models[engine.step].model[0][0].bias.add_(1.0)           # every epoch changes the model being trained

    def validate(loader, writer=None):
        engine.current_loss = torch.tensor(next(scores))

    inner_load = st.Engine.load

    def load(self, train=False):
        log.append(("load", self.step, train))
        inner_load(self, train=train)

    monkeypatch.setattr(st.Engine, "load", load)
    engine.train, engine.validate = train, validate
    return engine, log, st


def test_early_stopping_and_the_per_step_checkpoints(tmp_path, monkeypatch):
    # step 0: better, better, worse, worse -> out of patience after 4 epochs, the model of epoch 1 is the one saved;
    # step 1: better, worse, worse -> 3 epochs
    engine, log, st = scripted_engine(tmp_path, monkeypatch, [0.9, 0.8, 0.85, 0.81, 0.7, 0.75, 0.72])
    engine()
    assert os.path.exists(os.path.join(engine.checkpoint_dir, "config.json"))
    assert [x for x in log if x[0] == "train"] == [("train", 0, e) for e in range(4)] + [("train", 1, e) for e in range(3)]
    assert [x for x in log if x[0] == "load"] == [("load", 0, True), ("load", 1, True)]
    assert engine.step == 2 and engine.checkpoint_dir == os.path.join("experiments/checkpoint/", "t", "x")
    saved0 = torch.load(engine.checkpoint_dir + "/model_0")
    saved1 = torch.load(engine.checkpoint_dir + "/model_1")
    assert list(saved0) == [f"action_model.{i}.0.{p}" for i in range(3) for p in ("weight", "bias")] + [f"model.{i}.0.{p}" for i in range(2) for p in ("weight", "bias")]
    # model 0 was saved after its 2nd epoch, trained through 4, and reloaded from the checkpoint when step 1 began
    assert torch.equal(engine.models[0].state_dict()["model.0.0.bias"], saved0["model.0.0.bias"])
    # model 1 was saved after its 1st epoch and went on for two more
    assert torch.allclose(engine.models[1].state_dict()["model.0.0.bias"], saved1["model.0.0.bias"] + 2.0)
    assert float(engine.best_loss) == pytest.approx(0.7) and engine.last_improvement == 2
    assert isinstance(engine.optimizer, torch.optim.Adam) and engine.optimizer.param_groups[0]["params"][0] is next(engine.models[1].parameters())


def test_eval_loads_every_model(tmp_path, monkeypatch):
    engine, log, st = scripted_engine(tmp_path, monkeypatch, [0.9, 0.95, 0.95, 0.9, 0.95, 0.95])
    engine()
    ev, log2, _ = scripted_engine(tmp_path, monkeypatch, [0.5], eval=True)
    ev()
    assert log2 == [("load", 0, False)] and ev.step == 1
    for i in range(2):
        assert torch.equal(ev.models[i].state_dict()["model.0.0.bias"], torch.load(ev.checkpoint_dir + f"/model_{i}")["model.0.0.bias"])


def test_refusals(tmp_path, monkeypatch):
    engine, log, st = scripted_engine(tmp_path, monkeypatch, [])
    engine.models = engine.make_models()
    assert engine.args.fused_policy is st.FUSED_POLICY_DEFAULT      # the engine sets the knob args does not carry
    full = torch.zeros(2, 6)
    full[1] = 1
    obs = {"mask": full, "latent": torch.zeros(2, 5), "first_latent": torch.zeros(2, 5)}
    with pytest.raises(RuntimeError, match="element 1 at step 0"):
        engine.choose(0, obs)
    obs["mask"] = torch.zeros(2, 6)
    values, action = engine.choose(0, obs)
    assert engine.copied == [((2,), torch.int32)] * 2 and action.dtype == torch.int32
    engine.args.visualize = True
    with pytest.raises(NotImplementedError):
        engine()
    with pytest.raises(NotImplementedError):
        st.Engine.validate(engine, [])
    engine.args.visualize, engine.args.pretrained, engine.args.pretrained_root, engine.step = False, True, None, 0
    monkeypatch.delenv("PTEROTACTYL_PRETRAINED", raising=False)
    with pytest.raises(FileNotFoundError):
        engine.load()
    engine.args.pretrained_root = "/somewhere"
    assert engine.pretrained_location() == "/somewhere/policies/supervised/t_g"
    engine.args.use_img, engine.args.finger = True, True
    assert engine.pretrained_location() == "/somewhere/policies/supervised/v_t_p"


def test_ops_refuse_disagreeing_operands():
    c = su.make_case(41, 2, 6, 5, 2, 8, None)
    t = table_of(c["net"])
    mask, latent, first = (torch.from_numpy(c[k]) for k in ("mask", "latent", "first_latent"))
    for bad in ((mask[:, :5], latent, first, None), (mask, latent[:1], first, None), (mask, latent, first[:, :4], None),
                (mask, latent, first, mask[:1]), (mask.double(), latent, first, None), (mask[0], latent, first, None)):
        with pytest.raises(RuntimeError, match="latent_policy"):
            ops.latent_policy(t, *bad)
    layers = c["net"][0]
    with pytest.raises(RuntimeError, match="concat_at"):
        ops.PolicyTable([(torch.from_numpy(W), torch.from_numpy(b), r) for W, b, r in layers], 0)
    with pytest.raises(RuntimeError, match="does not chain"):
        ops.PolicyTable([(torch.from_numpy(W), torch.from_numpy(b), r) for W, b, r in layers[:1] + layers[2:]], 2)
    values = torch.zeros(2, 6)
    for a, tg in ((np.full((5, 2), 6), torch.zeros(5, 2)), (np.full((5, 2), -1), torch.zeros(5, 2)), (np.zeros((5, 3), int), torch.zeros(5, 3)),
                  (np.zeros((5, 2), int), torch.zeros(4, 2)), (np.zeros((5, 2)), torch.zeros(5, 2))):
        with pytest.raises(RuntimeError, match="action_value_loss"):
            ops.action_value_loss(values, a, tg)


def test_install_as_pterotactyl_registers_the_supervised_policy():
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); import a3vt_amd; a3vt_amd.install_as_pterotactyl();"
            "import pterotactyl.policies.supervised.train as t, pterotactyl.policies.supervised.model as m;"
            "assert t.Engine.__module__.startswith('a3vt_amd') and m.Latent_Model.__module__.startswith('a3vt_amd'); print('ok')") % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
