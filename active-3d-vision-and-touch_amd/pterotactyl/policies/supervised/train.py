"""Drop-in for ``pterotactyl/policies/supervised/train.py`` — the supervised latent policy.

One ``Latent_Model`` per grasp of the budget.  Model ``i`` is trained at step ``i``: the earlier models move the environment to
that step, the model predicts a value for every action, five random actions per element are tried (``check_step``), and the model
regresses its values of those actions onto the improvements they brought (reference :103-171).  Validation plays whole episodes
with the models trained so far, each choosing its lowest-valued action not performed yet (:174-242); a step's training stops
after ``patience`` epochs without a better validation score, and the model of the best epoch is the one saved (:244-257).

``Engine(args, sampler=None, loaders=None)`` has the reference's methods (``__call__``, ``get_loaders``, ``train``, ``validate``,
``check_values``, ``load``, ``save``) and attributes (``models``, ``optimizer``, ``step``, ``epoch``, ``best_loss``,
``last_improvement``, ``train_loss``, ``current_loss``, ``results_dir``, ``checkpoint_dir``); ``sampler`` goes to ``ActiveTouch``,
``loaders=(train, valid)`` injects data.  ``get_parser()`` carries the reference's flags and defaults (:317-437; ``use_recon =
False`` and ``use_latent = True`` are set after parsing).  Checkpoints are the reference's ``model_<i>`` state dicts.

What runs where:

* **Action choice** — ``Engine.choose(i, obs)``: one ``Latent_Model.evaluate`` call returns the values and the chosen action
  (``args.fused_policy``, default ``FUSED_POLICY_DEFAULT``: ``ops.latent_policy``, one launch), and one copy of E int32 leaves
  the device.  ``obs["mask"]`` is the table of performed actions: it marks exactly the actions the reference's ``cur_actions``
  loop sets to 1e10, since both start empty at ``reset`` and grow by the action of every ``step``.
* **Targets** — ``args.batched_targets`` (default ``BATCHED_TARGETS_DEFAULT``): the five random action lists are scored by one
  ``env.score_candidates`` call (one batch of 5 E meshes); off, the reference's five ``check_step`` calls run.
* **Update** — with the fused model the step does not go through autograd: ``ops.latent_policy_fwd`` with its stash,
  ``ops.action_value_loss``, ``ops.latent_policy_bwd`` into gradient tensors the engine owns, then this package's ``optim.Adam``:
  five launches, no host sync (``FusedUpdate``).  Otherwise the reference's lines run on torch ops.

What differs from the reference, and why:

* The random actions are drawn from ``args.num_actions``; the reference has the literal 50 (:135-137).  The draws are identical
  at the reference's default.
* The reference never zeroes gradients between iterations (:157-159 follow no ``zero_grad``): every step applies the sum of all
  gradients so far.  Mirrored by default — on the fused path through the kernel's ``accumulate`` — and switched off by
  ``args.zero_grad=True`` (``--zero_grad``).
* An element with no open action raises a ``RuntimeError`` naming element and step; the reference's ``argmin`` would return an
  action already performed.
* ``visualize`` raises ``NotImplementedError`` (pyrender; ``_core.refuse_visualize``).
* The bare ``except: continue`` around ``env.reset`` (:112-115, :183-186) is ``except Exception``.
* The loss is read once per ``train`` call, not per iteration (the reference's per-iteration message synchronises with the device).
* Pretrained policies resolve to ``<pretrained_root>/policies/supervised/{t_p,t_g,v_t_p,v_t_g}/`` (``args.pretrained_root`` or
  ``PTEROTACTYL_PRETRAINED``) by the reference's ``(use_img, finger)`` rule; the reference reads them from inside its package.
"""
import json
import os
from collections import namedtuple

import numpy as np
import torch

from .... import ops
from .... import optim as a3vt_optim
from ...utility import utils
from ...utility.utils import SummaryWriter
from .. import _core
from ..baselines import baselines
from . import model as learning_model

# Whether the engine turns the fused value network on, and scores the training targets as one batch, when args does not say: each
# on only if the new form's p90 lies below the old form's p10 on an MI355X (tools/supervised_bench.py ->
# profiles/supervised_step_ab.txt).  Measured, host wall per call at E = 3, 50 actions, latent 200, 4 x 200: one evaluation with
# action choice 0.173 ms (p90 0.178) against the modules and the masking loop's 0.682 (p10 0.665); one update 0.337 (p90 0.354)
# against 1.589 (p10 1.566); one train iteration 17.4 (p90 17.6) against 37.2 (p10 36.3) with five check_step calls.
FUSED_POLICY_DEFAULT = True
BATCHED_TARGETS_DEFAULT = True

TRAINING_ACTIONS = 5        # the literal 5 of the reference's random draw (:135-137)


def _knob(args, name, default):
    value = getattr(args, name, None)
    return default if value is None else bool(value)


class FusedUpdate:
    """One policy update outside autograd: forward with stash, loss, backward into gradient tensors kept here (``p.grad`` of the
    model's parameters, so the optimizer finds them), Adam — five launches.  ``accumulate`` keeps adding to the gradients, as
    the reference's missing ``zero_grad`` does; the first update starts from zeros either way."""

    def __init__(self, model, optimizer, accumulate):
        self.model, self.optimizer, self.accumulate = model, optimizer, bool(accumulate)
        self.table = model.table()
        self.grads = []
        for w, b, _ in self.table.layers:
            w.grad, b.grad = torch.zeros_like(w), torch.zeros_like(b)
            self.grads.append((w.grad, b.grad))

    def __call__(self, obs, actions, targets):
        """``actions`` (T, E) host integers, ``targets`` (T, E) -> (loss (device scalar), values (E, A))."""
        mask, latent, first_latent = self.model._inputs(obs)
        with torch.no_grad():
            values, _, stash = ops.latent_policy_fwd(self.table, mask, latent, first_latent, None, stash=True)
            loss, dvalues = ops.action_value_loss(values, actions, targets.to(values.device, torch.float32))
            ops.latent_policy_bwd(self.table, mask, latent, first_latent, dvalues, stash, self.grads, self.accumulate)
            self.optimizer.step()
        return loss, values


class Engine(_core.EngineBase):
    shuffle_train = True

    def __init__(self, args, sampler=None, loaders=None):
        super().__init__(args, sampler, loaders)     # (device: where the policy's models live)
        self.results_dir = os.path.join("results", args.exp_type, args.exp_id)
        os.makedirs(self.results_dir, exist_ok=True)
        self.checkpoint_dir = os.path.join("experiments/checkpoint/", args.exp_type, args.exp_id)
        os.makedirs(self.checkpoint_dir, exist_ok=True)
        if not self.args.eval:
            utils.save_config(self.checkpoint_dir, args)
        self.copied = []        # (shape, dtype) of every tensor `choose` brought to the host (tests)
        self.last = {}          # the last train iteration's random actions, targets, values and loss (tests, the bench)
        self._update = None

    def make_models(self):
        if getattr(self.args, "fused_policy", None) is None:
            self.args.fused_policy = FUSED_POLICY_DEFAULT
        return [learning_model.Latent_Model(self.args).to(self.policy_device()) for _ in range(self.args.budget)]

    def __call__(self):
        _core.refuse_visualize(self.args)
        # setup the environment, policy and data
        self.make_env()
        self.policy = baselines.even_sampler(self.args)
        train_loaders, valid_loaders = self.get_loaders()
        self.step = 0
        self.models = self.make_models()
        writer = SummaryWriter(os.path.join("experiments/tensorboard/", self.args.exp_type))

        if self.args.eval:
            with torch.no_grad():
                self.load(train=False)
                self.step = self.args.budget - 1
                self.validate(valid_loaders, writer)
                return
        for i in range(self.args.budget):
            self.start_step()
            for j in range(self.args.epoch):
                self.train(train_loaders, writer)
                with torch.no_grad():
                    self.validate(valid_loaders, writer)
                if self.check_values():
                    break
                self.epoch += 1
            self.step += 1

    def start_step(self):
        """What the reference does before the epochs of a step (:64-71): a fresh Adam over this step's model, the earlier
        steps' saved models loaded back, every model in eval mode, the early-stopping state cleared."""
        self.optimizer = a3vt_optim.Adam(list(self.models[self.step].parameters()), lr=self.args.lr, weight_decay=0)
        self._update = None
        self.load(train=True)
        for m in self.models:
            m.eval()
        self.epoch = 0
        self.best_loss = 10000
        self.last_improvement = 0

    def choose(self, i, obs):
        """Model ``i``'s step -> (values (E, A) on the device, actions (E,) host int32): the lowest value among the actions
        ``obs["mask"]`` leaves open.  One model call, one copy of E integers to the host."""
        values, action = self.models[i].evaluate(obs)
        action = action.cpu()
        self.copied.append((tuple(action.shape), action.dtype))
        missing = torch.where(action < 0)[0]
        if len(missing):
            raise RuntimeError(f"a3vt: supervised policy: element {int(missing[0])} at step {i} has no action left to take")
        return values, action

    def targets(self, obs, random_actions):
        """(T, E) host improvements of the random action lists (:139-152): ``first_score - score`` after each, divided by
        ``first_score`` with ``normalize``."""
        if _knob(self.args, "batched_targets", BATCHED_TARGETS_DEFAULT):
            scores = self.env.score_candidates([[int(a) for a in actions] for actions in random_actions])
            first = obs["first_score"].unsqueeze(0)
        else:
            checked = [self.env.check_step(actions) for actions in random_actions]
            scores = torch.stack([o["score"] for o in checked])
            first = torch.stack([o["first_score"] for o in checked])
        target = first - scores
        return target / first if self.args.normalize else target

    def update(self, obs, random_actions, target):
        """One optimizer step of ``models[step]`` on ``mean((target - values[e][a])^2)`` -> (loss, values), both on the device."""
        net = self.models[self.step]
        accumulate = not getattr(self.args, "zero_grad", False)
        if net.fused_policy and net._fused_ok(net._inputs(obs)[0]):
            if self._update is None or self._update.model is not net or self._update.optimizer is not self.optimizer:
                self._update = FusedUpdate(net, self.optimizer, accumulate)
            return self._update(obs, random_actions, target)
        all_pred_values = net(obs)
        idx = torch.as_tensor(np.asarray(random_actions), dtype=torch.long, device=all_pred_values.device)
        pred_values = all_pred_values.gather(1, idx.t()).t()          # pred_values[t][e] = all_pred_values[e, random_actions[t][e]]
        loss = ((target.to(all_pred_values.device) - pred_values) ** 2).mean()
        if not accumulate:
            self.optimizer.zero_grad()
        loss.backward()
        self.optimizer.step()
        return loss.detach(), all_pred_values.detach()

    def train(self, dataloader, writer=None):
        total_loss, iterations = None, 0
        self.models[self.step].train()
        E = self.args.env_batch_size
        for v, batch in enumerate(dataloader):
            if v >= self.args.train_steps:
                break
            try:
                obs = self.env.reset(batch)
            except Exception:
                continue
            # move to the correct step
            with torch.no_grad():
                for i in range(self.step):
                    _, actions = self.choose(i, obs)
                    obs, _, _ = self.env.step(actions.numpy())
            # sample some random actions and compute their value
            random_actions = np.random.randint(self.args.num_actions, size=E * TRAINING_ACTIONS).reshape(TRAINING_ACTIONS, E)
            with torch.no_grad():
                target = self.targets(obs, random_actions)
            loss, values = self.update(obs, random_actions, target)
            self.last = {"random_actions": random_actions, "target": target, "values": values, "loss": loss}
            total_loss = loss if total_loss is None else total_loss + loss
            iterations += 1
        self.train_loss = float(total_loss) / iterations if iterations else float("nan")
        print(f"Train || step {self.step + 1} || Epoch: {self.epoch}, loss: {self.train_loss:.3f}, b_ptp:  {self.best_loss:.3f}")
        if writer is not None:
            writer.add_scalars(f"train_loss_{self.step}", {self.args.exp_id: self.train_loss}, self.epoch)

    # perform the validation
    def take_step(self, i, obs):
        _, action = self.choose(i, obs)
        obs, _, done = self.env.step(action.numpy())
        return action.long(), obs, done

    def validate(self, dataloader, writer=None):
        _core.refuse_visualize(self.args)
        scores, actions, names = [], [], []
        self.models[self.step].eval()
        for v, batch in enumerate(dataloader):
            names += batch["names"]
            try:
                obs = self.env.reset(batch)
            except Exception:
                continue
            self.policy.reset()
            cur_scores, cur_actions = self.play(obs, self.take_step, steps=self.step + 1)
            scores.append(cur_scores)
            actions.append(cur_actions)
            now = _core.summary(cur_scores)
            print(f"Valid || score: {now['score']:.4f}, reward = {now['reward']:.4f}")
        total = self.report(scores, actions, names, f"Total Valid || step {self.step + 1} || score: {{score:.4f}}, reward = {{reward:.4f}}")
        self.current_loss = total["score"]
        if not self.args.eval and writer is not None:
            writer.add_scalars(f"valid_loss_{self.step}", {self.args.exp_id: self.current_loss}, self.epoch)

    def check_values(self):
        if self.best_loss >= self.current_loss:
            improvement = self.best_loss - self.current_loss
            print(f"Saving with {improvement:.3f} improvement on Validation Set ")
            self.best_loss = self.current_loss
            self.last_improvement = 0
            self.save()
            return False
        self.last_improvement += 1
        if self.last_improvement >= self.args.patience:
            print(f"Over {self.args.patience} steps since last improvement")
            print("Moving to next step or exiting")
            return True
        return None         # (as the reference: neither saved nor out of patience)

    def pretrained_location(self):
        return os.path.join(utils.pretrained_root(self.args), "policies", "supervised", _core.kind(self.args))

    def load(self, train=False):
        if self.args.pretrained:
            location = self.pretrained_location()
            with open(f"{location}/config.json") as json_file:
                data = json.load(json_file)
            data["auto_location"] = self.args.auto_location
            data["eval"] = True
            data["visualize"] = self.args.visualize
            for knob in ("fused_policy", "batched_targets", "pretrained_root"):     # (this package's knobs stay the caller's)
                data[knob] = getattr(self.args, knob, None)
            if data["fused_policy"] is None:
                data["fused_policy"] = FUSED_POLICY_DEFAULT
            self.args = namedtuple("ObjectName", data.keys())(*data.values())
            self.models = [learning_model.Latent_Model(self.args).to(self.policy_device()) for _ in range(self.args.budget)]
            for i in range(self.args.budget):
                self.models[i].load_state_dict(torch.load(location + f"/model_{i}", map_location=self.policy_device()))
            return
        for i in range(self.step if train else self.args.budget):
            self.models[i].load_state_dict(torch.load(self.checkpoint_dir + f"/model_{i}", map_location=self.policy_device()))

    def save(self):
        torch.save(self.models[self.step].state_dict(), self.checkpoint_dir + f"/model_{self.step}")


def get_parser():
    """The reference's flags and defaults (:317-437) and this package's."""
    parser = _core.common_parser(auto_location=True, pretrained=True)
    parser.add_argument("--epoch", type=int, default=3000, help="number of epochs per step")
    parser.add_argument("--eval", action="store_true", default=False, help="for evaluating on test set")
    parser.add_argument("--exp_id", type=str, default="test", help="The experiment name.")
    parser.add_argument("--layers", type=int, default=4, help="Number of layers in the q network")
    parser.add_argument("--patience", type=int, default=25, help="number of epochs without progress before stopping")
    parser.add_argument("--training_actions", type=int, default=5,
                        help="number of action values learned for each object in each iteration")
    parser.add_argument("--hidden_dim", type=int, default=200, help="hidden dimension size in layers in the q network")
    parser.add_argument("--train_steps", type=int, default=200, help="number of training steps per epoch")
    parser.add_argument("--normalize", type=int, default=0, help="number of training steps per epoch")
    parser.add_argument("--lr", type=float, default=0.001, help="Initial learning rate.")
    parser.add_argument("--fused_policy", dest="fused_policy", action="store_true", default=None,
                        help="evaluate and train the value network on the fused kernels")
    parser.add_argument("--no_fused_policy", dest="fused_policy", action="store_false", help="... on the torch modules")
    parser.add_argument("--batched_targets", dest="batched_targets", action="store_true", default=None,
                        help="score the five random action lists of a training iteration as one batch")
    parser.add_argument("--no_batched_targets", dest="batched_targets", action="store_false", help="... by five check_step calls")
    parser.add_argument("--zero_grad", action="store_true", default=False,
                        help="zero the gradients before every backward pass (the reference never does)")
    return parser


def main(argv=None):
    return _core.run(Engine, get_parser(), argv, after_parse=_core.latent_only)


if __name__ == "__main__":
    main()
