"""``pterotactyl.policies.DDQN.ddqn``: the double-DQN learner (reference ``policies/DDQN/ddqn.py``) on the library's kernels.

``update_parameters`` is the reference's rule, quirks included (see ``ops.ddqn_td``): three Q-network forwards, the target /
loss / loss gradient as ONE launch (``a3vt_ddqn_td``; the reference loops over the batch in Python with a device sync per
sample), one backward, and the gradient clamp inside the optimizer's single launch (``optim.Adam(grad_clamp=1)``).  The only host
sync of an update is the ``loss.item()`` it returns.  The model follows the module's device (nothing calls ``.cuda()``), and so
do the batches a host replay memory hands over (a replay built with ``device=`` samples there already).

New knob (no reference counterpart): ``args.fused_q_input`` — ``Graph_Model``'s features and layer 0 on ``ops.qnet_input``.  When
``args`` does not carry it, ``get_model`` sets it to ``FUSED_Q_INPUT_DEFAULT``: on, because ``tools/ddqn_bench.py`` measured the fused
update's p90 below the unfused one's p10 on an MI355X (``profiles/ddqn_update_ab.txt``).

New knob: ``args.fused_q_latent`` — off unless ``args`` sets it (``DDQN.train.Engine`` sets it).  With it a ``Latent_Model`` on the
GPU is updated without autograd: ``ops.ddqn_latent_update`` (three launches: the three forwards side by side, TD and deltas,
gradients and loss) writes the gradients into ``p.grad`` tensors this learner owns, overwritten every update, then the same
one-launch Adam follows; ``get_action`` is ``ops.ddqn_latent_q`` (one launch: values and the penalised argmax) and one copy of E
int32.  ``last_q`` / ``last_best_next`` / ``last_target`` stay, and the only sync of an update is still the ``loss.item()``."""
import random

import numpy as np
import torch
import torch.nn as nn

from .... import optim as _optim
from .... import ops as _ops
from ..baselines import baselines
from . import model

FUSED_Q_INPUT_DEFAULT = True

# hidden_dim / layers of the published checkpoints: (use_latent, use_img, finger) -> (hidden_dim, layers)
_PRETRAINED = {(True, True, True): (300, 5), (True, True, False): (300, 5), (True, False, True): (300, 5), (True, False, False): (300, 2),
               (False, True, True): (100, 5), (False, True, False): (100, 5), (False, False, True): (100, 5), (False, False, False): (100, 2)}


class DDQN(nn.Module):
    def __init__(self, args, adj_info, replay):
        super().__init__()
        self.args = args
        self.model = self.get_model(adj_info)
        self.replay = replay
        self.optimizer = _optim.Adam(self.model.parameters(), lr=args.lr, grad_clamp=1.0)
        self.random_sampler = baselines.random_sampler(self.args)
        self._latent_grads = None      # (table, [(dweight, dbias), ..]): the p.grad tensors of the fused latent update
        self.copied = []               # (shape, dtype) of every tensor a fused action choice brought to the host (tests)

    @property
    def device(self):
        return next(self.model.parameters()).device

    def penalise_actions(self, values, obs):
        """Actions already taken can never be the argmax."""
        values[obs["mask"].to(values.device) > 0] = -1e10
        return values

    def get_model(self, adj):
        a = self.args
        if a.pretrained:
            a.hidden_dim, a.layers = _PRETRAINED[(bool(a.use_latent), bool(a.use_img), bool(a.finger))]
        if not hasattr(a, "fused_q_input"):
            a.fused_q_input = FUSED_Q_INPUT_DEFAULT
        if a.use_latent:
            return model.Latent_Model(a)
        if a.use_recon:
            return model.Graph_Model(a, adj)
        raise SystemExit("No Model type selected")

    def update_epsilon(self, epsilon, args):
        return max(args.epsilon_end, epsilon * args.epsilon_decay)

    def add_experience(self, action, observation, next_observation, reward):
        self.replay.push(action, observation, next_observation, reward)

    def update_parameters(self, target_net):
        self.model.train()
        batch = self.replay.sample()
        if batch is None:
            return None
        dev = self.device
        batch = {k: v.to(dev, torch.float32) for k, v in batch.items()}    # (a device replay hands these over in place)
        norm = self.args.normalization
        denom = batch["first_score"] if norm == "first" else (batch["score"] if norm == "current" else None)
        if self._fused_latent(batch["mask"]) and isinstance(getattr(target_net, "model", None), model.Latent_Model):
            return self._fused_latent_update(batch, denom, target_net)
        q_cur = self.forward(batch, penalize=False)
        with torch.no_grad():
            q_next_online = self.forward(batch, next=True, penalize=False)     # penalised by the CURRENT mask inside ddqn_td
            q_next_target = target_net.forward(batch, next=True, penalize=False)
        loss, self.last_best_next, self.last_target = _ops.ddqn_td(
            q_cur, q_next_online, q_next_target, batch["mask"], batch["actions"], batch["rewards"], denom, self.args.budget,
            self.args.gamma)
        self.last_q = q_cur.detach()
        self.optimizer.zero_grad()
        loss.backward()
        self.optimizer.step()          # clamps every gradient to [-1, 1] in place, then Adam
        return loss.item()

    def _fused_latent(self, mask):
        return isinstance(self.model, model.Latent_Model) and self.model.fused_q_latent and torch.is_tensor(mask) and \
            self.model.fused_ok(mask)

    def _owned_grads(self, table):
        """The gradient tensors of the fused update: ``p.grad`` of the table's parameters, kept here and overwritten every update
        (so the optimizer's pointer table stays the same from step to step)."""
        if self._latent_grads is None or self._latent_grads[0] is not table or \
                any(w.grad is not dw or b.grad is not db for (w, b, _), (dw, db) in zip(table.layers, self._latent_grads[1])):
            grads = []
            for w, b, _ in table.layers:
                w.grad, b.grad = torch.zeros_like(w), torch.zeros_like(b)
                grads.append((w.grad, b.grad))
            self._latent_grads = (table, grads)
        return self._latent_grads[1]

    def _fused_latent_update(self, batch, denom, target_net):
        net = self.model
        table = net.table()
        mask, latent, first_latent = net.inputs(batch)
        mask_n, latent_n, _ = net.inputs(batch, next=True)
        with torch.no_grad():
            loss, self.last_q, self.last_best_next, self.last_target, _ = _ops.ddqn_latent_update(
                table, target_net.model.table(), self._owned_grads(table), mask, mask_n, latent, latent_n, first_latent,
                batch["actions"], batch["rewards"], denom, self.args.budget, self.args.gamma)
        self.optimizer.step()          # clamps every gradient to [-1, 1] in place, then Adam
        return loss.item()

    def forward(self, obs, next=False, penalize=True):
        value = self.model(obs, next=next)
        if penalize:
            value = self.penalise_actions(value, obs)
        return value

    def get_action(self, obs, eps_threshold, give_random=False):
        sample = random.random()
        if sample < eps_threshold or give_random:
            return self.random_sampler.get_action(obs["mask"])
        if isinstance(self.model, model.Latent_Model) and self.model.fused_q_latent:
            mask, latent, first_latent = self.model.inputs(obs)
            if self.model.fused_ok(mask):
                self.model.eval()
                _, action = _ops.ddqn_latent_q(self.model.table(), mask, latent, first_latent, mask)
                action = action.cpu()
                self.copied.append((tuple(action.shape), action.dtype))
                return action.numpy().astype(np.int64)
        with torch.no_grad():
            self.model.eval()
            q_values = self(obs)
        return torch.argmax(q_values, dim=1).cpu().numpy()
