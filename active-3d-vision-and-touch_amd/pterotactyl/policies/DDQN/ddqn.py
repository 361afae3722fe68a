"""``pterotactyl.policies.DDQN.ddqn``: the double-DQN learner (reference ``policies/DDQN/ddqn.py``) on the library's kernels.

``update_parameters`` is the reference's rule, quirks included (see ``ops.ddqn_td``): three Q-network forwards, the target /
loss / loss gradient as ONE launch (``a3vt_ddqn_td``; the reference loops over the batch in Python with a device sync per
sample), one backward, and the gradient clamp inside the optimizer's single launch (``optim.Adam(grad_clamp=1)``).  The only host
sync of an update is the ``loss.item()`` it returns.  The model follows the module's device (nothing calls ``.cuda()``), and so
do the batches a host replay memory hands over (a replay built with ``device=`` samples there already).

New knob (no reference counterpart): ``args.fused_q_input`` — ``Graph_Model``'s features and layer 0 on ``ops.qnet_input``.  When
``args`` does not carry it, ``get_model`` sets it to ``FUSED_Q_INPUT_DEFAULT``: on, because ``tools/ddqn_bench.py`` measured the fused
update's p90 below the unfused one's p10 on an MI355X (``profiles/ddqn_update_ab.txt``)."""
import random

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

    def forward(self, obs, next=False, penalize=True):
        value = self.model(obs, next=next)
        if penalize:
            value = self.penalise_actions(value, obs)
        return value

    def get_action(self, obs, eps_threshold, give_random=False):
        sample = random.random()
        if sample < eps_threshold or give_random:
            return self.random_sampler.get_action(obs["mask"])
        with torch.no_grad():
            self.model.eval()
            q_values = self(obs)
        return torch.argmax(q_values, dim=1).cpu().numpy()
