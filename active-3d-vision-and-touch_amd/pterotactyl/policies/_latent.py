"""The skeleton ``supervised.model.Latent_Model`` and ``DDQN.model.Latent_Model`` share (reference ``supervised/model.py:11-44``,
``DDQN/model.py:15-61``): the action embedding, the MLP over ``[action embedding | latent | first latent]``, the
``ops.PolicyTable`` of their parameters and the gathering of an observation's inputs.  The two classes differ in what follows the
MLP (a squashing for the value network, nothing for the Q-network) and in which fused ops take the table."""
import torch
import torch.nn as nn

from ... import ops as _ops
from ..utility import utils


def action_embedding(num_in, out):
    return nn.Sequential(nn.Sequential(nn.Linear(num_in, 200), nn.ReLU()),
                         nn.Sequential(nn.Linear(200, 100), nn.ReLU()),
                         nn.Sequential(nn.Linear(100, out)))


def latent_networks(args):
    """``(action_model, model)`` in the reference's construction order, so that a seed draws the reference's weights: the
    embedding of the performed actions into ``latent_size``, then ``args.layers`` Linear layers ``3 * latent_size -> hidden_dim ...
    -> num_actions`` with a ReLU after all but the last.  ``latent_size`` is the auto-encoder's ``encoding_size``."""
    latent_size = utils.load_model_config(args.auto_location)[0].encoding_size
    action_model = action_embedding(args.num_actions, latent_size)
    sizes = [latent_size * 3] + [args.hidden_dim] * (args.layers - 1) + [args.num_actions]
    layers = []
    for i in range(args.layers):
        mods = [nn.Linear(sizes[i], sizes[i + 1])]
        if i < args.layers - 1:
            mods.append(nn.ReLU())
        layers.append(nn.Sequential(*mods))
    return action_model, nn.Sequential(*layers)


class LatentInputs:
    """For a module with ``action_model`` and ``model`` of ``latent_networks``."""
    _table = None

    def table(self, transform=None):
        """The ``ops.PolicyTable`` of this model's parameters with the output ``transform`` (rebuilt when a parameter tensor was
        replaced)."""
        seqs = list(self.action_model) + list(self.model)
        params = [t for seq in seqs for t in (seq[0].weight, seq[0].bias)]
        if self._table is None or any(a is not b for a, b in zip(self._table.params(), params)):
            self._table = _ops.PolicyTable([(seq[0].weight, seq[0].bias, len(seq) > 1) for seq in seqs], len(self.action_model), transform)
        return self._table

    def inputs(self, obs, next=False):
        """(mask, latent, first_latent) of an observation — or with ``next`` of a replay batch's next state — on the model's
        device, as float32."""
        dev = self.model[0][0].weight.device
        sfx = "_n" if next else ""
        return tuple(obs[k].float().to(dev) for k in ("mask" + sfx, "latent" + sfx, "first_latent"))

    def mlp(self, mask, latent, first_latent):
        return self.model(torch.cat((self.action_model(mask), latent, first_latent), dim=-1))
