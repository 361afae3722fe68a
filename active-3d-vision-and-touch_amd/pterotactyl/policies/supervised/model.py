"""Drop-in for ``pterotactyl/policies/supervised/model.py`` — the supervised policy's value network.

``Latent_Model(args)`` has the reference's module tree in the reference's construction order (:11-44): ``action_model`` =
Linear(num_actions, 200) / ReLU, Linear(200, 100) / ReLU, Linear(100, latent_size), then ``model`` = ``args.layers`` Linear layers
``3 * latent_size -> hidden_dim ... -> num_actions`` with a ReLU after all but the last.  ``torch.manual_seed(s); Latent_Model(args)``
draws the reference's weights, the state dict has the reference's keys, so its ``model_<i>`` checkpoints load in both directions.
``latent_size`` is ``utils.load_model_config(args.auto_location)[0].encoding_size``.  The output rule is the reference's (:52-57):
``sigmoid(z) * 2 - 1`` with ``normalize``, else ``* 6 - 3`` with ``use_img``, else ``* 200 - 100``.

``args.fused_policy`` (new, no reference counterpart; off unless ``args`` sets it; ``supervised.train.Engine`` sets it): the
forward — under autograd the backward too — runs as ``ops.latent_policy`` (csrc/latent_policy.hip: one launch for the seven layers,
the concat and the squashing) whenever the observation is on the GPU and the sizes are inside the kernel's limits
(``ops.LATENT_POLICY_MAX``).  Otherwise the torch modules run, unchanged.  Same parameters, same state dict.

``evaluate(obs, taken)`` (new) returns the values and, per element, the index of the lowest value among the actions ``taken``
leaves open (``taken == 0``): the reference's ``values[e][act] = 1e10`` loop and ``argmin`` (train.py:119-128) as part of the same
op call.
"""
import torch
import torch.nn as nn

from .... import ops as _ops
from .. import _latent


def output_transform(args):
    """``(scale, offset)`` of ``sigmoid(z) * scale - offset`` (:52-57)."""
    if args.normalize:
        return 2.0, 1.0
    if args.use_img:
        return 6.0, 3.0
    return 200.0, 100.0


class Latent_Model(_latent.LatentInputs, nn.Module):
    def __init__(self, args):
        super().__init__()
        self.args = args
        # the embedding of the performed actions, then the MLP over [it | current latent | first latent] -> a value per action
        self.action_model, self.model = _latent.latent_networks(args)
        self.fused_policy = bool(getattr(args, "fused_policy", False))

    def table(self):
        return super().table(output_transform(self.args))

    def _inputs(self, obs):
        return self.inputs(obs)

    def _modules_forward(self, mask, latent, first_latent):
        scale, offset = output_transform(self.args)
        return torch.sigmoid(self.mlp(mask, latent, first_latent)) * scale - offset

    def _fused_ok(self, mask):
        return self.fused_policy and mask.is_cuda and mask.dim() == 2 and _ops.policy_supported(self.table(), mask)

    def forward(self, obs):
        mask, latent, first_latent = self._inputs(obs)
        if self._fused_ok(mask):
            return _ops.latent_policy(self.table(), mask, latent, first_latent)[0]
        return self._modules_forward(mask, latent, first_latent)

    def evaluate(self, obs, taken=None):
        """``(values (E, A), action (E,) int32)``: ``forward`` and the action choice among ``taken == 0`` (default:
        ``obs["mask"]``, the environment's record of the actions performed) — one op call with the knob on."""
        mask, latent, first_latent = self._inputs(obs)
        taken = mask if taken is None else taken.float().to(mask.device)
        if self._fused_ok(mask):
            return _ops.latent_policy(self.table(), mask, latent, first_latent, taken)
        values = self._modules_forward(mask, latent, first_latent)
        return values, _ops.choose_action_torch(values, taken)
