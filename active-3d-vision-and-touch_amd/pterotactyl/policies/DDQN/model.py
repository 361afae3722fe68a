"""``pterotactyl.policies.DDQN.model`` on MI355X — a consumer of the hot-path kernels.

``Graph_Model`` (reference ``policies/DDQN/model.py:65-128``): Q-network over the predicted mesh — per-vertex features
= [action embedding | positional embedding | mask embedding] (3 x 100), ``args.layers`` graph layers
(300 -> hidden_dim ... -> num_actions; the last aggregates every channel, no ReLU), max over vertices.  The graph
layers run as ``a3vt_gcn_layer_fwd/bwd`` calls through ``vision.model.GCN_layer``; the adjacency is the dense
``adj['adj']`` the reference keeps (:68), converted to CSR once.  ``Latent_Model`` (:15-61) is a plain MLP over
auto-encoder latents.

``args.fused_q_latent`` (new, no reference counterpart; off unless ``args`` sets it; ``DDQN.train.Engine`` sets it): the learner
evaluates and updates ``Latent_Model`` through ``ops.ddqn_latent_q`` / ``ops.ddqn_latent_update`` (csrc/ddqn_latent.hip) on
``table()``, the ``ops.PolicyTable`` of the module's own parameter tensors.  ``forward`` itself stays on the torch modules: the
knob changes what ``DDQN.get_action`` and ``DDQN.update_parameters`` call, not this module's outputs.  Same parameters, same state
dict; ``load_state_dict`` copies in place, so a table stays valid across target updates.

``args.fused_q_input`` (new, no reference counterpart; off unless set; ``DDQN.get_model`` sets it): the features and layer 0 run
as ``ops.qnet_input`` (csrc/qnet_input.hip), which never forms the (B N) x 300 feature rows.  Same parameters, same state dict.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .... import ops as _ops
from ...reconstruction.vision.model import GCN_layer, Mask_Encoder, Positional_Encoder, _csr_of, _cut_len  # noqa: F401
from .. import _latent


def _dev(t, device):
    return t.float().to(device)


class Latent_Model(_latent.LatentInputs, nn.Module):
    def __init__(self, args):
        super().__init__()
        self.args = args
        self.action_model, self.model = _latent.latent_networks(args)
        self.fused_q_latent = bool(getattr(args, "fused_q_latent", False))

    def fused_ok(self, mask):
        """Whether the learner takes the fused ops for this input: the knob, a 2-d mask on the GPU, sizes inside the kernels'."""
        return bool(self.fused_q_latent and mask.is_cuda and mask.dim() == 2 and _ops.ddqn_latent_supported(self.table(), mask))

    def forward(self, obs, next=False):
        return self.mlp(*self.inputs(obs, next))


class Graph_Model(nn.Module):
    def __init__(self, args, adj):
        super().__init__()
        self.args = args
        self.num_layers = args.layers
        self.fused_q_input = bool(getattr(args, "fused_q_input", False))
        input_size = 100
        self.adj = adj["adj"]      # dense (N,N), as the reference keeps it (:68)
        self._adj_info = adj       # the CSR handle is taken from / cached in this dict
        self.action_model = _latent.action_embedding(50, input_size)  # :75 (50 = number of candidate actions)
        self.positional_embedding = Positional_Encoder(input_size)
        self.mask_embedding = Mask_Encoder(input_size)
        sizes = [input_size * 3] + [args.hidden_dim] * (args.layers - 1) + [args.num_actions]
        self.layers = nn.ModuleList([GCN_layer(sizes[i], sizes[i + 1], cut=args.cut, do_cut=i != self.num_layers - 1)
                                     for i in range(args.layers)])

    def forward(self, obs, next=False):
        dev = self.layers[0].weight.device
        sfx = "_n" if next else ""
        action = self.action_model(_dev(obs["mask" + sfx], dev))
        mesh_all = _dev(obs["mesh" + sfx], dev)
        adj = _csr_of(self._adj_info, "adj")
        first = 0
        if self._fused_input_ok(mesh_all):
            l0 = self.layers[0]
            nout = l0.weight.shape[-1]
            x = _ops.qnet_input(mesh_all, action, self.positional_embedding, self.mask_embedding.model[0].weight, l0.weight[0], l0.bias,
                                adj, _cut_len(nout, l0.cut_size) if l0.do_cut else nout)
            first = 1
        else:
            mesh, mask = mesh_all[:, :, :3], mesh_all[:, :, 3:]
            x = torch.cat((action.unsqueeze(1).expand(-1, mesh.shape[1], -1), self.positional_embedding(mesh),
                           self.mask_embedding(mask)), dim=-1)
        for i, layer in enumerate(self.layers[first:], first):   # layer 0 always takes the ReLU, also when it is the only layer (:118)
            x = layer(x, adj, F.relu if i == 0 or i != self.num_layers - 1 else _identity)
        return torch.max(x, dim=1)[0]

    def _fused_input_ok(self, mesh_all):
        """The fused input layer takes fp32 observations on the GPU that need no gradient, exact products and h <= 304; every
        other call runs the unfused layer."""
        l0 = self.layers[0]
        return (self.fused_q_input and mesh_all.is_cuda and mesh_all.dim() == 3 and mesh_all.shape[-1] == 4 and not mesh_all.requires_grad
                and l0.weight.shape[1] == 300 and _ops.qnet_input_supported(l0.weight.shape[-1])
                and not _ops.gemm_mode(getattr(l0, "gemm_bf16", False)))


def _identity(x):
    return x
