"""One FoldingNet fold restated from its formulas, in whatever dtype its operands have (fp64 on the CPU is the reference of
``test_gpu_fold.py`` and ``test_gpu_fold_edges.py``):

    z1 = code W1[:, :512]^T + b1 + g W1[:, 512:]^T,  h1 = relu(z1),  z2 = h1 W2^T + b2,  h2 = relu(z2),  y = h2 W3^T + b3

``code`` (B, 512), ``g`` (B, P, k), the parameters in ``Conv1d``'s layout ((out, in, 1) weights) under the names of ``_Fold``."""
import torch

CONV_KEYS = [f"conv{c}.{w}" for c in (1, 2, 3) for w in ("weight", "bias")]


def fold_restated(code, g, p, prefix=""):
    """-> y (B, P, 3) and the two pre-activations z1, z2 (B, P, 512) (the ReLU kinks sit at their zeros)."""
    w1, b1 = p[prefix + "conv1.weight"][:, :, 0], p[prefix + "conv1.bias"]
    w2, b2 = p[prefix + "conv2.weight"][:, :, 0], p[prefix + "conv2.bias"]
    w3, b3 = p[prefix + "conv3.weight"][:, :, 0], p[prefix + "conv3.bias"]
    z1 = (code @ w1[:, :512].T + b1)[:, None, :] + g @ w1[:, 512:].T
    z2 = torch.relu(z1) @ w2.T + b2
    return torch.relu(z2) @ w3.T + b3, z1, z2


def fp64_leaf(t):
    """A detached fp64 CPU copy that takes a gradient."""
    return t.detach().double().cpu().requires_grad_(True)
