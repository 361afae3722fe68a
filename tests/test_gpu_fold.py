"""-m gpu: the fused FoldingNet decoder (``args.fused_decoder``: ``ops.fold`` on ``a3vt_fold_fwd/bwd``, csrc/fold.hip).

* against the reference's golden vectors (the body of ``test_g9_autoencoder`` with the knob on);
* against an fp64 restatement of the decoder, written here from the formulas
      h1 = relu(W1[:, :512] code_b + b1 + W1[:, 512:] g_p),  h2 = relu(W2 h1 + b2),  y = W3 h2 + b3
  applied twice (fold 1 on the 80 x 80 lattice, fold 2 on fold 1's output), at the trainer's shapes;
* that no (B * P) x 512 tensor exists: the peak of the allocator over a forward + backward;
* that two runs give the same bits and that a sample's forward does not depend on the batch around it.

The upstream gradient of the fp64 comparison is smooth and one-signed, dy[b, c, p] = s_c (1 + 0.5 sin(3 u_p + c)),
s = (1, -0.7, 0.4), u_p the lattice's first coordinate: with a random dy the weight gradients are cancelling sums in which a
single ReLU unit that flips between two correct evaluations moves a whole column, and torch's own fp32 decoder does not stay
inside ``assert_grad_close``'s caps against fp64 either; with this dy it does (0 elements outside, relative L2 <= 5.5e-5)."""
import numpy as np
import pytest
import torch

from fold_ref import fold_restated, fp64_leaf
from golden_util import load
from helpers import assert_grad_close, make_args, rel_err

pytestmark = pytest.mark.gpu

DEC_KEYS = [f"fold{f}.conv{c}.{w}" for f in (1, 2) for c in (1, 2, 3) for w in ("weight", "bias")]


def _decoder(cuda, fused, seed=0):
    from a3vt_amd.pterotactyl.reconstruction.autoencoder import model as am
    torch.manual_seed(seed)
    return am.FoldingNetDec(fused=fused).to(cuda)        # torch's default Conv1d initialisation, as the reference


def _lattice(points):
    from a3vt_amd.pterotactyl.reconstruction.autoencoder import model as am
    return torch.from_numpy(am.GridSamplingLayer(1, [[-0.5, 0.5, 80], [-0.5, 0.5, 80]]))[0, :points]      # (P, 2)


def _fused_decode(dec, code, points):
    """The fused decoder on the first ``points`` lattice points (6400: exactly ``dec(code)``) -> (B, P, 3)."""
    from a3vt_amd import ops
    grid = _lattice(points).to(code.device)[None].expand(code.size(0), -1, -1).contiguous()
    folded = ops.fold(code, grid, dec.fold1.conv1, dec.fold1.conv2, dec.fold1.conv3)
    return ops.fold(code, folded, dec.fold2.conv1, dec.fold2.conv2, dec.fold2.conv3)


def _fp64_decode(sd, code, points):
    """fp64 restatement (CPU): returns y (B, P, 3) and the leaves (code, parameters) it was computed from."""
    code = fp64_leaf(code)
    p = {k: fp64_leaf(v) for k, v in sd.items()}
    g = _lattice(points).double()[None].expand(code.size(0), -1, -1)
    for f in (1, 2):
        g = fold_restated(code, g, p, f"fold{f}.")[0]
    return g, code, p


def _smooth_dy(batch, points):
    u = _lattice(points)[:, 0].double()
    s = torch.tensor([1.0, -0.7, 0.4], dtype=torch.float64)
    c = torch.arange(3, dtype=torch.float64)
    dy = s[None, :] * (1.0 + 0.5 * torch.sin(3.0 * u[:, None] + c[None, :]))       # (P, 3)
    return dy[None].expand(batch, -1, -1).contiguous()


def test_g9_autoencoder_fused_decoder(cuda):
    """Reference-anchored: ``test_g9_autoencoder`` with ``fused_decoder=True``.  ``g:decoder.initial.bias`` and everything
    upstream of it pass through both folds' backward."""
    from golden_util import state_sha256
    from a3vt_amd import ops
    from a3vt_amd.pterotactyl.reconstruction.autoencoder import model as am
    from a3vt_amd.pterotactyl.utility import utils
    z = load("g9_autoencoder.npz")
    args = make_args(use_touch=True, num_grasps=1, finger=False, num_GCN_layers=3, hidden_GCN_size=300, encoding_size=200,
                     fused_decoder=True)
    info, verts = utils.load_mesh_vision(args, "vision_charts")
    torch.manual_seed(0)
    net = am.AutoEncoder(info, verts, args)
    assert net.decoder.model.fused
    assert np.array_equal(state_sha256(net.state_dict()), z["weight_sha256"]), "init differs from the reference"
    net = net.to(cuda)
    v_in, mask = torch.from_numpy(z["verts_in"]).to(cuda), torch.from_numpy(z["mask"]).to(cuda)
    samples = tuple(torch.from_numpy(z[k].astype(np.int32) if k == "face_idx" else z[k]).to(cuda) for k in ("face_idx", "u", "v"))
    ops.path_counts(reset=True)
    pred, latent = net(v_in, mask)
    assert pred.shape == (2, 6400, 3)
    assert rel_err(latent, torch.from_numpy(z["latent"])) < 1e-4
    assert rel_err(pred[:, ::16], torch.from_numpy(z["pred_points"])) < 1e-4
    cd = utils.chamfer_distance(v_in, info["faces"], pred, num=300, samples=samples)
    assert rel_err(cd, torch.from_numpy(z["cd"])) < 1e-4
    (9000.0 * cd.mean()).backward()
    counts = ops.path_counts()
    assert counts["fold_fwd"] == 2 and counts["fold_bwd"] == 2, counts
    params = dict(net.named_parameters())
    for key in [k for k in z.files if k.startswith("g:")]:
        gk = params[key[2:]].grad
        got = gk[..., ::7, ::11] if key == "g:encoder.layers.2.weight" else gk
        assert_grad_close(got, torch.from_numpy(z[key]), key)


@pytest.mark.parametrize("batch,points,scale", [(1, 6400, 1.0), (3, 6400, 0.3), (16, 6400, 3.0), (3, 1000, 1.0)])
def test_fused_decoder_against_fp64(cuda, batch, points, scale):
    dec = _decoder(cuda, fused=True, seed=1)
    g = torch.Generator().manual_seed(100 + batch)
    code = (scale * torch.randn(batch, 512, generator=g)).to(cuda).requires_grad_(True)
    y = _fused_decode(dec, code, points)
    if points == 6400:       # the module's own forward is the same computation
        assert torch.equal(dec(code), y.transpose(2, 1))
    dy = _smooth_dy(batch, points)
    y.backward(dy.float().to(cuda))
    ref, rcode, rp = _fp64_decode(dict(dec.named_parameters()), code, points)
    ref.backward(dy)
    print(f"\nfold fp64 B={batch} P={points} scale={scale}: output rel_err {rel_err(y, ref):.3e}")
    assert rel_err(y, ref) < 1e-4
    got = dict(dec.named_parameters())
    for key in DEC_KEYS:
        a, b = got[key].grad.double().cpu(), rp[key].grad
        print(f"  {key}: max {((a - b).abs().max() / b.abs().max()).item():.3e}  l2 {((a - b).norm() / b.norm()).item():.3e}")
    assert_grad_close(code.grad, rcode.grad, "code")
    for key in DEC_KEYS:
        assert_grad_close(got[key].grad, rp[key].grad, key)


def test_fused_decoder_keeps_no_wide_tensor(cuda):
    """B = 16: forward + backward of the fused decoder allocate less than ONE (B * 6400) x 512 fp32 tensor, the library's own
    workspace included (its tag is dropped first, so the buffer is allocated inside the measured window)."""
    from a3vt_amd import ops
    batch = 16
    dec = _decoder(cuda, fused=True)
    code = torch.randn(batch, 512, generator=torch.Generator().manual_seed(3)).to(cuda).requires_grad_(True)
    dy = torch.ones(batch, 3, 6400, device=cuda)
    for key in [k for k in ops._WORKSPACES if k[0] == "fold"]:
        del ops._WORKSPACES[key]
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    dec(code).backward(dy)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    wide = batch * 6400 * 512 * 4
    print(f"\nfused decoder B=16 forward + backward: peak {peak / 1e6:.1f} MB above the baseline (one wide tensor: {wide / 1e6:.1f} MB)")
    assert peak < wide


def test_fused_decoder_repeatable_and_batch_invariant(cuda):
    dec = _decoder(cuda, fused=True, seed=2)
    code0 = torch.randn(16, 512, generator=torch.Generator().manual_seed(4)).to(cuda)
    dy = _smooth_dy(16, 6400).float().to(cuda).transpose(2, 1)
    runs = []
    for _ in range(2):
        dec.zero_grad(set_to_none=True)
        code = code0.clone().requires_grad_(True)
        y = dec(code)
        y.backward(dy)
        runs.append([y.detach().clone(), code.grad.clone()] + [p.grad.clone() for p in dec.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    with torch.no_grad():
        assert torch.equal(dec(code0[5:6])[0], runs[0][0][5])
