"""ONE fused FoldingNet fold (``ops.fold`` on ``a3vt_fold_fwd/bwd``, csrc/fold.hip) at the edges of its host plan and kernels, against
an fp64 restatement on the CPU (``fold_ref.fold_restated``, gradients from fp64 autograd), for k = 2 and k = 3.

Inputs: the convs of a fresh ``_Fold(512 + k)`` (torch's default init, fixed seed), code ~ N(0, 1), ``g`` random and NOT the lattice
(U(-0.5, 0.5) for k = 2; N(0, 0.3) with a gradient for k = 3), dy ~ N(0, 1) with mixed signs: a wrong sign, a dropped row or a
permuted column in a cancelling sum is not scaled down by a coherent part.  ``dg`` is compared directly.

Shapes (``CASES``) and what each reaches: ``test_case_list_reaches_every_edge`` recomputes the rule of ``fold_plan`` in Python and
asserts, without a device, that the list hits a forward tile with several samples, partial 32-row tiles, an uneven ``tpc`` split,
empty dW2 groups and ``batch > 256``.

Tolerances are measured against a yardstick, not invented: torch's own unfused fp32 ``_Fold`` on the GPU runs on the same inputs and
its error against fp64 is computed in the same test; the fused kernel must stay within 4 x that error (both are fp32 chains over
k = 512; the 4 x pays for a different, equally valid summation order), max-norm relative to max|ref| for y, relative L2 for each
gradient, with an absolute floor of 8 * 2^-24 * sqrt(512) = 1.08e-5 relative for the cases where torch happens to be nearly exact.

ReLU kinks: with a random dy a unit whose pre-activation sits within rounding of 0 can legitimately flip.  For every shape up to
(7, 20) the seed (``SEEDS``, found by a search on the CPU: 44 of 64 seeds tried at the shapes of 140 rows and more qualify, about
4e-6 per unit) is one for which the fp64 reference has no pre-activation with |z| < 1e-6 max|z| in either layer; the test asserts that on the reference side, and then requires ALL elements
of every gradient within ``assert_grad_close``'s 1e-3 of max|ref|.  (300, 40) and (128, 150) have too many units for that: there the
outlier share is capped at 1e-3 (for the yardstick too) and the L2 bound applies.  Their seeds keep the reference 1e-7 from every
kink (``KINK_LARGE``): with an arbitrary seed torch's fp32 chain on the CPU flips a unit in about every other run, and ONE flip
moves an element of a 512-element gradient (conv2.bias) by 1e-2 of the max, outside the cap (seen at seed 1, k = 2, (300, 40)).

Further: a sample's forward alone and inside a batch (the sample that starts mid-tile), two runs giving the same bits, a workspace
left by a larger call / a fresh one / one filled with NaN giving the same bits (nothing reads masks or partials of an earlier call;
empty dW2 groups write their zeros), the refusal of a k = 2 ``g`` that wants a gradient, and NaN inputs: the fold's three ReLUs keep
a NaN as ``nn.ReLU`` does, so the NaN pattern of the output equals the unfused module's and the other samples keep their bits.

Observed on the MI355X, worst over the 22 cases (every case is in the table at the end of this file): fused error / torch's error
y 3.93 (at k = 2, (1, 1), where torch is nearly exact: 2.2e-7 against 5e-8), code 2.63, g 1.74, conv1.weight 2.34 / 2.34,
conv1.bias 2.40, conv2.weight 1.92, conv2.bias 2.63, conv3.weight 2.05, conv3.bias 2.96; largest errors: fused 1.45e-6 (y) and
9.3e-7 (gradients), torch 7.6e-7 and 9.1e-7; fused error / bound at most 0.134: 4 x torch's error stays below the floor in every
case, so the floor is the bound that holds.  No element of any gradient outside 1e-3 of the max, at the large shapes either."""
import functools
import types

import pytest
import torch

from fold_ref import CONV_KEYS, fold_restated, fp64_leaf
from helpers import assert_grad_close

gpu = pytest.mark.gpu

CASES = [(1, 1), (2, 31), (2, 32), (2, 33), (3, 63), (3, 64), (3, 65), (70, 1), (7, 20), (300, 40), (128, 150)]      # (batch, points)
LARGE = [(300, 40), (128, 150)]          # too many units for a kink-free seed: the outlier form of the gradient check
KS = [2, 3]
FLOOR = 8 * 2.0 ** -24 * 512 ** 0.5      # relative; see the module docstring
KINK = 1e-6                              # no reference pre-activation closer to 0 than this, relative to the layer's max |z|
# seed of a case's inputs (code, g, dy): for the small shapes the first that meets the kink condition (searched on the CPU from 1)
SEEDS = {(k, *c): 1 for k in KS for c in CASES + [(3, 33)]}       # ((3, 33): the bit-identity and NaN tests)
SEEDS[(2, 70, 1)] = 2
# The large shapes cannot meet KINK (1.2e7 to 2e7 units), but a seed need not be left to chance either: an fp32 z2 is a sum of 512
# products, off by about sqrt(512) * 2^-24 * |product| = 2^-24 * rms(z2), 1.3e-8 of max |z2| = 4.5 rms.  A reference margin of 1e-7
# puts every unit seven such deviations from its kink, for torch's fp32 module and for the kernel alike (one seed in 70 to 1000).
KINK_LARGE = 1e-7
SEEDS.update({(2, 300, 40): 3, (2, 128, 150): 53, (3, 300, 40): 104, (3, 128, 150): 1156})


def plan(batch, points):
    """The rule of ``fold_plan`` (csrc/fold.hip) and of the kernels' tiling, restated."""
    tp = (points + 31) // 32
    want = 256 // batch
    want = min(max(want, 1), tp)
    tpc = (tp + want - 1) // want
    chunks = (tp + tpc - 1) // tpc
    ntiles = batch * tp
    groups = min(ntiles, 64)
    per = (ntiles + groups - 1) // groups
    m = batch * points
    fwd_tiles = (m + 63) // 64
    return types.SimpleNamespace(
        tp=tp, want=want, tpc=tpc, chunks=chunks, ntiles=ntiles, groups=groups, per=per, fwd_tiles=fwd_tiles,
        split=[min(tpc, tp - c * tpc) for c in range(chunks)],                       # tiles of each workgroup of a sample
        empty_groups=[grp for grp in range(groups) if grp * per >= ntiles],           # dW2 row groups without a tile
        last_tile_rows=points - 32 * (tp - 1),
        last_fwd_rows=m - 64 * (fwd_tiles - 1),
        samples_per_fwd_tile=[(min(m, 64 * t + 64) - 1) // points - (64 * t) // points + 1 for t in range(fwd_tiles)])


def test_case_list_reaches_every_edge():
    """CPU only: a later edit of ``CASES`` cannot quietly lose an edge."""
    pl = {c: plan(*c) for c in CASES}
    assert any(max(p.samples_per_fwd_tile) >= 2 for p in pl.values())                 # a forward tile with two or more samples
    assert any(p.last_tile_rows < 32 for p in pl.values())                            # a partial 32-row tile
    assert any(p.tpc > 1 and len(set(p.split)) > 1 for p in pl.values())              # tpc > 1 with an uneven split
    assert any(p.empty_groups for p in pl.values())                                   # an empty dW2 group
    assert any(b > 256 for b, _ in CASES)                                             # 256 / batch == 0
    # and each row of the table
    p = pl[(1, 1)]
    assert (p.groups, p.ntiles, p.last_tile_rows, p.last_fwd_rows) == (1, 1, 1, 1)
    assert [pl[(2, n)].last_tile_rows for n in (31, 32, 33)] == [31, 32, 1] and [pl[(2, n)].tp for n in (31, 32, 33)] == [1, 1, 2]
    assert pl[(2, 31)].samples_per_fwd_tile == [2] and pl[(2, 32)].samples_per_fwd_tile == [2]
    assert pl[(2, 33)].samples_per_fwd_tile == [2, 1] and pl[(2, 33)].last_fwd_rows == 2
    assert [pl[(3, n)].fwd_tiles for n in (63, 64, 65)] == [3, 3, 4] and pl[(3, 64)].samples_per_fwd_tile == [1, 1, 1]
    assert pl[(3, 63)].samples_per_fwd_tile == [2, 2, 1] and pl[(3, 65)].last_fwd_rows == 3
    p = pl[(70, 1)]
    assert p.samples_per_fwd_tile == [64, 6] and p.ntiles == 70 and p.per == 2 and p.empty_groups == list(range(35, 64))
    p = pl[(7, 20)]
    assert max(p.samples_per_fwd_tile) >= 4 and p.last_tile_rows == 20 and p.tp == 1
    p = pl[(300, 40)]
    assert 256 // 300 == 0 and (p.want, p.tpc, p.chunks, p.ntiles, p.per) == (1, 2, 1, 600, 10) and p.empty_groups == [60, 61, 62, 63]
    p = pl[(128, 150)]
    assert (p.want, p.tp, p.tpc, p.chunks, p.split, p.last_tile_rows) == (2, 5, 3, 2, [3, 2], 22)


# ---- the cases: inputs and the fp64 reference, computed once and never modified -------------------------------------------------------
def _fold_module(k):
    from a3vt_amd.pterotactyl.reconstruction.autoencoder import model as am
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(40 + k)
        return am._Fold(512 + k)                 # torch's default Conv1d initialisation, as the decoder's folds


def make_inputs(k, batch, points, seed):
    gen = torch.Generator().manual_seed(seed)
    code = torch.randn(batch, 512, generator=gen)
    g = torch.rand(batch, points, 2, generator=gen) - 0.5 if k == 2 else 0.3 * torch.randn(batch, points, 3, generator=gen)
    dy = torch.randn(batch, points, 3, generator=gen)
    return code, g, dy


def _quantities(y, code, g, params):
    """What a run is compared on, under one set of names: y, the input gradients, the parameter gradients (conv1.weight in its
    two slices, which the fused path produces by different routes)."""
    q = {"y": y.detach(), "code.grad": code.grad}
    if g.grad is not None:
        q["g.grad"] = g.grad
    for key in CONV_KEYS:
        grad = params[key].grad
        if key == "conv1.weight":
            q["conv1.weight.grad[:, :512]"], q["conv1.weight.grad[:, 512:]"] = grad[:, :512], grad[:, 512:]
        else:
            q[key + ".grad"] = grad
    return q


def reference(k, code, g, dy, state):
    """fp64 on the CPU -> the quantities and the kink margin min |z| / max |z| over the two layers."""
    code, g = fp64_leaf(code), fp64_leaf(g)
    p = {key: fp64_leaf(v) for key, v in state.items()}
    y, z1, z2 = fold_restated(code, g, p)
    y.backward(dy.double())
    if k == 2:
        g.grad = None
    margin = min((z.detach().abs().min() / z.detach().abs().max()).item() for z in (z1, z2))
    return _quantities(y, code, g, p), margin


@functools.lru_cache(maxsize=None)
def case(k, batch, points):
    state = {key: v.detach().clone() for key, v in _fold_module(k).state_dict().items()}
    code, g, dy = make_inputs(k, batch, points, SEEDS[(k, batch, points)])
    ref, margin = reference(k, code, g, dy, state)
    return types.SimpleNamespace(k=k, state=state, code=code, g=g, dy=dy, ref=ref, margin=margin)


def _run(c, cuda, fused, code=None, g=None, state=None, backward=True):
    """Forward (+ backward) of the fold on the GPU: the fused kernels, or torch's unfused fp32 module on cat(code, g)."""
    from a3vt_amd import ops
    mod = _fold_module(c.k)
    mod.load_state_dict(c.state if state is None else state)
    mod = mod.to(cuda)
    code = (c.code if code is None else code).to(cuda).clone().requires_grad_(backward)            # (never the case's own tensors)
    g = (c.g if g is None else g).to(cuda).clone().requires_grad_(backward and c.k == 3)
    points = g.size(1)
    with torch.set_grad_enabled(backward):
        if fused:
            y = ops.fold(code, g, mod.conv1, mod.conv2, mod.conv3)
        else:
            y = mod(torch.cat((code[:, :, None].expand(-1, -1, points), g.transpose(2, 1)), dim=1)).transpose(2, 1)
    if not backward:
        return y
    y.backward(c.dy.to(cuda))
    return _quantities(y, code, g, dict(mod.named_parameters()))


def _error(name, got, ref):
    d = got.detach().double().cpu() - ref
    if name == "y":
        return (d.abs().max() / ref.abs().max()).item()
    return (d.norm() / ref.norm()).item()


# ---- against fp64, with torch's fp32 module as the yardstick ------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("batch,points", CASES)
@pytest.mark.parametrize("k", KS)
def test_one_fold_against_fp64(cuda, k, batch, points):
    c = case(k, batch, points)
    small = (batch, points) not in LARGE
    assert c.margin >= (KINK if small else KINK_LARGE), \
        f"seed {SEEDS[(k, batch, points)]}: the reference has a pre-activation at {c.margin:.2e} of the max"
    fused, plain = _run(c, cuda, True), _run(c, cuda, False)
    assert set(fused) == set(c.ref) == set(plain)
    assert ("g.grad" in fused) == (k == 3)
    print(f"\nfold k={k} B={batch} P={points}: kink margin {c.margin:.2e}")
    failures = []
    for name, ref in c.ref.items():
        assert fused[name].shape == ref.shape, name
        e_f, e_t = _error(name, fused[name], ref), _error(name, plain[name], ref)
        bound = max(4.0 * e_t, FLOOR)
        print(f"  {name:28s} fused {e_f:.3e}  torch fp32 {e_t:.3e}  ratio {e_f / max(e_t, 1e-300):6.2f}  fused / bound {e_f / bound:.3f}")
        if not e_f <= bound:
            failures.append(f"{name}: fused {e_f:.3e} > max(4 x {e_t:.3e}, {FLOOR:.2e})")
    assert not failures, "; ".join(failures)
    for name, ref in c.ref.items():
        if name != "y":
            assert_grad_close(fused[name], ref, name, outlier_frac=0.0 if small else 1e-3)
            if not small:
                assert_grad_close(plain[name], ref, "torch fp32 " + name)         # the yardstick stays inside the cap too


# ---- bits ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("batch,points", [(3, 33), (70, 1)])
@pytest.mark.parametrize("k", KS)
def test_sample_alone_equals_sample_in_batch(cuda, k, batch, points):
    """Sample 1 starts in the middle of a forward tile (row 33; row 1 of a tile of 64 samples).  The kernels see a sample through its
    row of ``bias_s`` and its points: on the batch's own ``bias_s`` row the sample alone gives the bits it has inside the batch, always.
    ``bias_s`` itself is a torch ``addmm`` in ``ops.fold``, and torch picks its product by shape: on the MI355X the row of sample 1
    computed alone differs from its row in the batch of 70 by 1.5e-6 (not in the batch of 3), so the whole of ``ops.fold`` is held to
    the same bits where torch's own product is, and that is asserted rather than assumed."""
    from a3vt_amd import ops
    c = case(k, batch, points)
    mod = _fold_module(k)
    mod.load_state_dict(c.state)
    mod = mod.to(cuda)
    code, g = c.code.to(cuda), c.g.to(cuda)
    with torch.no_grad():
        whole = ops.fold(code, g, mod.conv1, mod.conv2, mod.conv3)
        w1 = mod.conv1.weight.squeeze(-1)
        bias_s = torch.addmm(mod.conv1.bias, code, w1[:, :512].t())                   # as ops.fold forms it
        rest = (w1[:, 512:], mod.conv2.weight.squeeze(-1), mod.conv2.bias, mod.conv3.weight.squeeze(-1), mod.conv3.bias)
        assert torch.equal(ops.FoldFn.apply(bias_s, g, *rest), whole)
        row = ops.FoldFn.apply(bias_s[1:2].contiguous(), g[1:2].contiguous(), *rest)
        assert torch.equal(row[0], whole[1]), "the kernel's result for a sample depends on the batch around it"
        alone = ops.fold(code[1:2], g[1:2].contiguous(), mod.conv1, mod.conv2, mod.conv3)
        same_bias = torch.equal(torch.addmm(mod.conv1.bias, code[1:2], w1[:, :512].t()), bias_s[1:2])
        print(f"\nk={k} B={batch} P={points}: torch's bias_s row alone == in the batch: {same_bias}")
        if same_bias:
            assert torch.equal(alone[0], whole[1])
        else:       # two valid fp32 evaluations of the same row: not the same bits, the same value
            diff = ((alone[0] - whole[1]).abs().max() / whole.abs().max()).item()
            print(f"  ops.fold alone against in the batch: {diff:.3e} of max |y| (floor {FLOOR:.2e})")
            assert diff <= FLOOR


@gpu
@pytest.mark.parametrize("k", KS)
def test_two_runs_give_the_same_bits(cuda, k):
    c = case(k, 300, 40)
    first, second = _run(c, cuda, True), _run(c, cuda, True)
    for name in first:
        assert torch.equal(first[name], second[name]), name


@gpu
@pytest.mark.parametrize("k", KS)
def test_stale_workspace_is_not_read(cuda, k):
    """(70, 1) on the workspace a (300, 40) call left behind, on a fresh one, and on one filled with NaN: the same bits.  The masks
    and partials are written before they are read, the 29 empty dW2 groups included."""
    from a3vt_amd import ops
    _run(case(k, 300, 40), cuda, True)
    c = case(k, 70, 1)
    stale = _run(c, cuda, True)
    for key in [key for key in ops._WORKSPACES if key[0] == "fold"]:
        del ops._WORKSPACES[key]
    fresh = _run(c, cuda, True)
    keys = [key for key in ops._WORKSPACES if key[0] == "fold"]
    assert keys
    for key in keys:
        ops._WORKSPACES[key].fill_(float("nan"))
    poisoned = _run(c, cuda, True)
    for name in stale:
        assert torch.equal(stale[name], fresh[name]), name
        assert torch.equal(stale[name], poisoned[name]), name


@gpu
def test_k2_lattice_with_a_gradient_is_refused(cuda):
    from a3vt_amd import ops
    c = case(2, 2, 31)
    mod = _fold_module(2).to(cuda)
    g = c.g.to(cuda).requires_grad_(True)
    with pytest.raises(RuntimeError, match="the k = 2 lattice has no gradient path"):
        ops.fold(c.code.to(cuda), g, mod.conv1, mod.conv2, mod.conv3)


# ---- NaN through the ReLUs ------------------------------------------------------------------------------------------------------------
def _nan_pattern_case(c, cuda, code=None, g=None, state=None):
    fused = _run(c, cuda, True, code=code, g=g, state=state, backward=False)
    plain = _run(c, cuda, False, code=code, g=g, state=state, backward=False)
    assert torch.equal(torch.isnan(fused), torch.isnan(plain)), "the NaN pattern differs from the unfused module's"
    return fused


@gpu
@pytest.mark.parametrize("k", KS)
def test_nan_in_a_code_stays_in_its_sample(cuda, k):
    c = case(k, 3, 33)
    clean = _run(c, cuda, True, backward=False)
    assert torch.isfinite(clean).all()
    code = c.code.clone()
    code[1, 77] = float("nan")
    y = _nan_pattern_case(c, cuda, code=code)
    assert torch.isnan(y[1]).all()
    assert torch.equal(y[0], clean[0]) and torch.equal(y[2], clean[2])


@gpu
def test_nan_in_a_point_stays_in_its_row(cuda):
    c = case(3, 3, 33)
    clean = _run(c, cuda, True, backward=False)
    g = c.g.clone()
    g[1, 5, 2] = float("nan")
    y = _nan_pattern_case(c, cuda, g=g)
    want = torch.zeros(3, 33, 3, dtype=torch.bool, device=cuda)
    want[1, 5] = True
    assert torch.equal(torch.isnan(y), want)
    assert torch.equal(y[~want], clean[~want])


@gpu
@pytest.mark.parametrize("k", KS)
def test_nan_in_a_weight_reaches_every_output(cuda, k):
    c = case(k, 3, 33)
    state = {key: v.clone() for key, v in c.state.items()}
    state["conv2.weight"][300, 17, 0] = float("nan")
    y = _nan_pattern_case(c, cuda, state=state)
    assert torch.isnan(y).all()


# ---- observed on the MI355X: fused / torch fp32 error against fp64 per case, in units of 1e-7 (max-norm for y, relative L2 for the rest;
# dW1c / dW1g: the code and the point slice of conv1.weight.grad) -------------------------------------------------------------------
#   k=2 (1, 1):     y 2.2/0.5 dcode 3.4/4.4 dW1c 3.0/3.0 dW1g 3.0/3.0 db1 3.0/3.0 dW2 2.3/2.3 db2 0.4/0.3 dW3 3.3/2.7 db3 0.0/0.0
#   k=2 (2, 31):    y 4.9/3.9 dcode 3.0/3.3 dW1c 2.6/2.4 dW1g 5.7/5.6 db1 2.7/2.5 dW2 2.3/2.2 db2 1.1/0.6 dW3 3.1/2.7 db3 0.6/0.3
#   k=2 (2, 32):    y 4.9/3.9 dcode 4.9/6.4 dW1c 4.7/4.6 dW1g 4.1/4.1 db1 5.0/5.0 dW2 2.6/2.9 db2 1.6/1.1 dW3 5.5/4.2 db3 1.3/0.4
#   k=2 (2, 33):    y 4.9/3.9 dcode 6.6/9.1 dW1c 6.3/6.5 dW1g 2.9/2.9 db1 7.5/7.5 dW2 3.3/4.1 db2 2.9/2.0 dW3 9.3/6.2 db3 0.8/3.4
#   k=2 (3, 63):    y 5.5/4.4 dcode 3.3/3.9 dW1c 2.8/3.2 dW1g 2.8/3.1 db1 2.9/2.8 dW2 2.4/2.7 db2 1.3/0.8 dW3 3.8/3.0 db3 0.7/1.0
#   k=2 (3, 64):    y 5.5/4.4 dcode 2.9/3.2 dW1c 2.5/2.7 dW1g 3.7/3.9 db1 2.5/2.4 dW2 2.4/2.5 db2 1.1/0.7 dW3 3.3/2.5 db3 0.4/0.4
#   k=2 (3, 65):    y 5.5/4.4 dcode 3.5/4.1 dW1c 3.2/3.3 dW1g 3.9/3.9 db1 3.0/3.0 dW2 2.3/2.4 db2 1.3/0.8 dW3 3.6/2.7 db3 0.5/0.5
#   k=2 (70, 1):    y 6.5/3.5 dcode 4.1/1.6 dW1c 3.1/1.3 dW1g 2.5/1.2 db1 3.2/1.3 dW2 4.3/2.3 db2 1.4/0.9 dW3 5.7/2.8 db3 0.8/1.8
#   k=2 (7, 20):    y 4.5/4.4 dcode 3.6/4.3 dW1c 3.1/3.0 dW1g 2.9/3.0 db1 3.2/3.3 dW2 2.4/2.5 db2 1.4/0.9 dW3 4.6/3.3 db3 0.7/0.5
#   k=2 (300, 40):  y 8.1/4.8 dcode 4.3/4.2 dW1c 3.8/4.7 dW1g 3.4/4.3 db1 3.0/3.1 dW2 4.6/3.2 db2 2.5/1.3 dW3 6.1/3.7 db3 0.5/1.7
#   k=2 (128, 150): y 8.2/5.8 dcode 4.4/4.1 dW1c 3.6/5.6 dW1g 3.7/5.2 db1 3.9/3.6 dW2 5.4/3.9 db2 3.4/1.5 dW3 7.4/4.5 db3 3.2/1.5
#   k=3 (1, 1):     y 3.9/5.7 dcode 3.4/4.0 dg 2.8/5.2 dW1c 3.0/2.9 dW1g 3.0/2.9 db1 3.0/2.9 dW2 2.4/2.2 db2 0.4/0.3 dW3 3.9/2.5 db3 0.0/0.0
#   k=3 (2, 31):    y 9.1/6.5 dcode 3.0/3.2 dg 4.2/4.3 dW1c 2.5/2.3 dW1g 3.5/3.4 db1 2.1/2.0 dW2 2.2/2.2 db2 0.7/0.5 dW3 2.6/2.2 db3 0.3/0.3
#   k=3 (2, 32):    y 9.1/6.5 dcode 3.6/4.1 dg 3.3/4.3 dW1c 3.1/2.8 dW1g 3.3/3.0 db1 3.4/3.0 dW2 2.5/2.5 db2 1.3/0.8 dW3 3.8/3.1 db3 0.5/1.4
#   k=3 (2, 33):    y 9.1/6.7 dcode 5.5/7.3 dg 3.0/4.3 dW1c 5.1/5.1 dW1g 3.2/3.3 db1 5.8/5.5 dW2 3.0/4.1 db2 2.1/1.6 dW3 8.0/6.6 db3 2.9/2.3
#   k=3 (3, 63):    y 14.5/7.5 dcode 3.6/4.1 dg 3.1/3.9 dW1c 3.3/3.4 dW1g 3.6/3.7 db1 3.1/3.0 dW2 2.5/2.5 db2 1.3/0.8 dW3 3.8/2.5 db3 0.9/0.7
#   k=3 (3, 64):    y 14.5/7.5 dcode 3.5/3.9 dg 3.0/4.0 dW1c 2.9/2.9 dW1g 3.2/3.3 db1 3.2/2.9 dW2 2.8/2.7 db2 1.7/0.9 dW3 4.9/3.5 db3 1.7/1.1
#   k=3 (3, 65):    y 14.5/7.5 dcode 3.2/3.7 dg 2.9/3.9 dW1c 2.9/3.1 dW1g 3.6/3.7 db1 3.0/2.8 dW2 2.5/2.5 db2 1.4/0.8 dW3 3.8/2.7 db3 1.0/1.7
#   k=3 (70, 1):    y 7.7/3.9 dcode 4.1/1.6 dg 2.6/1.5 dW1c 3.1/1.3 dW1g 3.2/1.4 db1 2.7/1.1 dW2 4.0/2.1 db2 1.4/0.6 dW3 4.4/2.2 db3 0.5/0.7
#   k=3 (7, 20):    y 6.3/5.3 dcode 4.1/5.1 dg 2.5/3.7 dW1c 3.7/3.6 dW1g 3.1/3.1 db1 3.7/3.5 dW2 2.4/2.4 db2 1.0/0.8 dW3 4.5/3.2 db3 0.5/0.5
#   k=3 (300, 40):  y 9.4/5.6 dcode 4.2/4.1 dg 2.5/3.8 dW1c 3.8/4.8 dW1g 3.6/4.6 db1 3.3/3.2 dW2 4.7/3.2 db2 2.4/1.4 dW3 6.2/3.9 db3 2.2/1.1
#   k=3 (128, 150): y 9.2/5.9 dcode 4.4/4.2 dg 2.5/3.7 dW1c 3.6/5.5 dW1g 3.9/5.8 db1 3.6/3.2 dW2 5.1/3.6 db2 3.3/1.2 dW3 6.6/4.6 db3 2.6/1.8
