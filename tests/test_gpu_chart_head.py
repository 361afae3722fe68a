"""GPU tests of ``a3vt_touch_chart_head`` (csrc/chart_head.hip) through ``ops.touch_chart_head``, against the fp64 emulation of
``chart_head_util.rows64`` (written for these tests): three ``Linear`` with ReLU after the first two, the template add,
``rot . v + pos``, the select on the code.

The cap.  The torch fp32 tail the kernel replaces (``ops._chart_head_torch``: the lines of ``Encoder.forward`` and ``touch_slots``)
differs from the fp64 values by ``e_torch``; two equally valid fp32 evaluations with different summation orders get 4 x that (the
cap ``conv5f`` is held to in ``test_gpu_touch_model.py``).  Per size n in 1, 15, 16, 17, 67: ``e_torch`` is the tail's largest error
on the same n views evaluated as one batch of n, and the kernel's largest error on those views must be at most 4 x it.  The tail's
error over all 67 views is held as a second cap beside it.  Views whose code is not 2 hold no rounded sum: they are compared exactly.

Measured on an MI355X: see the test's output (``-s``) and DESIGN.md's entry."""
import functools

import pytest
import torch

from chart_head_util import rows64

pytestmark = pytest.mark.gpu

SIZES = (1, 15, 16, 17, 67)          # one view; a tile less one, a tile, a tile and one; five tiles, the last with three rows
POOL = 67


@functools.lru_cache(maxsize=None)
def pool():
    """Seeded inputs of 67 views (CPU, never modified): features, the encoder's ``fc``, template, frames, codes, and the fp64 rows."""
    from a3vt_amd import mesh
    from a3vt_amd.pterotactyl.reconstruction.touch import model
    torch.manual_seed(0)
    fc = model.Encoder().fc
    g = torch.Generator().manual_seed(67)
    features = torch.randn(POOL, 512, generator=g) * 2.0
    rot = torch.randn(POOL, 3, 3, generator=g)                       # arbitrary, not symmetric: a transposed product shows
    pos = torch.randn(POOL, 3, generator=g) * 0.2
    code = torch.full((POOL,), 2, dtype=torch.int32)
    code[1::5] = 1                                                    # rows 1, 6, 11, 16, ...
    code[2::7] = 0                                                    # rows 2, 9, 16, ...: every batch of three or more has all codes
    template = torch.from_numpy(mesh.load_asset("touch_chart")[0]).float()
    return features, fc, template, rot, pos, code, rows64(features, fc, template, rot, pos, code)


@pytest.fixture(scope="module")
def dev(cuda):
    """The pool on the GPU, and ``e_torch``: (features, fc, template, rot, pos, code, want64, e_torch)."""
    import copy

    from a3vt_amd import ops
    features, fc, template, rot, pos, code, want = pool()
    fc_d = copy.deepcopy(fc).to(cuda)
    d = (features.to(cuda), fc_d, template.to(cuda), rot.to(cuda), pos.to(cuda), code.to(cuda))
    with torch.no_grad():
        charts, masks = ops._chart_head_torch(*d)
    tail = torch.cat((charts, masks), dim=-1).double().cpu()
    e_torch = (tail - want).abs().max().item()
    assert 0.0 < e_torch < 1e-4
    return d + (want, e_torch)


def head(dev, index, **kw):
    from a3vt_amd import ops
    features, fc, template, rot, pos, code = dev[:6]
    return ops.touch_chart_head(features[index], fc, template, rot[index], pos[index], code[index], **kw)


@pytest.mark.parametrize("n", SIZES)
def test_against_fp64(dev, n):
    from a3vt_amd import ops
    want, e_pool, code = dev[6][:n], dev[7], dev[5][:n].cpu()
    rows = head(dev, slice(0, n))
    assert rows.shape == (n, 25, 4) and rows.dtype == torch.float32
    got = rows.double().cpu()
    assert torch.isfinite(got).all()
    err = (got - want).abs().max().item()
    features, fc, template, rot, pos, code_d = dev[:6]
    with torch.no_grad():                                                      # the torch tail on the SAME n views, as one batch of n
        tail = torch.cat(ops._chart_head_torch(features[:n], fc, template, rot[:n], pos[:n], code_d[:n]), dim=-1).double().cpu()
    e_torch = (tail - want).abs().max().item()
    print(f"n={n}: kernel max err {err:.3e}, torch fp32 tail on the same {n} views {e_torch:.3e}: {err / e_torch:.2f} x "
          f"(on all 67 views {e_pool:.3e}: {err / e_pool:.2f} x)")
    assert e_torch > 0
    assert err <= 4 * e_torch, f"n={n}: {err:.3e} > 4 x {e_torch:.3e}"
    assert err <= 4 * e_pool, f"n={n}: {err:.3e} > 4 x {e_pool:.3e} (the tail's error on all 67 views)"
    assert torch.equal(got[code != 2], want[code != 2])                        # the position / zeros and the mask: no rounding
    assert torch.equal(got[..., 3], want[..., 3])
    if n >= 3:
        assert sorted(code.unique().tolist()) == [0, 1, 2]


def test_a_batch_of_code_0_and_codes_outside(dev):
    from a3vt_amd import ops
    features, fc, template, rot, pos, code = dev[:6]
    for n in (1, 17):
        rows = ops.touch_chart_head(features[:n], fc, template, rot[:n], pos[:n], torch.zeros(n, dtype=torch.int32, device=code.device))
        assert rows.shape == (n, 25, 4) and not rows.any()
    odd = torch.tensor([3, -1, 1 << 30, 2], dtype=torch.int32, device=code.device)
    rows = ops.touch_chart_head(features[:4], fc, template, rot[:4], pos[:4], odd)
    assert not rows[:3].any() and (rows[3, :, 3] == 2).all() and torch.equal(rows[3], head(dev, slice(3, 4))[0])


def test_batch_invariant_permutable_and_repeatable(dev):
    full = head(dev, slice(0, POOL))
    assert torch.equal(full, head(dev, slice(0, POOL))), "two calls differ"
    for i in (0, 3, 15, 16, 31, 64, 66):                                       # first / last rows of tiles, the ragged last tile
        alone = head(dev, slice(i, i + 1))
        assert torch.equal(alone[0].view(torch.int32), full[i].view(torch.int32)), f"view {i} alone differs from the same view in 67"
    for n in SIZES:
        assert torch.equal(head(dev, slice(0, n)), full[:n]), f"the first {n} views differ from the same views in 67"
    perm = torch.randperm(POOL, generator=torch.Generator().manual_seed(1)).to(full.device)
    assert torch.equal(head(dev, perm), full[perm]), "permuting the views does not permute the rows"


def test_nan_stays_in_its_view(dev):
    from a3vt_amd import ops
    features, fc, template, rot, pos, code = dev[:6]
    n = 20
    clean = head(dev, slice(0, n))
    code_h = code[:n].cpu()
    assert code_h[1] == 1 and code_h[2] == 0 and code_h[3] == 2 and code_h[17] == 2
    bad = features[:n].clone()
    bad[1, 7] = float("nan")                                                   # "no_touch"
    bad[2] = float("nan")                                                      # "no_intersection": all of its features
    rot_bad = rot[:n].clone()
    rot_bad[1] = float("nan")
    rot_bad[2] = float("nan")
    pos_bad = pos[:n].clone()
    pos_bad[2] = float("nan")                                                  # (code 0 takes nothing from the position either)
    rows = ops.touch_chart_head(bad, fc, template, rot_bad, pos_bad, code[:n])
    assert torch.isfinite(rows).all() and torch.equal(rows, clean)
    for i in (3, 17):                                                          # "touch": in the first tile, in the second
        bad = features[:n].clone()
        bad[i, 511] = float("nan")
        rows = ops.touch_chart_head(bad, fc, template, rot[:n], pos[:n], code[:n])
        assert torch.isnan(rows[i, :, :3]).all() and (rows[i, :, 3] == 2).all()
        others = [j for j in range(n) if j != i]
        assert torch.equal(rows[others], clean[others]), f"the NaN of view {i} reached another view"


def test_one_launch_and_the_slots(dev):
    from a3vt_amd import ops
    ops.chart_head_launches(reset=True)
    for calls, n in enumerate(SIZES):
        rows, charts, masks = head(dev, slice(0, n), want_slots=True)
        assert ops.chart_head_launches() == {"calls": 2 * calls + 1}          # one call, one launch, whatever n
        assert charts.shape == (n, 25, 3) and masks.shape == (n, 25, 1) and charts.is_contiguous() and masks.is_contiguous()
        assert torch.equal(rows[..., :3].view(torch.int32), charts.view(torch.int32)) and torch.equal(rows[..., 3:], masks)
        assert torch.equal(rows, head(dev, slice(0, n)))
    assert ops.chart_head_launches(reset=True) == {"calls": 2 * len(SIZES)} and ops.chart_head_launches() == {"calls": 0}


def test_views_off_a_16_byte_boundary_are_taken(dev):
    """A view into a larger tensor need not start on a 16-byte boundary; the entry point wants one, ``ops`` provides it."""
    from a3vt_amd import ops
    features, fc, template, rot, pos, code = dev[:6]
    n = 5
    store = torch.empty(n * 512 + 1, device=features.device)
    shifted = store[1:].view(n, 512)
    shifted.copy_(features[:n])
    assert shifted.data_ptr() % 16 == 4
    assert torch.equal(ops.touch_chart_head(shifted, fc, template, rot[:n], pos[:n], code[:n]), head(dev, slice(0, n)))
