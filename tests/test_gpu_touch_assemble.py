"""``ops.touch_assemble`` (``a3vt_touch_assemble``, csrc/touch_assemble.hip) on the GPU against the NumPy loop of
``touch_assemble_util.reference``.  Every comparison is of bits (``.view(torch.int32)``): the kernel moves words, and the tables hold
NaNs with payloads, the infinities and -0.0.

Shapes (K, E, A, F, G, C): the minimum; (3, 2, 5, 4, 5, 25), whose blocks are 75 floats = 300 bytes, so that only every fourth one
starts on a 16-byte boundary — with the inputs 4, 8 and 12 bytes into larger buffers as well; the production shape; the ``finger``
topology."""
import numpy as np
import pytest
import torch

import touch_assemble_util as ta
from a3vt_amd import ops

pytestmark = pytest.mark.gpu

MINIMUM, ODD, PRODUCTION, FINGER = (1, 1, 1, 1, 1, 1), (3, 2, 5, 4, 5, 25), (50, 3, 50, 4, 5, 25), (7, 3, 4, 1, 5, 25)
CASES = [(MINIMUM, 0), (ODD, 0), (ODD, 2), (ODD, 4), (PRODUCTION, 3), (FINGER, 1)]


def bits(t):
    return t.contiguous().view(torch.int32).cpu()


def want_bits(a):
    return torch.from_numpy(a.view(np.int32))


def upload(a, cuda, offset_bytes=0):
    """``a`` on the device, ``offset_bytes`` (a multiple of 4) into a larger buffer whose other words are poison."""
    flat = torch.from_numpy(a.reshape(-1).view(np.int32).copy())
    pad = offset_bytes // 4
    buf = torch.full((flat.numel() + 8,), 0x7FC0DEAD, dtype=torch.int32, device=cuda)
    buf[pad:pad + flat.numel()] = flat.to(cuda)
    t = buf[pad:pad + flat.numel()].view(torch.float32 if a.dtype == np.float32 else torch.int32).view(a.shape)
    assert t.data_ptr() % 16 == (buf.data_ptr() + offset_bytes) % 16 and t.is_contiguous()
    return t


@pytest.fixture(scope="module")
def references():
    """Per (shape, slot): the inputs and the reference's words, computed once and never written."""
    out = {}
    for i, (shape, slot) in enumerate(CASES):
        arrays = ta.inputs(*shape, seed=40 + i)
        out[shape, slot] = (arrays, ta.reference(*arrays, slot))
    return out


@pytest.mark.parametrize("shape,slot", CASES, ids=lambda v: str(v))
def test_bits_against_the_numpy_loop(cuda, references, shape, slot):
    arrays, (want_c, want_m) = references[shape, slot]
    tensors = [upload(a, cuda) for a in arrays]
    kept = [t.clone() for t in tensors]
    ops.touch_assemble_launches(reset=True)
    charts, masks = ops.touch_assemble(*tensors, slot)
    assert ops.touch_assemble_launches() == {"calls": 1}                               # one call is one launch
    K, E, A, F, G, C = shape
    assert charts.shape == (K, E, F * G * C, 3) and masks.shape == (K, E, F * G * C, 1) and charts.is_cuda and masks.is_cuda
    assert torch.equal(bits(charts), want_bits(want_c)) and torch.equal(bits(masks), want_bits(want_m))
    again = ops.touch_assemble(*tensors, slot)                                         # the same bits on every call
    assert torch.equal(bits(again[0]), bits(charts)) and torch.equal(bits(again[1]), bits(masks))
    assert ops.touch_assemble_launches() == {"calls": 2}
    assert all(torch.equal(bits(t), bits(k)) for t, k in zip(tensors, kept))           # no input is written
    # candidates from the host (checked and uploaded) are the same call
    host = ops.touch_assemble(*tensors[:4], arrays[4].tolist(), slot)
    assert torch.equal(bits(host[0]), bits(charts)) and torch.equal(bits(host[1]), bits(masks))
    if shape != MINIMUM:
        assert np.isnan(want_c.view(np.float32)).any() and (want_m.view(np.float32) == 2).any()   # the case holds what it claims


@pytest.mark.parametrize("offset", [4, 8, 12])
def test_inputs_off_the_16_byte_boundary(cuda, references, offset):
    """The (3, 2, 5, 4, 5, 25) inputs 4, 8 and 12 bytes into larger buffers: every pointer 4-byte aligned and no more."""
    for slot in (0, 2, 4):
        arrays, (want_c, want_m) = references[ODD, slot]
        tensors = [upload(a, cuda, offset) for a in arrays]
        assert all(t.data_ptr() % 16 == offset for t in tensors)
        charts, masks = ops.touch_assemble(*tensors, slot)
        assert torch.equal(bits(charts), want_bits(want_c)) and torch.equal(bits(masks), want_bits(want_m)), (offset, slot)


def test_actions_outside_the_table_give_zero_blocks(cuda, references):
    """A device candidate tensor is not checked on the host: -1 and A give a zero chart and mask 0 in their blocks, and every other
    block is what it was."""
    arrays, (plain_c, plain_m) = references[ODD, 2]
    K, E, A, F, G, C = ODD
    cand = arrays[4].copy()
    cand[0, 1], cand[2, 0] = -1, A
    want_c, want_m = ta.reference(*arrays[:4], cand, 2)
    tensors = [upload(a, cuda) for a in arrays[:4]]
    charts, masks = ops.touch_assemble(*tensors, torch.from_numpy(cand).to(cuda), 2)
    assert torch.equal(bits(charts), want_bits(want_c)) and torch.equal(bits(masks), want_bits(want_m))
    c6, m5 = bits(charts).view(K, E, F, G, C, 3), bits(masks).view(K, E, F, G, C)
    for k, e in ((0, 1), (2, 0)):
        assert not c6[k, e, :, 2].any() and not m5[k, e, :, 2].any()
    differs = (bits(charts) != want_bits(plain_c)).view(K, E, F, G, C * 3).any(-1)
    assert set(map(tuple, differs.nonzero().tolist())) <= {(k, e, f, 2) for k, e in ((0, 1), (2, 0)) for f in range(F)}
    with pytest.raises(ValueError, match="candidates outside"):                          # the same list from the host is refused
        ops.touch_assemble(*tensors, cand, 2)


def test_repeated_actions_and_shared_columns(cuda, references):
    """Candidates that repeat an action (rows 0 and 1 of every case are equal) get equal blocks."""
    arrays, _ = references[ODD, 0]
    assert (arrays[4][0] == arrays[4][1]).all()
    charts, masks = ops.touch_assemble(*[upload(a, cuda) for a in arrays], 0)
    assert torch.equal(bits(charts[0]), bits(charts[1])) and torch.equal(bits(masks[0]), bits(masks[1]))
    same = torch.zeros((4, 2), dtype=torch.int32, device=cuda) + 3                       # one action for everybody
    charts, _ = ops.touch_assemble(*[upload(a, cuda) for a in arrays[:4]], same, 0)
    assert all(torch.equal(bits(charts[0]), bits(charts[k])) for k in range(1, 4))
