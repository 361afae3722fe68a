"""Two small kernels of csrc/gcn_csr.hip on their own: ``a3vt_check_finite`` (the deferred NaN trap of the layer loop,
vision/model.py:326 in the reference) and ``a3vt_vertex_update`` with ``ops.VertexUpdateFn``'s backward (vision/model.py:250,270,283).
Whole-model tests only ever see the flag stay 0 and the update inside a training step."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GRID = 2048 * 256                      # check_finite's largest grid: beyond it a thread takes a second element
SIZES = [1, 63, 64, 65, 255, 257, GRID + 3]
NEIGHBOUR = 0x5A5A5A5A


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def base(dev):
    """One buffer for every size, a view of it starting one element off a 16-byte boundary included."""
    g = torch.Generator().manual_seed(0)
    t = torch.randn(GRID + 8, generator=g).to(dev)
    assert t.data_ptr() % 16 == 0
    return t


def _flag(dev, start=0):
    cells = torch.tensor([NEIGHBOUR, start, NEIGHBOUR], dtype=torch.int32, device=dev)
    return cells, cells[1:2]


def _fires(t, dev, start=0):
    from a3vt_amd import ops
    cells, flag = _flag(dev, start)
    ops.check_finite(t, flag)
    got = cells.tolist()
    assert got[0] == NEIGHBOUR and got[2] == NEIGHBOUR, "the flag's neighbours were written"
    assert got[1] in (0, 1)
    return got[1]


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_check_finite_fires_for_every_placement(base, dev, n, shift):
    t = base[shift:shift + n]
    assert t.data_ptr() % 16 == 4 * shift and t.is_contiguous()
    assert _fires(t, dev) == 0                                         # the clean tensor first
    for at in sorted({0, n - 1} | ({GRID} if n > GRID else set())):
        for bad in (float("nan"), float("inf"), float("-inf")):
            keep = t[at].item()
            t[at] = bad
            assert _fires(t, dev) == 1, (n, at, bad)
            t[at] = keep
    assert _fires(t, dev) == 0 and bool(torch.isfinite(base).all())    # and the buffer is as it was


@pytest.mark.parametrize("n", [7, 65, GRID + 3])
def test_check_finite_stays_quiet_on_finite_extremes(dev, n):
    fmax, tiny = float(np.finfo(np.float32).max), 2.0 ** -149
    vals = torch.tensor([fmax, -fmax, tiny, -tiny, 0.0, -0.0, 1e38], dtype=torch.float32)
    assert vals[2].item() == tiny and vals[2].item() > 0 and bool(torch.isfinite(vals).all())
    t = vals.repeat(-(-n // 7))[:n].contiguous().to(dev)
    assert _fires(t, dev) == 0


def test_check_finite_ors_into_the_flag(base, dev):
    t = base[:300]
    assert _fires(t, dev, start=1) == 1                                # a clean call leaves a raised flag raised
    t[299] = float("nan")
    assert _fires(t, dev, start=1) == 1
    t[299] = 0.0
    assert _fires(t, dev, start=0) == 0


SHAPES = [(1, 1, 1), (1, 1, 0), (3, 85, 0), (3, 85, 85), (3, 85, 40), (2, 1001, 1000)]


def _inputs(dev, B, N, nv, seed):
    g = torch.Generator().manual_seed(seed)
    verts = (torch.randn(B, N, 3, generator=g) * 10.0 ** torch.randint(-3, 3, (B, N, 1), generator=g).float()).to(dev)
    update = (torch.randn(B, N, 3, generator=g) * 10.0 ** torch.randint(-3, 3, (B, N, 1), generator=g).float()).to(dev)
    update[:, nv:] = float("nan")                  # rows the kernel must never read into the result
    return verts, update


@pytest.mark.parametrize("B,N,nv", SHAPES)
def test_vertex_update_forward_is_one_fp32_add(dev, B, N, nv):
    from a3vt_amd import ops
    verts, update = _inputs(dev, B, N, nv, 1)
    keep_v, keep_u = verts.clone(), update.clone()
    out = ops.VertexUpdateFn.apply(verts, update, nv)
    want = verts.clone()
    want[:, :nv] += update[:, :nv]
    assert out.shape == verts.shape and out.data_ptr() != verts.data_ptr()
    assert torch.equal(out, want) and bool(torch.isfinite(out).all())
    assert torch.equal(verts, keep_v) and torch.equal(update.view(torch.int32), keep_u.view(torch.int32))


@pytest.mark.parametrize("B,N,nv", SHAPES)
def test_vertex_update_backward(dev, B, N, nv):
    from a3vt_amd import ops
    verts, update = _inputs(dev, B, N, nv, 2)
    verts.requires_grad_(True)
    update.requires_grad_(True)
    out = ops.VertexUpdateFn.apply(verts, update, nv)
    gin = torch.randn(B, N, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    keep = gin.clone()
    out.backward(gin)
    want_u = keep.clone()
    want_u[:, nv:] = 0
    assert torch.equal(verts.grad, keep) and torch.equal(update.grad, want_u)
    assert torch.equal(gin, keep), "the incoming gradient was modified in place"
