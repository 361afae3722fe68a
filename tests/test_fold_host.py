"""CPU tests (no GPU, no compute) of the fused FoldingNet decoder's host side: the argument checks of ``a3vt_fold_fwd/bwd``
(an error code and a message, fake device addresses never dereferenced), the trainer's registration under the reference's module
name, the knob's effect on the model's parameters (none), and the trainer's error for a missing frozen model."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FAKE = ctypes.c_void_p(0x7F0000001000)       # a "device pointer": 16-byte aligned, never mapped on the host
FAKE_ODD = ctypes.c_void_p(0x7F0000001008)   # 8 mod 16
FAKE_BYTE = ctypes.c_void_p(0x7F0000001002)  # 2 mod 4


@pytest.fixture(scope="module")
def L():
    from a3vt_amd import lib
    return lib.load()


def _err(L):
    return L.a3vt_last_error().decode()


def _fwd(L, **kw):
    b, p = kw.get("batch", 2), kw.get("points", 100)
    need = kw.get("ws_bytes", L.a3vt_fold_workspace_bytes(max(b, 1), max(p, 1), 0))
    return L.a3vt_fold_fwd(kw.get("bias_s", FAKE), kw.get("g", FAKE), kw.get("k", 2), kw.get("w1g", FAKE), kw.get("w2", FAKE),
                           kw.get("b2", FAKE), kw.get("w3", FAKE), kw.get("b3", FAKE), b, p, kw.get("width", 512), kw.get("y", FAKE),
                           kw.get("ws", FAKE), need, None)


def _bwd(L, **kw):
    b, p = kw.get("batch", 2), kw.get("points", 100)
    need = kw.get("ws_bytes", L.a3vt_fold_workspace_bytes(max(b, 1), max(p, 1), 1))
    return L.a3vt_fold_bwd(kw.get("bias_s", FAKE), kw.get("g", FAKE), kw.get("k", 3), kw.get("w1g", FAKE), kw.get("w2", FAKE),
                           kw.get("b2", FAKE), kw.get("w3", FAKE), kw.get("dy", FAKE), b, p, kw.get("width", 512),
                           kw.get("dbias", FAKE), kw.get("dg", FAKE), kw.get("dw1g", FAKE), kw.get("dw2", FAKE), kw.get("db2", FAKE),
                           kw.get("dw3", FAKE), kw.get("db3", FAKE), kw.get("ws", FAKE), need, None)


def test_fold_workspace_sizes(L):
    wide = 16 * 6400 * 512 * 4
    assert 0 < L.a3vt_fold_workspace_bytes(16, 6400, 0) <= L.a3vt_fold_workspace_bytes(16, 6400, 1) < wide
    assert L.a3vt_fold_workspace_bytes(32, 6400, 1) < wide
    assert L.a3vt_fold_workspace_bytes(0, 6400, 1) == 0 and L.a3vt_fold_workspace_bytes(4, -1, 0) == 0
    for b, p in ((1, 1), (3, 1000), (300, 7), (1, 6400)):
        assert L.a3vt_fold_workspace_bytes(b, p, 1) > 0


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_fold_entry_points_refuse_bad_arguments(L, call):
    for bad in (dict(bias_s=None), dict(g=None), dict(w1g=None), dict(w2=None), dict(b2=None), dict(w3=None), dict(ws=None),
                dict(w2=FAKE_ODD), dict(bias_s=FAKE_ODD), dict(ws=FAKE_ODD), dict(g=FAKE_BYTE),
                dict(k=1), dict(k=4), dict(width=300), dict(width=0), dict(batch=0), dict(batch=-3), dict(points=0), dict(points=-1),
                dict(ws_bytes=1024)):
        assert call(L, **bad) != 0, bad
        assert "argument check failed" in _err(L), bad


def test_fold_entry_points_refuse_their_own_operands(L):
    assert _fwd(L, b3=None) != 0 and _fwd(L, y=None) != 0 and _fwd(L, y=FAKE_BYTE) != 0
    assert _bwd(L, dy=None) != 0 and _bwd(L, dw2=None) != 0 and _bwd(L, dbias=None) != 0 and _bwd(L, db3=None) != 0
    assert _bwd(L, dw2=FAKE_ODD) != 0 and _bwd(L, dy=FAKE_BYTE) != 0
    assert _bwd(L, k=2, dg=FAKE) != 0            # the lattice has no gradient
    assert "argument check failed" in _err(L)
    short = L.a3vt_fold_workspace_bytes(2, 100, 0)
    assert _bwd(L, ws_bytes=short) != 0          # the forward's workspace is too small for the backward


def test_k2_lattice_with_a_gradient_is_refused():
    """``FoldFn`` has no dg for k = 2: a ``g`` that wants one is refused before anything touches a device (a ``None`` from
    ``backward`` would read as a zero gradient).  Without the gradient the same call gets as far as the device check."""
    from a3vt_amd import ops
    from a3vt_amd.pterotactyl.reconstruction.autoencoder import model as am
    fold = am._Fold(514)
    code, g = torch.zeros(2, 512), torch.zeros(2, 5, 2)
    with pytest.raises(RuntimeError, match="the k = 2 lattice has no gradient path"):
        ops.fold(code, g.clone().requires_grad_(True), fold.conv1, fold.conv2, fold.conv3)
    with pytest.raises(RuntimeError, match="must be a tensor on the GPU"):
        ops.fold(code, g, fold.conv1, fold.conv2, fold.conv3)
    with pytest.raises(RuntimeError, match="must be a tensor on the GPU"):       # k = 3 has the path
        ops.fold(code, torch.zeros(2, 5, 3, requires_grad=True), am._Fold(515).conv1, fold.conv2, fold.conv3)


def test_path_counters_are_appended(L):
    from a3vt_amd import ops
    # every counter keeps its index: the fold counters at 14 and 15, later ones (csr3_split) behind them
    assert ops.PATH_NAMES[14:16] == ("fold_fwd", "fold_bwd") and ops.PATH_NAMES[:2] == ("stack_quad", "stack_rows")
    assert ops.PATH_NAMES[16:] == ("csr3_split",)
    buf = (ctypes.c_longlong * len(ops.PATH_NAMES))()
    assert L.a3vt_dbg_path_counts(buf, len(ops.PATH_NAMES), 0) == len(ops.PATH_NAMES)
    assert L.a3vt_version() == 163


def test_install_as_pterotactyl_registers_the_autoencoder_trainer():
    code = ("import sys; sys.path.insert(0, %r); import a3vt_amd; a3vt_amd.install_as_pterotactyl();"
            "import pterotactyl.reconstruction.autoencoder.train as t;"
            "assert t.Engine.__module__.startswith('a3vt_amd') and callable(t.get_parser);"
            "a = t.get_parser().parse_args([]);"
            "assert (a.batch_size, a.number_points, a.encoding_size, a.num_GCN_layers, a.lr, a.patience) == (16, 30000, 200, 20, 0.0003, 70);"
            "print('ok')") % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]


def test_fused_knob_changes_no_parameter():
    from golden_util import load, state_sha256
    from helpers import make_args
    from a3vt_amd.pterotactyl.reconstruction.autoencoder import model as am
    kw = dict(num_GCN_layers=3, hidden_GCN_size=300, encoding_size=200)
    torch.manual_seed(0)
    plain = am.AutoEncoder({}, torch.zeros(4, 3), make_args(**kw))
    torch.manual_seed(0)
    fused = am.AutoEncoder({}, torch.zeros(4, 3), make_args(fused_decoder=True, **kw))
    assert fused.decoder.model.fused and not plain.decoder.model.fused
    assert list(fused.state_dict()) == list(plain.state_dict())
    assert [tuple(v.shape) for v in fused.state_dict().values()] == [tuple(v.shape) for v in plain.state_dict().values()]
    assert np.array_equal(state_sha256(fused.state_dict()), load("g9_autoencoder.npz")["weight_sha256"])
    # on CPU tensors the fused path is not taken: the torch ops answer, the same values as with the knob off
    code = torch.randn(1, 512, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        assert torch.equal(fused.decoder.model(code), plain.decoder.model(code))


def test_trainer_names_a_missing_vision_model(tmp_path, monkeypatch):
    from helpers import make_args
    from a3vt_amd.pterotactyl.reconstruction.autoencoder import train
    monkeypatch.chdir(tmp_path)
    missing = str(tmp_path / "no_such_vision_model")
    args = make_args(vision_location=missing, exp_type="t", exp_id="missing", eval=False, encoding_size=200, batch_size=2, epochs=1,
                     patience=5)
    with pytest.raises(FileNotFoundError, match="no_such_vision_model"):
        train.Engine(args)
    assert train.pretrained_location(make_args(use_img=True, finger=False, pretrained_root="/p")).rstrip("/") == \
        "/p/reconstruction/auto/v_t_g"
