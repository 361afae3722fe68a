"""CPU tests (no GPU, no compute): ``a3vt_latent_nearest`` and ``a3vt_latent_nearest_scratch_bytes`` refuse what the contract in
``include/a3vt.h`` excludes with an error code and a message, before anything is launched — every call below passes fake device
addresses that must never be dereferenced on the host (the manner of ``test_capi_argument_checks.py``)."""
import ctypes

import pytest

FAKE = 0x7F0000001000        # a "device pointer": 16-byte aligned, never mapped on the host
GOOD = dict(bank=FAKE, bank_actions=FAKE + 0x1000, bank_rows=100, dim=200, queries=FAKE + 0x2000, taken=FAKE + 0x3000, n_queries=3,
            num_actions=50, k=25, idx=FAKE + 0x4000, dist=FAKE + 0x5000, action=FAKE + 0x6000, rank=FAKE + 0x7000,
            scratch=FAKE + 0x8000, stream=None)
ORDER = ("bank", "bank_actions", "bank_rows", "dim", "queries", "taken", "n_queries", "num_actions", "k", "idx", "dist", "action",
         "rank", "scratch", "stream")


@pytest.fixture(scope="module")
def L():
    from a3vt_amd import lib
    return lib.load()


def call(L, **changes):
    a = dict(GOOD, **changes)
    return L.a3vt_latent_nearest(*(a[name] for name in ORDER)), L.a3vt_last_error().decode()


def test_scratch_bytes(L):
    assert L.a3vt_latent_nearest_scratch_bytes(3, 15400, 25) == 3 * 15400 * 4
    assert L.a3vt_latent_nearest_scratch_bytes(1024, 1 << 24, 64) == 1024 * (1 << 24) * 4          # (64 GiB: computed in size_t)
    for bad in ((0, 100, 25), (1025, 100, 25), (3, 0, 25), (3, (1 << 24) + 1, 25), (3, 100, 0), (3, 100, 65), (-1, 100, 25)):
        assert L.a3vt_latent_nearest_scratch_bytes(*bad) == 0, bad


@pytest.mark.parametrize("name,values", [("dim", (0, -1, 4097)), ("n_queries", (0, -3, 1025)), ("k", (0, -1, 65)),
                                         ("bank_rows", (0, -1, (1 << 24) + 1)), ("num_actions", (0, -1, 305))])
def test_limits(L, name, values):
    for v in values:
        rc, msg = call(L, **{name: v})
        assert rc != 0 and "latent_nearest" in msg and f"{name}={v}" in msg, (name, v, msg)


@pytest.mark.parametrize("name", ["bank", "queries", "idx", "dist", "scratch"])
def test_required_pointers(L, name):
    rc, msg = call(L, **{name: None})
    assert rc != 0 and "argument check failed" in msg


def test_actions_go_together(L):
    """``bank_actions`` may be NULL only together with ``action`` and ``rank``."""
    for missing in (("bank_actions",), ("action",), ("rank",), ("bank_actions", "action"), ("action", "rank"), ("bank_actions", "rank")):
        rc, msg = call(L, **{m: None for m in missing})
        assert rc != 0 and "argument check failed" in msg, missing


def test_alignment(L):
    for name in ("bank", "queries"):                       # rows of 200 floats are read with 16-byte loads
        for off in (4, 8):
            rc, msg = call(L, **{name: GOOD[name] + off})
            assert rc != 0 and "aligned_to" in msg, (name, off)
        rc, msg = call(L, dim=201, **{name: GOOD[name] + 2})
        assert rc != 0 and "aligned_to" in msg, name
    for name in ("bank_actions", "taken", "idx", "dist", "action", "rank", "scratch"):
        rc, msg = call(L, **{name: GOOD[name] + 2})
        assert rc != 0 and "aligned_to" in msg, name


def test_the_lookup_is_in_the_build():
    from a3vt_amd import lib
    assert "latent_nn.hip" in lib.SOURCES and ctypes.sizeof(ctypes.c_size_t) == 8
