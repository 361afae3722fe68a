"""CPU tests (no GPU, no compute): ``a3vt_hull_place`` refuses what the contract in ``include/a3vt.h`` excludes with an error code and a
message that names ``hull_place``, the argument and its value, before anything is launched — the device arguments below are fake
addresses that must never be dereferenced; ``vert_offset``, ``directions`` and ``tip_offset`` are HOST tables and real (the manner
of ``test_grasp_capi.py``)."""
import ctypes

import numpy as np
import pytest

FAKE = 0x7F0000001000        # a "device pointer": 16-byte aligned, never mapped on the host
ORDER = ("verts", "V", "vert_offset", "M", "directions", "A", "hand_distance", "tip_offset", "status", "base_pos", "base_rot", "simplex",
         "t", "stream")
DEVICE = ("verts", "status", "base_pos", "base_rot", "simplex", "t")
HOST = ("vert_offset", "directions", "tip_offset")


@pytest.fixture(scope="module")
def L():
    from a3vt_amd import lib
    return lib.load()


@pytest.fixture(scope="module")
def tables():
    rng = np.random.default_rng(0)
    return dict(vert_offset=np.array([0, 162, 170], np.int32), directions=np.ascontiguousarray(rng.normal(size=(50, 3))),
                tip_offset=np.array([0.0, 0.0, 0.133]))


def call(L, tables, **changes):
    """One call with the good arguments but for ``changes``: arrays replace a host table, ints a pointer's address."""
    args = dict(V=174, M=2, A=50, hand_distance=0.013, stream=None)
    for i, name in enumerate(DEVICE):
        args[name] = FAKE + 0x1000 * i
    keep = {}
    for name in HOST:
        keep[name] = np.ascontiguousarray(changes.pop(name)) if isinstance(changes.get(name), np.ndarray) else tables[name]
        args[name] = keep[name].ctypes.data
    args.update(changes)
    rc = L.a3vt_hull_place(*(args[name] for name in ORDER))
    return rc, L.a3vt_last_error().decode()


@pytest.mark.parametrize("name,values", [("M", (0, -3, (1 << 20) + 1)), ("A", (0, -1, 129)), ("V", (-1, (1 << 28) + 1))])
def test_counts_outside(L, tables, name, values):
    for v in values:
        rc, msg = call(L, tables, **{name: v})
        assert rc != 0 and "hull_place" in msg and f"{name}={v}" in msg, (name, v, msg)


def test_pairs_outside(L, tables):
    offsets = np.zeros((1 << 14) + 2, np.int32)
    rc, msg = call(L, tables, M=(1 << 14) + 1, A=64, vert_offset=offsets, directions=np.ones((64, 3)))
    assert rc != 0 and "hull_place" in msg and f"M*A={((1 << 14) + 1) * 64}" in msg, msg


@pytest.mark.parametrize("name", DEVICE + HOST)
def test_required_pointers(L, tables, name):
    rc, msg = call(L, tables, **{name: None})
    assert rc != 0 and "hull_place" in msg and f"{name}=NULL" in msg, msg


@pytest.mark.parametrize("name", DEVICE)
def test_alignment(L, tables, name):
    for off in (1, 2) + ((4,) if name == "t" else ()):
        rc, msg = call(L, tables, **{name: FAKE + 0x100000 + off})
        assert rc != 0 and f"{name}=0x" in msg and ("8-byte aligned" if name == "t" else "4-byte aligned") in msg, (name, off, msg)


def test_host_table_alignment(L, tables):
    rc, msg = call(L, tables, directions=tables["directions"].ctypes.data + 4)
    assert rc != 0 and "directions=0x" in msg and "8-byte aligned" in msg, msg
    rc, msg = call(L, tables, tip_offset=tables["tip_offset"].ctypes.data + 4)
    assert rc != 0 and "tip_offset=0x" in msg and "8-byte aligned" in msg, msg
    rc, msg = call(L, tables, vert_offset=tables["vert_offset"].ctypes.data + 2)
    assert rc != 0 and "vert_offset=0x" in msg and "4-byte aligned" in msg, msg


def test_vert_offset_must_be_monotone_and_inside(L, tables):
    rc, msg = call(L, tables, vert_offset=np.array([0, 165, 162], np.int32))
    assert rc != 0 and "hull_place" in msg and "vert_offset[2]=162" in msg and "must not decrease" in msg, msg
    rc, msg = call(L, tables, vert_offset=np.array([-1, 162, 170], np.int32))
    assert rc != 0 and "vert_offset[0]=-1" in msg, msg
    rc, msg = call(L, tables, vert_offset=np.array([0, 162, 175], np.int32))
    assert rc != 0 and "vert_offset[2]=175" in msg and "V=174" in msg, msg


def test_directions_and_scalars(L, tables):
    def changed(row, col, value):
        d = tables["directions"].copy()
        d[row, col] = value
        return d
    for value in (np.nan, np.inf, -np.inf):
        rc, msg = call(L, tables, directions=changed(17, 2, value))
        assert rc != 0 and "hull_place" in msg and "directions[17][2]" in msg and "finite" in msg, msg
    zero = tables["directions"].copy()
    zero[49] = 0.0
    rc, msg = call(L, tables, directions=zero)
    assert rc != 0 and "directions[49]" in msg and "zero" in msg, msg
    rc, msg = call(L, tables, hand_distance=float("nan"))
    assert rc != 0 and "hand_distance=nan" in msg, msg
    rc, msg = call(L, tables, tip_offset=np.array([0.0, np.inf, 0.133]))
    assert rc != 0 and "tip_offset[1]=inf" in msg, msg


def test_bindings_and_build_flags(L):
    from a3vt_amd import lib, ops
    assert "hull_place.hip" in lib.SOURCES and "-ffp-contract=off" in lib.EXTRA_FLAGS["hull_place.hip"]
    res, args = lib.SIGNATURES["a3vt_hull_place"]
    assert len(args) == len(ORDER) and args[ORDER.index("hand_distance")] is ctypes.c_double and res is ctypes.c_int
    before = ops.hull_place_launches()
    assert set(before) == {"calls", "launches"}
    assert L.a3vt_version() == 163
