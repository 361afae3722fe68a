"""CPU tests (no GPU, no compute): ``a3vt_grasp_close`` refuses what the contract in ``include/a3vt.h`` excludes with an error code and
a message that names the argument, before anything is launched — the device arguments below are fake addresses that must never be
dereferenced; ``face_offset``, ``grasp_mesh``, ``hand_table`` and ``q0`` are HOST tables and real (the manner of
``test_touch_render_capi.py`` and ``test_scene_render_capi.py``)."""
import ctypes

import numpy as np
import pytest

import grasp_ref as gr

FAKE = 0x7F0000001000        # a "device pointer": 16-byte aligned, never mapped on the host
ORDER = ("verts", "V", "faces", "F", "face_offset", "M", "grasp_mesh", "base_pos", "base_rot", "G", "hand_table", "q0", "steps", "q_out",
         "blocked_step", "link_pos", "link_rot", "frame_pos", "frame_rot", "stream")
DEVICE = ("verts", "faces", "base_pos", "base_rot", "q_out", "blocked_step", "link_pos", "link_rot", "frame_pos", "frame_rot")
HOST = ("face_offset", "grasp_mesh", "hand_table", "q0")


@pytest.fixture(scope="module")
def L():
    from a3vt_amd import lib
    return lib.load()


@pytest.fixture(scope="module")
def tables():
    hand = gr.hand()
    return dict(face_offset=np.array([0, 320, 332], np.int32), grasp_mesh=np.array([0, 1, 0], np.int32),
                hand_table=np.ascontiguousarray(hand.table()), q0=np.ascontiguousarray(hand.q0, np.float64))


def call(L, tables, **changes):
    """One call with the good arguments but for ``changes``: arrays replace a host table, ints a pointer's address."""
    args = dict(V=174, F=332, M=2, G=3, steps=64, stream=None)
    for i, name in enumerate(DEVICE):
        args[name] = FAKE + 0x1000 * i
    keep = {}
    for name in HOST:
        keep[name] = np.ascontiguousarray(changes.pop(name)) if isinstance(changes.get(name), np.ndarray) else tables[name]
        args[name] = keep[name].ctypes.data
    args.update(changes)
    rc = L.a3vt_grasp_close(*(args[name] for name in ORDER))
    return rc, L.a3vt_last_error().decode()


@pytest.mark.parametrize("name,values", [("G", (-1, (1 << 20) + 1)), ("M", (0, -3, (1 << 20) + 1)), ("V", (-1, (1 << 28) + 1)),
                                         ("F", (-1, (1 << 28) + 1)), ("steps", (0, -1, (1 << 16) + 1))])
def test_counts_outside(L, tables, name, values):
    for v in values:
        rc, msg = call(L, tables, **{name: v})
        assert rc != 0 and "grasp_close" in msg and f"{name}={v}" in msg, (name, v, msg)


@pytest.mark.parametrize("name", DEVICE + HOST)
def test_required_pointers(L, tables, name):
    rc, msg = call(L, tables, **{name: None})
    assert rc != 0 and "grasp_close" in msg and f"{name}=NULL" in msg, msg


@pytest.mark.parametrize("name", DEVICE)
def test_alignment(L, tables, name):
    for off in (1, 2):
        rc, msg = call(L, tables, **{name: FAKE + 0x100000 + off})
        assert rc != 0 and f"{name}=0x" in msg and "4-byte aligned" in msg, (name, off, msg)


def test_host_table_alignment(L, tables):
    rc, msg = call(L, tables, hand_table=tables["hand_table"].ctypes.data + 4)
    assert rc != 0 and "hand_table=0x" in msg and "8-byte aligned" in msg, msg
    rc, msg = call(L, tables, face_offset=tables["face_offset"].ctypes.data + 2)
    assert rc != 0 and "face_offset=0x" in msg and "4-byte aligned" in msg, msg


def test_face_offset_must_be_monotone_and_inside(L, tables):
    rc, msg = call(L, tables, face_offset=np.array([0, 330, 320], np.int32))
    assert rc != 0 and "face_offset[2]=320" in msg and "must not decrease" in msg, msg
    rc, msg = call(L, tables, face_offset=np.array([-1, 320, 332], np.int32))
    assert rc != 0 and "face_offset[0]=-1" in msg, msg
    rc, msg = call(L, tables, face_offset=np.array([0, 320, 333], np.int32))
    assert rc != 0 and "face_offset[2]=333" in msg and "F=332" in msg, msg


def test_grasp_mesh_out_of_range(L, tables):
    for bad in (-1, 2):
        rc, msg = call(L, tables, grasp_mesh=np.array([0, bad, 0], np.int32))
        assert rc != 0 and f"grasp_mesh[1]={bad}" in msg and "0..1" in msg, msg


def test_hand_table_contents(L, tables):
    def changed(row, col, value):
        t = tables["hand_table"].copy()
        t[row, col] = value
        return t
    rc, msg = call(L, tables, hand_table=changed(3, 4, np.nan))
    assert rc != 0 and "hand_table[3][4]" in msg and "finite" in msg, msg
    rc, msg = call(L, tables, hand_table=changed(9, 1, 0.0))            # a chain's third link must be revolute
    assert rc != 0 and "hand_table[9][1]" in msg and "revolute" in msg, msg
    rc, msg = call(L, tables, hand_table=changed(5, 1, 1.0))            # and its sixth fixed
    assert rc != 0 and "hand_table[5][1]" in msg and "fixed" in msg, msg
    rc, msg = call(L, tables, hand_table=changed(8, 0, 3.0))            # a parent in another chain
    assert rc != 0 and "hand_table[8][0]" in msg and "parent" in msg, msg
    rc, msg = call(L, tables, hand_table=changed(8, 0, 8.0))            # a link as its own parent
    assert rc != 0 and "hand_table[8][0]" in msg, msg
    rc, msg = call(L, tables, hand_table=changed(1, 17, 2.0))
    assert rc != 0 and "hand_table[1][17]" in msg and "upper" in msg, msg
    rc, msg = call(L, tables, hand_table=changed(2, 14, 0.5))
    assert rc != 0 and "hand_table[2][14..16]" in msg and "axis" in msg, msg
    rc, msg = call(L, tables, hand_table=changed(4, 24, -0.01))
    assert rc != 0 and "hand_table[4][19]" in msg and "half-extents" in msg, msg
    q0 = tables["q0"].copy()
    q0[22] = np.inf
    rc, msg = call(L, tables, q0=q0)
    assert rc != 0 and "q0[22]" in msg, msg


def test_no_grasp_is_accepted_and_launches_nothing(L, tables):
    """G == 0: returns 0 without reading a device pointer (all of them may be NULL) and without counting a call."""
    from a3vt_amd import ops
    before = ops.grasp_launches()
    nothing = {name: None for name in DEVICE if name not in ("verts", "faces")}
    rc, msg = call(L, tables, G=0, grasp_mesh=None, **nothing)
    assert rc == 0, msg
    assert ops.grasp_launches() == before


def test_reach_and_limits(L, tables):
    """``a3vt_grasp_reach``: no box point of a chain is further from the chain's first joint, in any pose within the limits."""
    from a3vt_amd import lib, ops
    hand = gr.hand()
    reach = ops.grasp_reach(hand.table())
    assert len(reach) == 4 and all(0.1 < r < 0.25 for r in reach)
    rng = np.random.default_rng(0)
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    for _ in range(50):
        q = hand.lower + rng.random(28) * (hand.upper - hand.lower)
        pos, rot = hand.forward(np.zeros(3), np.eye(3), q)
        for i in np.flatnonzero(hand.has_box):
            world = pos[i] + (hand.box_centre[i] + corners * hand.box_half[i]) @ rot[i].T
            assert np.linalg.norm(world - pos[7 * (i // 7)], axis=1).max() <= reach[i // 7]
    assert ops.grasp_limits() == {"capacity": 3072, "per_launch": 64, "table_cols": 26}
    assert L.a3vt_grasp_limit(7) == 0
    assert L.a3vt_grasp_reach(None, 0) < 0 and "grasp_reach" in L.a3vt_last_error().decode()
    assert "grasp_close.hip" in lib.SOURCES and "-ffp-contract=off" in lib.EXTRA_FLAGS["grasp_close.hip"]
    assert len(lib.SIGNATURES["a3vt_grasp_close"][1]) == len(ORDER) and lib.SIGNATURES["a3vt_grasp_reach"][0] is ctypes.c_double
