"""CPU tests (no GPU, no compute): ``a3vt_touch_render`` and ``a3vt_touch_finish`` refuse what the contract in ``include/a3vt.h``
excludes with an error code and a message that names the argument, before anything is launched — every call below passes fake
device addresses that must never be dereferenced on the host (the manner of ``test_candidate_tally_capi.py``)."""
import math

import pytest

FAKE = 0x7F0000001000        # a "device pointer": 16-byte aligned, never mapped on the host
GOOD = dict(verts=FAKE, V=42, faces=FAKE + 0x1000, F=80, face_offset=FAKE + 0x2000, M=1, image_mesh=FAKE + 0x3000, cam_pos=FAKE + 0x4000,
            cam_rot=FAKE + 0x5000, I=12, max_depth=0.025, yfov=40.0 / 180.0 * math.pi, znear=1e-4, zfar=10.0, depth=FAKE + 0x6000,
            touch=FAKE + 0x7000, points=FAKE + 0x8000, count=FAKE + 0x9000, status=FAKE + 0xA000, stream=None)
ORDER = ("verts", "V", "faces", "F", "face_offset", "M", "image_mesh", "cam_pos", "cam_rot", "I", "max_depth", "yfov", "znear", "zfar",
         "depth", "touch", "points", "count", "status", "stream")
FINISH_ORDER = ("depth", "cam_pos", "cam_rot", "I", "max_depth", "yfov", "touch", "points", "count", "status", "stream")
POINTERS = ("verts", "faces", "face_offset", "image_mesh", "cam_pos", "cam_rot", "depth", "touch", "points", "count", "status")


@pytest.fixture(scope="module")
def L():
    from a3vt_amd import lib
    return lib.load()


def render(L, **changes):
    a = dict(GOOD, **changes)
    return L.a3vt_touch_render(*(a[name] for name in ORDER)), L.a3vt_last_error().decode()


def finish(L, **changes):
    a = dict(GOOD, **changes)
    return L.a3vt_touch_finish(*(a[name] for name in FINISH_ORDER)), L.a3vt_last_error().decode()


@pytest.mark.parametrize("name,values", [("I", (0, -1, 65537)), ("M", (0, -3, (1 << 20) + 1)), ("V", (-1, (1 << 28) + 1)),
                                         ("F", (-1, (1 << 28) + 1))])
def test_counts_outside(L, name, values):
    for v in values:
        rc, msg = render(L, **{name: v})
        assert rc != 0 and "touch_render" in msg and f"{name}={v}" in msg, (name, v, msg)


def test_scalars_outside(L):
    for call, who in ((render, "touch_render"), (finish, "touch_finish")):
        for v in (0.0, -0.025, float("nan")):
            rc, msg = call(L, max_depth=v)
            assert rc != 0 and who in msg and "max_depth=" in msg, (v, msg)
        for v in (0.0, -0.1, math.pi, 4.0, float("nan")):
            rc, msg = call(L, yfov=v)
            assert rc != 0 and who in msg and "yfov=" in msg and "(0, pi)" in msg, (v, msg)
    for v in (0.0, -1e-4, float("nan")):
        rc, msg = render(L, znear=v)
        assert rc != 0 and "znear=" in msg, (v, msg)
    for near, far in ((1.0, 1.0), (2.0, 1.0), (1e-4, float("nan"))):
        rc, msg = render(L, znear=near, zfar=far)
        assert rc != 0 and "zfar=" in msg and "znear=" in msg, (near, far, msg)


@pytest.mark.parametrize("name", ["verts", "faces", "face_offset", "image_mesh", "cam_pos", "cam_rot", "depth", "status"])
def test_required_pointers(L, name):
    rc, msg = render(L, **{name: None})
    assert rc != 0 and f"{name}=NULL" in msg, msg
    if name in FINISH_ORDER:
        rc, msg = finish(L, **{name: None})
        assert rc != 0 and "touch_finish" in msg and f"{name}=NULL" in msg, msg


def test_pointers_that_go_together(L):
    for call in (render, finish):
        rc, msg = call(L, count=None)
        assert rc != 0 and "count=NULL" in msg and "together" in msg, msg
        rc, msg = call(L, points=None)
        assert rc != 0 and "points=NULL" in msg and "together" in msg, msg


@pytest.mark.parametrize("name", POINTERS)
def test_alignment(L, name):
    for off in (1, 2):
        rc, msg = render(L, **{name: GOOD[name] + off})
        assert rc != 0 and f"{name}=0x" in msg and "4-byte aligned" in msg, (name, off, msg)
        if name in FINISH_ORDER:
            rc, msg = finish(L, **{name: GOOD[name] + off})
            assert rc != 0 and "touch_finish" in msg and f"{name}=0x" in msg and "4-byte aligned" in msg, (name, off, msg)


def test_empty_tables_need_no_pointer(L):
    """``verts`` may be NULL when V == 0 and ``faces`` when F == 0: such a call gets past those two (and is refused here for a
    reason of its own, so that nothing is launched)."""
    rc, msg = render(L, verts=None, V=0, faces=None, F=0, status=None)
    assert rc != 0 and "status=NULL" in msg, msg


def test_the_renderer_is_in_the_build():
    from a3vt_amd import lib
    assert "touch_render.hip" in lib.SOURCES and "a3vt_touch_render" in lib.SIGNATURES and "a3vt_touch_finish" in lib.SIGNATURES
    assert len(lib.SIGNATURES["a3vt_touch_render"][1]) == len(ORDER) and len(lib.SIGNATURES["a3vt_touch_finish"][1]) == len(FINISH_ORDER)
