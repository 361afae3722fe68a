"""CPU tests (no GPU, no compute): ``a3vt_scene_render_posed`` and ``a3vt_pose_parts`` refuse what the contract in ``include/a3vt.h``
excludes with an error code and a message that names the argument, before anything is launched — the device pointers below are fake
addresses that must never be dereferenced on the host (the manner of ``test_scene_render_capi.py``).  The small HOST tables (part and
instance offsets, bounds, lights, background) are real arrays: the calls read and check them."""
import ctypes
import math

import numpy as np
import pytest

FAKE = 0x7F0000001000        # a "device pointer": 16-byte aligned, never mapped on the host
ORDER = ("part_verts", "PV", "part_faces", "PF", "part_face_offset", "part_bound", "P", "inst_part", "inst_pos", "inst_rot", "inst_rgb", "N",
         "inst_offset", "cam_pos", "cam_rot", "I", "yfov", "znear", "zfar", "W", "H", "lights", "L", "ambient", "background", "rgb", "depth",
         "prim_inst", "prim_face", "stream")
DEVICE = ("part_verts", "part_faces", "inst_part", "inst_pos", "inst_rot", "inst_rgb", "cam_pos", "cam_rot", "rgb", "depth", "prim_inst", "prim_face")
ALIGNED = ("part_verts", "part_faces", "inst_part", "inst_pos", "inst_rot", "cam_pos", "cam_rot", "depth", "prim_inst", "prim_face")
HOST = dict(part_face_offset=np.array([0, 30, 30, 80], np.int32), inst_offset=np.array([0, 22, 22, 23, 44], np.int32),
            part_bound=np.array([[0, 0, 0, 1], [0.1, 0, 0, 0], [0, 0.2, 0, 0.5]], np.float32),
            lights=np.array([[0, -0.8, 0.3, 1.0], [1, 0, 1, 1.0]], np.float32), background=np.array([255, 255, 255], np.uint8))
POSE_ORDER = ("part_verts", "PV", "part_faces", "PF", "part_vert_offset", "part_face_offset", "P", "inst_part", "inst_pos", "inst_rot", "inst_rgb",
              "N", "vert_base", "face_base", "verts_out", "TV", "faces_out", "face_rgb_out", "TF", "stream")
POSE_DEVICE = ("part_verts", "part_faces", "inst_part", "inst_pos", "inst_rot", "inst_rgb", "vert_base", "face_base", "verts_out", "faces_out",
               "face_rgb_out")
POSE_HOST = dict(part_vert_offset=np.array([0, 20, 20, 42], np.int32), part_face_offset=HOST["part_face_offset"])


def host(a):
    return a.ctypes.data_as(ctypes.c_void_p)


GOOD = dict({name: FAKE + 0x1000 * i for i, name in enumerate(DEVICE)}, PV=42, PF=80, P=3, N=44, I=4, yfov=60.0 / 180.0 * math.pi, znear=0.01,
            zfar=10.0, W=256, H=256, L=2, ambient=0.3, stream=None, **{k: host(v) for k, v in HOST.items()})
POSE_GOOD = dict({name: FAKE + 0x1000 * i for i, name in enumerate(POSE_DEVICE)}, PV=42, PF=80, P=3, N=44, TV=900, TF=1700, stream=None,
                 **{k: host(v) for k, v in POSE_HOST.items()})


@pytest.fixture(scope="module")
def native():
    from a3vt_amd import lib
    return lib.load()


def call(native, fn, order, good, changes):
    a = dict(good, **{k: host(v) if isinstance(v, np.ndarray) else v for k, v in changes.items()})
    return getattr(native, fn)(*(a[name] for name in order)), native.a3vt_last_error().decode()


def render(native, **changes):
    return call(native, "a3vt_scene_render_posed", ORDER, GOOD, changes)


def pose(native, **changes):
    return call(native, "a3vt_pose_parts", POSE_ORDER, POSE_GOOD, changes)


@pytest.mark.parametrize("name,values", [("I", (0, -1, 65537)), ("P", (0, -3, 97)), ("W", (0, -1, 2049)), ("H", (0, 2049)), ("L", (-1, 9)),
                                         ("PV", (-1, (1 << 28) + 1)), ("PF", (-1, (1 << 28) + 1)), ("N", (-1, (1 << 24) + 1))])
def test_counts_outside(native, name, values):
    for v in values:
        rc, msg = render(native, **{name: v})
        assert rc != 0 and "scene_render_posed" in msg and f"{name}={v}" in msg, (name, v, msg)


@pytest.mark.parametrize("name,values", [("P", (0, 97)), ("PV", (-1, (1 << 28) + 1)), ("PF", (-1,)), ("N", (-1, (1 << 24) + 1)),
                                         ("TV", (-1, (1 << 28) + 1)), ("TF", (-1, (1 << 28) + 1))])
def test_pose_parts_counts_outside(native, name, values):
    for v in values:
        rc, msg = pose(native, **{name: v})
        assert rc != 0 and "pose_parts" in msg and f"{name}={v}" in msg, (name, v, msg)


def test_scalars_outside(native):
    for v in (0.0, -0.1, math.pi, 4.0, float("nan")):
        rc, msg = render(native, yfov=v)
        assert rc != 0 and "scene_render_posed" in msg and "yfov=" in msg and "(0, pi)" in msg, (v, msg)
    for v in (0.0, -1e-4, float("nan")):
        rc, msg = render(native, znear=v)
        assert rc != 0 and "znear=" in msg, (v, msg)
    for near, far in ((1.0, 1.0), (2.0, 1.0), (0.01, float("nan")), (0.01, float("inf"))):
        rc, msg = render(native, znear=near, zfar=far)
        assert rc != 0 and "zfar=" in msg and "znear=" in msg, (near, far, msg)
    for v in (float("nan"), float("inf")):
        rc, msg = render(native, ambient=v)
        assert rc != 0 and "ambient=" in msg, (v, msg)


@pytest.mark.parametrize("name", ["part_verts", "part_faces", "part_face_offset", "part_bound", "inst_part", "inst_pos", "inst_rot", "inst_rgb",
                                  "inst_offset", "cam_pos", "cam_rot", "lights", "background", "rgb", "depth"])
def test_required_pointers(native, name):
    rc, msg = render(native, **{name: None})
    assert rc != 0 and "scene_render_posed" in msg and f"{name}=NULL" in msg, msg


@pytest.mark.parametrize("name", [n for n in POSE_ORDER if n in POSE_DEVICE or n in POSE_HOST])
def test_pose_parts_required_pointers(native, name):
    rc, msg = pose(native, **{name: None})
    assert rc != 0 and "pose_parts" in msg and f"{name}=NULL" in msg, msg


def test_the_primitive_images_come_together(native):
    rc, msg = render(native, prim_inst=None)
    assert rc != 0 and "prim_inst=NULL" in msg, msg
    rc, msg = render(native, prim_face=None)
    assert rc != 0 and "prim_face=NULL" in msg, msg
    rc, msg = render(native, prim_inst=None, prim_face=None, rgb=None)      # neither: accepted, the refusal is rgb's
    assert rc != 0 and "rgb=NULL" in msg, msg


@pytest.mark.parametrize("name", ALIGNED)
def test_alignment(native, name):
    for off in (1, 2):
        rc, msg = render(native, **{name: GOOD[name] + off})
        assert rc != 0 and f"{name}=0x" in msg and "4-byte aligned" in msg, (name, off, msg)


def test_offsets(native):
    for fn, table, count, good in ((render, "part_face_offset", "PF", GOOD), (render, "inst_offset", "N", GOOD),
                                   (pose, "part_vert_offset", "PV", POSE_GOOD), (pose, "part_face_offset", "PF", POSE_GOOD)):
        t = dict(HOST, **POSE_HOST)[table]
        n = len(t) - 1
        bad = t.copy()
        bad[0] = -1
        rc, msg = fn(native, **{table: bad})
        assert rc != 0 and f"{table}[0]=-1" in msg, msg
        bad = t.copy()
        bad[1] = t[2] + 3
        rc, msg = fn(native, **{table: bad})
        assert rc != 0 and f"{table}[2]={t[2]}" in msg and "decrease" in msg, msg
        bad = t.copy()
        bad[n] = good[count] + 1
        rc, msg = fn(native, **{table: bad})
        assert rc != 0 and f"{table}[{n}]={good[count] + 1}" in msg and f"{count}={good[count]}" in msg, msg


def test_part_bound(native):
    for p, k, v in ((1, 0, float("nan")), (2, 2, float("inf")), (0, 3, -1.0), (2, 3, float("nan"))):
        bound = HOST["part_bound"].copy()
        bound[p, k] = v
        rc, msg = render(native, part_bound=bound)
        assert rc != 0 and f"part_bound[{p}][{k}]=" in msg, msg


def test_empty_tables_need_no_pointer(native):
    """The instance tables may be NULL when N == 0, the templates when PV == 0 / PF == 0, ``lights`` when L == 0: such a call gets
    past them (and is refused here for a reason of its own, so that nothing is launched)."""
    rc, msg = render(native, part_verts=None, PV=0, part_faces=None, PF=0, part_face_offset=np.zeros(4, np.int32), inst_part=None, inst_pos=None,
                     inst_rot=None, inst_rgb=None, N=0, inst_offset=np.zeros(5, np.int32), lights=None, L=0, depth=None)
    assert rc != 0 and "depth=NULL" in msg, msg
    rc, msg = pose(native, inst_part=None, inst_pos=None, inst_rot=None, inst_rgb=None, vert_base=None, face_base=None, N=0, verts_out=None,
                   TV=0, faces_out=None, face_rgb_out=None, TF=0, P=0)
    assert rc != 0 and "P=0" in msg, msg


def test_nothing_was_launched(native):
    counts = (ctypes.c_longlong * 3)()
    assert native.a3vt_posed_launches(counts, 1) == 3
    render(native, I=0)
    render(native, inst_offset=np.array([0, 22, 22, 23, 45], np.int32))
    pose(native, TV=-1)
    assert native.a3vt_posed_launches(counts, 0) == 3 and list(counts) == [0, 0, 0]


def test_the_renderer_is_in_the_build():
    from a3vt_amd import lib
    assert "posed_render.hip" in lib.SOURCES and "a3vt_posed_launches" in lib.SIGNATURES
    assert len(lib.SIGNATURES["a3vt_scene_render_posed"][1]) == len(ORDER) and len(lib.SIGNATURES["a3vt_pose_parts"][1]) == len(POSE_ORDER)
