"""CPU tests (no GPU, no compute): ``a3vt_scene_render`` refuses what the contract in ``include/a3vt.h`` excludes with an error code
and a message that names the argument, before anything is launched — the device pointers below are fake addresses that must never
be dereferenced on the host (the manner of ``test_touch_render_capi.py``).  The small HOST tables (offsets, image_scene, lights,
background) are real arrays: the call reads and checks them."""
import ctypes
import math

import numpy as np
import pytest

FAKE = 0x7F0000001000        # a "device pointer": 16-byte aligned, never mapped on the host
ORDER = ("verts", "V", "faces", "face_rgb", "F", "centres", "radii", "sphere_rgb", "S", "face_offset", "sphere_offset", "M", "image_scene",
         "cam_pos", "cam_rot", "I", "yfov", "znear", "zfar", "W", "H", "lights", "L", "ambient", "background", "rgb", "depth", "prim", "stream")
DEVICE = ("verts", "faces", "face_rgb", "centres", "radii", "sphere_rgb", "cam_pos", "cam_rot", "rgb", "depth", "prim")
ALIGNED = ("verts", "faces", "centres", "radii", "cam_pos", "cam_rot", "depth", "prim")       # (the byte tables need no alignment)
HOST = dict(face_offset=np.array([0, 30, 30, 80], np.int32), sphere_offset=np.array([0, 0, 5, 9], np.int32),
            image_scene=np.array([0, 2, 1, 2], np.int32), lights=np.array([[0, -0.8, 0.3, 1.8], [1, 0, 1, 1.8]], np.float32),
            background=np.array([255, 255, 255], np.uint8))


def host(a):
    return a.ctypes.data_as(ctypes.c_void_p)


GOOD = dict({name: FAKE + 0x1000 * i for i, name in enumerate(DEVICE)}, V=42, F=80, S=9, M=3, I=4, yfov=60.0 / 180.0 * math.pi, znear=0.01,
            zfar=10.0, W=512, H=512, L=2, ambient=0.3, stream=None, **{k: host(v) for k, v in HOST.items()})


@pytest.fixture(scope="module")
def native():
    from a3vt_amd import lib
    return lib.load()


def render(native, **changes):
    a = dict(GOOD, **{k: host(v) if isinstance(v, np.ndarray) else v for k, v in changes.items()})
    return native.a3vt_scene_render(*(a[name] for name in ORDER)), native.a3vt_last_error().decode()


@pytest.mark.parametrize("name,values", [("I", (0, -1, 65537)), ("M", (0, -3, (1 << 20) + 1)), ("W", (0, -1, 2049)), ("H", (0, 2049)),
                                         ("L", (-1, 9)), ("V", (-1, (1 << 28) + 1)), ("F", (-1, (1 << 28) + 1)), ("S", (-1, (1 << 28) + 1))])
def test_counts_outside(native, name, values):
    for v in values:
        rc, msg = render(native, **{name: v})
        assert rc != 0 and "scene_render" in msg and f"{name}={v}" in msg, (name, v, msg)


def test_scalars_outside(native):
    for v in (0.0, -0.1, math.pi, 4.0, float("nan")):
        rc, msg = render(native, yfov=v)
        assert rc != 0 and "scene_render" in msg and "yfov=" in msg and "(0, pi)" in msg, (v, msg)
    for v in (0.0, -1e-4, float("nan")):
        rc, msg = render(native, znear=v)
        assert rc != 0 and "znear=" in msg, (v, msg)
    for near, far in ((1.0, 1.0), (2.0, 1.0), (0.01, float("nan")), (0.01, float("inf"))):
        rc, msg = render(native, znear=near, zfar=far)
        assert rc != 0 and "zfar=" in msg and "znear=" in msg, (near, far, msg)
    for v in (float("nan"), float("inf")):
        rc, msg = render(native, ambient=v)
        assert rc != 0 and "ambient=" in msg, (v, msg)


@pytest.mark.parametrize("name", ["verts", "faces", "face_rgb", "centres", "radii", "sphere_rgb", "face_offset", "sphere_offset", "image_scene",
                                  "cam_pos", "cam_rot", "lights", "background", "rgb", "depth"])
def test_required_pointers(native, name):
    rc, msg = render(native, **{name: None})
    assert rc != 0 and "scene_render" in msg and f"{name}=NULL" in msg, msg


@pytest.mark.parametrize("name", ALIGNED)
def test_alignment(native, name):
    for off in (1, 2):
        rc, msg = render(native, **{name: GOOD[name] + off})
        assert rc != 0 and f"{name}=0x" in msg and "4-byte aligned" in msg, (name, off, msg)


def test_offsets(native):
    for table, count in (("face_offset", "F"), ("sphere_offset", "S")):
        good = HOST[table]
        rc, msg = render(native, **{table: np.array([-1, good[1], good[2], good[3]], np.int32)})
        assert rc != 0 and f"{table}[0]=-1" in msg, msg
        rc, msg = render(native, **{table: np.array([0, good[2] + 3, good[2], good[3]], np.int32)})
        assert rc != 0 and f"{table}[2]={good[2]}" in msg and "decrease" in msg, msg
        rc, msg = render(native, **{table: np.array([0, good[1], good[2], good[3] + 1], np.int32)})
        assert rc != 0 and f"{table}[3]={good[3] + 1}" in msg and f"{count}={GOOD[count]}" in msg, msg


def test_image_scene(native):
    for bad in (-1, 3, 1 << 30):
        table = HOST["image_scene"].copy()
        table[2] = bad
        rc, msg = render(native, image_scene=table)
        assert rc != 0 and f"image_scene[2]={bad}" in msg and "0..2" in msg, msg


def test_empty_tables_need_no_pointer(native):
    """``verts`` may be NULL when V == 0, ``faces`` / ``face_rgb`` when F == 0, the sphere tables when S == 0, ``lights`` when
    L == 0: such a call gets past them (and is refused here for a reason of its own, so that nothing is launched)."""
    zeros = np.zeros(4, np.int32)
    rc, msg = render(native, verts=None, V=0, faces=None, face_rgb=None, F=0, centres=None, radii=None, sphere_rgb=None, S=0, lights=None, L=0,
                     face_offset=zeros, sphere_offset=zeros, depth=None)
    assert rc != 0 and "depth=NULL" in msg, msg
    rc, msg = render(native, prim=None, rgb=None)                 # prim is optional: the refusal is rgb's
    assert rc != 0 and "rgb=NULL" in msg, msg


def test_nothing_was_launched(native):
    counts = (ctypes.c_longlong * 2)()
    assert native.a3vt_scene_launches(counts, 1) == 2
    render(native, I=0)
    render(native, image_scene=np.array([0, 0, 0, 9], np.int32))
    assert native.a3vt_scene_launches(counts, 0) == 2 and list(counts) == [0, 0]


def test_the_renderer_is_in_the_build():
    from a3vt_amd import lib
    assert "scene_render.hip" in lib.SOURCES and "a3vt_scene_render" in lib.SIGNATURES and "a3vt_scene_launches" in lib.SIGNATURES
    assert len(lib.SIGNATURES["a3vt_scene_render"][1]) == len(ORDER)
