"""CPU tests (no GPU, no compute): ``a3vt_touch_pack`` refuses what the contract in ``include/a3vt.h`` excludes with an error code and
a message that names ``touch_pack``, the argument and its value, before anything is launched — every call below passes fake device
addresses that must never be dereferenced on the host (the manner of ``test_chart_head_capi.py``)."""
import pytest

FAKE = 0x7F0000001000        # a "device pointer": 16-byte aligned, never mapped on the host
ORDER = ("touch", "points", "count", "status", "I", "capacity", "touch_u8", "offsets", "cloud", "stream")
POINTERS = tuple(name for name in ORDER if name not in ("I", "capacity", "stream"))
GOOD = dict({name: FAKE + 0x1000 * i for i, name in enumerate(POINTERS)}, I=12, capacity=12 * 14641, stream=None)
IMAGE, CLOUD = ("touch", "touch_u8"), ("points", "count", "status", "offsets", "cloud")
ALIGN = {name: 16 if name == "touch" else 4 for name in POINTERS}
MAX_IMAGES = 1 << 16


@pytest.fixture(scope="module")
def L():
    from a3vt_amd import lib
    return lib.load()


def pack(L, **changes):
    a = dict(GOOD, **changes)
    return L.a3vt_touch_pack(*(a[name] for name in ORDER)), L.a3vt_last_error().decode()


def test_the_view_count(L):
    for v in (0, -1, -(1 << 31), MAX_IMAGES + 1, (1 << 31) - 1):
        rc, msg = pack(L, I=v)
        assert rc != 0 and "touch_pack" in msg and f"I={v} " in msg and f"1..{MAX_IMAGES}" in msg, (v, msg)
    rc, msg = pack(L, I=MAX_IMAGES, offsets=None)          # the limit itself passes this check; the next refusal shows it
    assert rc != 0 and "offsets=NULL" in msg, msg


def test_negative_capacity(L):
    for v in (-1, -(1 << 31)):
        rc, msg = pack(L, capacity=v)
        assert rc != 0 and "touch_pack" in msg and f"capacity={v} " in msg, (v, msg)
    rc, msg = pack(L, capacity=0, cloud=None, count=None)  # capacity 0 needs no cloud: the next refusal is count's
    assert rc != 0 and "count=NULL" in msg, msg
    rc, msg = pack(L, capacity=1, cloud=None)
    assert rc != 0 and "cloud=NULL" in msg and "capacity > 0" in msg, msg


def test_nothing_to_pack(L):
    rc, msg = pack(L, **{name: None for name in POINTERS})
    assert rc != 0 and "touch_pack" in msg and "nothing to pack" in msg, msg


@pytest.mark.parametrize("name", IMAGE)
def test_touch_and_touch_u8_come_together(L, name):
    rc, msg = pack(L, **{name: None})
    assert rc != 0 and "touch_pack" in msg and f"{name}=NULL" in msg and "together" in msg, msg
    rc, msg = pack(L, **{name: None}, **{other: None for other in CLOUD})      # ... with the cloud group absent too
    assert rc != 0 and f"{name}=NULL" in msg and "together" in msg, msg


@pytest.mark.parametrize("name", CLOUD[:4])
def test_the_cloud_group_comes_whole(L, name):
    rc, msg = pack(L, **{name: None})
    assert rc != 0 and "touch_pack" in msg and f"{name}=NULL" in msg and "together" in msg, msg
    rc, msg = pack(L, touch=None, touch_u8=None, **{name: None})               # ... with the image group absent too
    assert rc != 0 and f"{name}=NULL" in msg and "together" in msg, msg
    only = {other: None for other in CLOUD if other != name}                   # one pointer of the group alone: the first missing is named
    rc, msg = pack(L, **only)
    assert rc != 0 and "touch_pack" in msg and "=NULL" in msg and "together" in msg and f"{name}=NULL" not in msg, msg


def test_either_group_alone_is_accepted_by_the_null_checks(L):
    """A whole group absent passes the NULL rules; neither call is completed here (it would launch): one more refusal shows it."""
    rc, msg = pack(L, touch=None, touch_u8=None, points=GOOD["points"] + 2)
    assert rc != 0 and "points=0x" in msg and "4-byte aligned" in msg, msg
    rc, msg = pack(L, **{name: None for name in CLOUD}, touch=GOOD["touch"] + 8)
    assert rc != 0 and "touch=0x" in msg and "16-byte aligned" in msg, msg


@pytest.mark.parametrize("name", POINTERS)
def test_alignment(L, name):
    for off in (1, 2, 3) + ((4, 8, 12) if ALIGN[name] == 16 else ()):
        rc, msg = pack(L, **{name: GOOD[name] + off})
        assert rc != 0 and "touch_pack" in msg and f"{name}=0x" in msg and f"{ALIGN[name]}-byte aligned" in msg, (name, off, msg)
    if ALIGN[name] == 4:                                   # a 4-byte boundary is enough there: the next refusal is another one
        rc, msg = pack(L, **{name: GOOD[name] + 4, "I": 0})
        assert rc != 0 and "I=0" in msg, msg


def test_the_launch_counter_counts_no_refused_call(L):
    import ctypes
    buf = (ctypes.c_longlong * 1)()
    assert L.a3vt_touch_pack_launches(buf, 1) == 1
    for changes in (dict(I=0), dict(capacity=-1), dict(offsets=None), dict(touch_u8=None), dict(touch=GOOD["touch"] + 4)):
        assert pack(L, **changes)[0] != 0
    assert L.a3vt_touch_pack_launches(buf, 0) == 1 and buf[0] == 0
    assert L.a3vt_touch_pack_launches(None, 0) == 1


def test_the_entry_is_in_the_build():
    from a3vt_amd import lib, ops
    assert "touch_pack.hip" in lib.SOURCES and "a3vt_touch_pack" in lib.SIGNATURES
    assert len(lib.SIGNATURES["a3vt_touch_pack"][1]) == len(ORDER) and len(lib.SIGNATURES["a3vt_touch_pack_launches"][1]) == 2
    assert callable(ops.touch_pack) and callable(ops.touch_pack_launches)
    assert ops.VISION_DEFAULTS["cam_pos"] == (-0.3, 0.0, 0.3) and ops.VISION_DEFAULTS["width"] == ops.VISION_DEFAULTS["height"] == 256
