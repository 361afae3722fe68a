"""CPU tests (no GPU, no compute): ``a3vt_touch_chart_head`` refuses what the contract in ``include/a3vt.h`` excludes with an error
code and a message that names ``touch_chart_head``, the argument and its value, before anything is launched — every call below
passes fake device addresses that must never be dereferenced on the host (the manner of ``test_touch_assemble_capi.py``)."""
import pytest

FAKE = 0x7F0000001000        # a "device pointer": 16-byte aligned, never mapped on the host
ORDER = ("features", "w1", "b1", "w2", "b2", "w3", "b3", "tmpl", "rot", "pos", "code", "n", "rows", "charts", "masks", "stream")
POINTERS = tuple(name for name in ORDER if name not in ("n", "stream"))
GOOD = dict({name: FAKE + 0x1000 * i for i, name in enumerate(POINTERS)}, n=600, stream=None)
REQUIRED = tuple(name for name in POINTERS if name not in ("charts", "masks"))
ALIGN = {name: 16 if name in ("features", "w1", "w2", "w3", "rows") else 4 for name in POINTERS}


@pytest.fixture(scope="module")
def L():
    from a3vt_amd import lib
    return lib.load()


def head(L, **changes):
    a = dict(GOOD, **changes)
    return L.a3vt_touch_chart_head(*(a[name] for name in ORDER)), L.a3vt_last_error().decode()


def test_n_below_one(L):
    for v in (0, -1, -(1 << 31)):
        rc, msg = head(L, n=v)
        assert rc != 0 and "touch_chart_head" in msg and f"n={v}" in msg, (v, msg)


def test_the_product_limit(L):
    """n * 512 < 2**31: the last n that fits passes this check (and is refused for a NULL pointer, so nothing is launched); the
    first that does not is refused by name with the product and n."""
    last = (1 << 22) - 1
    rc, msg = head(L, n=last, rows=None)
    assert rc != 0 and "rows=NULL" in msg, msg
    for n in (last + 1, 1 << 25, (1 << 31) - 1):
        rc, msg = head(L, n=n)
        assert rc != 0 and "touch_chart_head" in msg and f"n*512={512 * n} " in msg and f"n={n}" in msg and "2147483648" in msg, (n, msg)


@pytest.mark.parametrize("name", REQUIRED)
def test_required_pointers(L, name):
    rc, msg = head(L, **{name: None})
    assert rc != 0 and "touch_chart_head" in msg and f"{name}=NULL" in msg, msg


def test_charts_and_masks_come_together(L):
    for name in ("charts", "masks"):
        rc, msg = head(L, **{name: None})
        assert rc != 0 and "touch_chart_head" in msg and f"{name}=NULL" in msg and "together" in msg, msg
    # neither is fine: that call passes every check, so it is not made here (it would launch); one more refusal behind it shows it
    rc, msg = head(L, charts=None, masks=None, code=None)
    assert rc != 0 and "code=NULL" in msg, msg


@pytest.mark.parametrize("name", POINTERS)
def test_alignment(L, name):
    for off in (1, 2, 3) + ((4, 8, 12) if ALIGN[name] == 16 else ()):
        rc, msg = head(L, **{name: GOOD[name] + off})
        assert rc != 0 and "touch_chart_head" in msg and f"{name}=0x" in msg and f"{ALIGN[name]}-byte aligned" in msg, (name, off, msg)
    if ALIGN[name] == 4:                                   # a 4-byte boundary is enough there: the next refusal is another one
        rc, msg = head(L, **{name: GOOD[name] + 4, "n": 0})
        assert rc != 0 and "n=0" in msg, msg


def test_the_launch_counter_counts_no_refused_call(L):
    import ctypes
    buf = (ctypes.c_longlong * 1)()
    assert L.a3vt_touch_chart_head_launches(buf, 1) == 1
    for changes in (dict(n=0), dict(n=1 << 22), dict(rows=None), dict(masks=None), dict(features=GOOD["features"] + 4)):
        assert head(L, **changes)[0] != 0
    assert L.a3vt_touch_chart_head_launches(buf, 0) == 1 and buf[0] == 0
    assert L.a3vt_touch_chart_head_launches(None, 0) == 1


def test_the_entry_is_in_the_build():
    from a3vt_amd import lib, ops
    assert "chart_head.hip" in lib.SOURCES and "a3vt_touch_chart_head" in lib.SIGNATURES
    assert len(lib.SIGNATURES["a3vt_touch_chart_head"][1]) == len(ORDER) and len(lib.SIGNATURES["a3vt_touch_chart_head_launches"][1]) == 2
    assert callable(ops.touch_chart_head) and callable(ops.chart_head_launches)
