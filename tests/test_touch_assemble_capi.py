"""CPU tests (no GPU, no compute): ``a3vt_touch_assemble`` refuses what the contract in ``include/a3vt.h`` excludes with an error
code and a message that names ``touch_assemble``, the argument and its value, before anything is launched — every call below
passes fake device addresses that must never be dereferenced on the host (the manner of ``test_touch_render_capi.py``)."""
import pytest

FAKE = 0x7F0000001000        # a "device pointer": 16-byte aligned, never mapped on the host
GOOD = dict(table_charts=FAKE, table_codes=FAKE + 0x1000, state_charts=FAKE + 0x2000, state_masks=FAKE + 0x3000,
            candidates=FAKE + 0x4000, K=50, E=3, A=50, F=4, G=5, C=25, slot=2, charts=FAKE + 0x5000, masks=FAKE + 0x6000, stream=None)
ORDER = ("table_charts", "table_codes", "state_charts", "state_masks", "candidates", "K", "E", "A", "F", "G", "C", "slot", "charts",
         "masks", "stream")
POINTERS = ("table_charts", "table_codes", "state_charts", "state_masks", "candidates", "charts", "masks")


@pytest.fixture(scope="module")
def L():
    from a3vt_amd import lib
    return lib.load()


def assemble(L, **changes):
    a = dict(GOOD, **changes)
    return L.a3vt_touch_assemble(*(a[name] for name in ORDER)), L.a3vt_last_error().decode()


@pytest.mark.parametrize("name", ["K", "E", "A", "F", "G", "C"])
def test_counts_below_one(L, name):
    for v in (0, -1, -(1 << 31)):
        rc, msg = assemble(L, **{name: v})
        assert rc != 0 and "touch_assemble" in msg and f"{name}={v}" in msg, (name, v, msg)


def test_slot_outside(L):
    for slot, G in ((-1, 5), (5, 5), (1, 1), (-(1 << 31), 5), ((1 << 31) - 1, 5)):
        rc, msg = assemble(L, slot=slot, G=G)
        assert rc != 0 and "touch_assemble" in msg and f"slot={slot}" in msg, (slot, G, msg)


def test_the_product_limit(L):
    """K * E * F * G * C * 3 < 2**31: the last product that fits passes this check (and is refused for a NULL pointer, so nothing
    is launched); the first that does not is refused by name with its value, also where it overflows 64 bits."""
    fits = dict(K=1 << 14, E=1 << 8, F=1, G=1, C=170, slot=0)                                # 3 * 2**22 * 170 = 2 139 095 040
    rc, msg = assemble(L, masks=None, **fits)
    assert rc != 0 and "masks=NULL" in msg, msg
    for sizes in (dict(fits, C=171), dict(K=1 << 20, E=1 << 10, F=1, G=1, C=1, slot=0), dict(K=715827883, E=1, F=1, G=1, C=1, slot=0),
                  dict(K=(1 << 31) - 1, E=(1 << 31) - 1, A=1, F=(1 << 31) - 1, G=(1 << 31) - 1, C=(1 << 31) - 1, slot=0)):
        a = dict(GOOD, **sizes)
        product = 3 * a["K"] * a["E"] * a["F"] * a["G"] * a["C"]
        rc, msg = assemble(L, **sizes)
        assert rc != 0 and "touch_assemble" in msg and "K*E*F*G*C*3=" in msg and "2147483648" in msg, (sizes, msg)
        assert all(f"{n}={a[n]}" in msg for n in "KEFGC"), msg
        if product < 1 << 53:
            assert f"K*E*F*G*C*3={product} " in msg, msg
    rc, msg = assemble(L, K=715827882, E=1, F=1, G=1, C=1, slot=0, masks=None)          # 3 * K = 2**31 - 2
    assert rc != 0 and "masks=NULL" in msg, msg
    # the table's size is not limited by the product: A is free
    rc, msg = assemble(L, A=(1 << 31) - 1, masks=None)
    assert rc != 0 and "masks=NULL" in msg, msg


@pytest.mark.parametrize("name", POINTERS)
def test_required_pointers(L, name):
    rc, msg = assemble(L, **{name: None})
    assert rc != 0 and "touch_assemble" in msg and f"{name}=NULL" in msg, msg


@pytest.mark.parametrize("name", POINTERS)
def test_alignment(L, name):
    for off in (1, 2, 3):
        rc, msg = assemble(L, **{name: GOOD[name] + off})
        assert rc != 0 and "touch_assemble" in msg and f"{name}=0x" in msg and "4-byte aligned" in msg, (name, off, msg)


def test_the_launch_counter_counts_no_refused_call(L):
    import ctypes
    buf = (ctypes.c_longlong * 1)()
    assert L.a3vt_touch_assemble_launches(buf, 1) == 1
    for changes in (dict(K=0), dict(slot=5), dict(charts=None), dict(masks=GOOD["masks"] + 2)):
        assert assemble(L, **changes)[0] != 0
    assert L.a3vt_touch_assemble_launches(buf, 0) == 1 and buf[0] == 0
    assert L.a3vt_touch_assemble_launches(None, 0) == 1


def test_the_entry_is_in_the_build():
    from a3vt_amd import lib
    assert "touch_assemble.hip" in lib.SOURCES and "a3vt_touch_assemble" in lib.SIGNATURES
    assert len(lib.SIGNATURES["a3vt_touch_assemble"][1]) == len(ORDER) and len(lib.SIGNATURES["a3vt_touch_assemble_launches"][1]) == 2
