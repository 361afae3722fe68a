"""CPU tests (no GPU, no compute): ``a3vt_latent_policy_fwd`` / ``_bwd``, ``a3vt_action_value_loss`` and
``a3vt_latent_policy_stash_floats`` refuse what the contract in ``include/a3vt.h`` excludes with an error code and a message that
names the value, before anything is launched — every call below passes fake device addresses that must never be dereferenced on
the host (the manner of ``test_capi_argument_checks.py``)."""
import ctypes

import pytest

FAKE = 0x7F0000001000        # a "device pointer": 16-byte aligned, never mapped on the host
DIMS = [(50, 200, 1), (200, 100, 1), (100, 200, 0), (600, 200, 1), (200, 200, 1), (200, 200, 1), (200, 50, 0)]     # t_p's Latent_Model


@pytest.fixture(scope="module")
def L():
    from a3vt_amd import lib
    return lib.load()


def net(dims=DIMS, concat_at=3, latent_size=200, transform=1, n_layers=None, weight_offset=0):
    from a3vt_amd import lib
    m = lib.Mlp()
    for l, (n_in, n_out, relu) in enumerate(dims):
        m.layer[l] = lib.MlpLayer(FAKE + 0x100000 * l + weight_offset, FAKE + 0x100000 * l + 0x80000, n_in, n_out, relu, 0)
    m.n_layers, m.concat_at, m.latent_size, m.transform = len(dims) if n_layers is None else n_layers, concat_at, latent_size, transform
    m.scale, m.offset = 200.0, 100.0
    return m


def grads(n=7, missing=None):
    from a3vt_amd import lib
    g = lib.MlpGrads()
    for l in range(n):
        g.dweight[l], g.dbias[l] = FAKE + 0x4000000 + 0x100000 * l, FAKE + 0x4000000 + 0x100000 * l + 0x80000
    if missing is not None:
        g.dweight[missing] = None
    return g


FWD = dict(mask=FAKE + 0x9000000, latent=FAKE + 0x9100000, first_latent=FAKE + 0x9200000, taken=FAKE + 0x9300000, rows=3,
           values=FAKE + 0x9400000, action=FAKE + 0x9500000, stash=FAKE + 0x9600000, stream=None)


def fwd(L, m, **changes):
    a = dict(FWD, **changes)
    rc = L.a3vt_latent_policy_fwd(ctypes.byref(m) if m is not None else None, *(a[k] for k in ("mask", "latent", "first_latent", "taken", "rows", "values", "action", "stash", "stream")))
    return rc, L.a3vt_last_error().decode()


def bwd(L, m, g, **changes):
    a = dict(dict(FWD, dvalues=FAKE + 0x9700000, delta=FAKE + 0x9800000, accumulate=0), **changes)
    rc = L.a3vt_latent_policy_bwd(ctypes.byref(m), ctypes.byref(g) if g is not None else None,
                                  *(a[k] for k in ("mask", "latent", "first_latent", "dvalues", "stash", "delta", "rows", "accumulate", "stream")))
    return rc, L.a3vt_last_error().decode()


def loss(L, **changes):
    a = dict(dict(values=FAKE, actions=FAKE + 0x1000, targets=FAKE + 0x2000, steps=5, rows=3, num_actions=50, loss=FAKE + 0x3000,
                  dvalues=FAKE + 0x4000, stream=None), **changes)
    rc = L.a3vt_action_value_loss(*(a[k] for k in ("values", "actions", "targets", "steps", "rows", "num_actions", "loss", "dvalues", "stream")))
    return rc, L.a3vt_last_error().decode()


def test_source_signatures_and_limits(L):
    from a3vt_amd import lib, ops
    assert "latent_policy.hip" in lib.SOURCES
    for name in ("a3vt_latent_policy_fwd", "a3vt_latent_policy_bwd", "a3vt_action_value_loss", "a3vt_latent_policy_stash_floats",
                 "a3vt_latent_policy_limit", "a3vt_latent_policy_launches"):
        assert name in lib.SIGNATURES
    assert ctypes.sizeof(lib.Mlp) == 16 * 32 + 24 and ctypes.sizeof(lib.MlpGrads) == 32 * 8
    assert tuple(L.a3vt_latent_policy_limit(i) for i in range(4)) == (4096, 1024, 16, 0)
    assert ops.LATENT_POLICY_MAX == dict(rows=4096, width=1024, layers=16)
    assert L.a3vt_latent_policy_stash_floats(ctypes.byref(net())) == 200 + 100 + 200 + 200 + 200 + 200 + 50
    assert L.a3vt_latent_policy_stash_floats(ctypes.byref(net(n_layers=17))) == 0
    assert L.a3vt_latent_policy_stash_floats(None) == 0


def test_launch_counter_reads_and_resets(L):
    buf = (ctypes.c_longlong * 3)()
    assert L.a3vt_latent_policy_launches(buf, 1) == 3 and L.a3vt_latent_policy_launches(buf, 0) == 3 and list(buf) == [0, 0, 0]
    assert L.a3vt_latent_policy_launches(None, 0) == 3
    fwd(L, net(), rows=0)                                    # a refused call launches nothing
    L.a3vt_latent_policy_launches(buf, 0)
    assert list(buf) == [0, 0, 0]


@pytest.mark.parametrize("kw,says", [
    (dict(n_layers=17), "n_layers=17"), (dict(n_layers=1), "n_layers=1"), (dict(n_layers=0), "n_layers=0"),
    (dict(concat_at=0), "concat_at=0"), (dict(concat_at=7), "concat_at=7"), (dict(latent_size=0), "latent_size=0"),
    (dict(latent_size=342), "latent_size=342"), (dict(transform=2), "transform=2"),
    (dict(dims=[(50, 200, 1), (200, 100, 1), (100, 200, 0), (600, 1025, 1), (1025, 50, 0)]), "out=1025"),
    (dict(dims=[(0, 200, 1), (200, 100, 1), (100, 200, 0), (600, 50, 0)]), "in=0"),
    (dict(dims=[(50, 200, 1), (200, 100, 1), (100, 200, 0), (599, 50, 0)]), "layer 3 in=599"),
    (dict(dims=[(50, 200, 1), (199, 100, 1), (100, 200, 0), (600, 50, 0)]), "layer 1 in=199"),
    (dict(latent_size=100), "layer 3 in=600"),
    (dict(weight_offset=4), "misaligned"),
])
def test_the_table_is_checked(L, kw, says):
    m = net(**kw)
    for rc, msg in (fwd(L, m), bwd(L, m, grads())):
        assert rc != 0 and "latent_policy" in msg and says in msg, (kw, msg)


def test_scalar_rows_need_only_four_byte_alignment(L):
    dims = [(7, 5, 1), (5, 3, 0), (5, 7, 0)]
    ok = net(dims=dims, concat_at=2, latent_size=1, weight_offset=4)
    rc, msg = fwd(L, ok, rows=0)                              # (passes the table, is refused for its rows)
    assert rc != 0 and "rows=0" in msg
    rc, msg = fwd(L, net(dims=dims, concat_at=2, latent_size=1, weight_offset=2), rows=0)
    assert rc != 0 and "misaligned" in msg


def test_rows_and_pointers(L):
    m = net()
    assert fwd(L, None)[0] != 0 and "net is null" in fwd(L, None)[1]
    for rows in (0, -1, 4097):
        rc, msg = fwd(L, m, rows=rows)
        assert rc != 0 and f"rows={rows}" in msg
        rc, msg = bwd(L, m, grads(), rows=rows)
        assert rc != 0 and f"rows={rows}" in msg
    for name in ("mask", "latent", "first_latent", "values"):
        rc, msg = fwd(L, m, **{name: None})
        assert rc != 0 and "argument check failed" in msg, name
    for missing in (("taken",), ("action",)):                 # the choice needs both; neither is fine (refused later for the fake rows)
        rc, msg = fwd(L, m, **{k: None for k in missing})
        assert rc != 0 and "argument check failed" in msg, missing
    rc, msg = fwd(L, m, mask=FWD["mask"] + 2)
    assert rc != 0 and "aligned_to" in msg
    for name in ("mask", "latent", "first_latent", "dvalues", "stash", "delta"):
        rc, msg = bwd(L, m, grads(), **{name: None})
        assert rc != 0 and "argument check failed" in msg, name
    assert bwd(L, m, None)[0] != 0
    rc, msg = bwd(L, m, grads(missing=4))
    assert rc != 0 and "layer 4 dweight" in msg


@pytest.mark.parametrize("name,values", [("steps", (0, -1, 4097)), ("rows", (0, -2, 4097)), ("num_actions", (0, -1, 1025))])
def test_loss_limits(L, name, values):
    for v in values:
        rc, msg = loss(L, **{name: v})
        assert rc != 0 and "action_value_loss" in msg and f"{name}={v}" in msg, (name, v, msg)


def test_loss_pointers(L):
    for name in ("values", "actions", "targets", "loss", "dvalues"):
        rc, msg = loss(L, **{name: None})
        assert rc != 0 and "argument check failed" in msg, name
        rc, msg = loss(L, **{name: FAKE + 0x10002})
        assert rc != 0 and "aligned_to" in msg, name
