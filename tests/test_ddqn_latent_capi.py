"""CPU tests (no GPU, no compute): ``a3vt_ddqn_latent_q`` / ``a3vt_ddqn_latent_update`` / ``a3vt_ddqn_latent_scratch_bytes`` refuse
what the contract in ``include/a3vt.h`` excludes with an error code and a message that names the value, before anything is
launched — every call below passes fake device addresses that must never be dereferenced on the host (the manner of
``test_latent_policy_capi.py``) — and the torch forms of ``ops.ddqn_latent_q`` / ``ops.ddqn_latent_update`` against the composition
of the existing torch forms."""
import ctypes

import numpy as np
import pytest
import torch

FAKE = 0x7F0000001000        # a "device pointer": 16-byte aligned, never mapped on the host
DIMS = [(50, 200, 1), (200, 100, 1), (100, 200, 0), (600, 200, 1), (200, 200, 1), (200, 200, 1), (200, 50, 0)]     # t_p's Latent_Model


@pytest.fixture(scope="module")
def L():
    from a3vt_amd import lib
    return lib.load()


def net(dims=DIMS, concat_at=3, latent_size=200, transform=0, n_layers=None, weight_offset=0, base=0):
    from a3vt_amd import lib
    m = lib.Mlp()
    for l, (n_in, n_out, relu) in enumerate(dims):
        m.layer[l] = lib.MlpLayer(FAKE + base + 0x100000 * l + weight_offset, FAKE + base + 0x100000 * l + 0x80000, n_in, n_out, relu, 0)
    m.n_layers, m.concat_at, m.latent_size, m.transform = len(dims) if n_layers is None else n_layers, concat_at, latent_size, transform
    m.scale, m.offset = 1.0, 0.0
    return m


def grads(n=7, missing=None):
    from a3vt_amd import lib
    g = lib.MlpGrads()
    for l in range(n):
        g.dweight[l], g.dbias[l] = FAKE + 0x4000000 + 0x100000 * l, FAKE + 0x4000000 + 0x100000 * l + 0x80000
    if missing is not None:
        g.dweight[missing] = None
    return g


Q = dict(mask=FAKE + 0x9000000, latent=FAKE + 0x9100000, first_latent=FAKE + 0x9200000, mask_penalty=FAKE + 0x9300000, rows=3,
         q=FAKE + 0x9400000, action=FAKE + 0x9500000, stream=None)
UPD_ORDER = ("mask", "mask_n", "latent", "latent_n", "first_latent", "actions", "rewards", "denom", "batch", "budget", "gamma", "q_cur",
             "best_next", "target", "diff", "loss", "scratch", "stream")
UPD = dict(mask=FAKE + 0xA000000, mask_n=FAKE + 0xA100000, latent=FAKE + 0xA200000, latent_n=FAKE + 0xA300000,
           first_latent=FAKE + 0xA400000, actions=FAKE + 0xA500000, rewards=FAKE + 0xA600000, denom=FAKE + 0xA700000, batch=16, budget=5,
           gamma=0.9, q_cur=FAKE + 0xA800000, best_next=FAKE + 0xA900000, target=FAKE + 0xAA00000, diff=FAKE + 0xAB00000,
           loss=FAKE + 0xAC00000, scratch=FAKE + 0xAD00000, stream=None)


def q_call(L, m, **changes):
    a = dict(Q, **changes)
    rc = L.a3vt_ddqn_latent_q(ctypes.byref(m) if m is not None else None,
                              *(a[k] for k in ("mask", "latent", "first_latent", "mask_penalty", "rows", "q", "action", "stream")))
    return rc, L.a3vt_last_error().decode()


def upd_call(L, online, target_net, g, **changes):
    a = dict(UPD, **changes)
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    rc = L.a3vt_ddqn_latent_update(ref(online), ref(target_net), ref(g), *(a[k] for k in UPD_ORDER))
    return rc, L.a3vt_last_error().decode()


def counts(L, reset=0):
    buf = (ctypes.c_longlong * 2)()
    assert L.a3vt_ddqn_latent_launches(buf, reset) == 2
    return list(buf)


def test_source_signatures_and_scratch(L):
    from a3vt_amd import lib
    assert "ddqn_latent.hip" in lib.SOURCES
    for name in ("a3vt_ddqn_latent_q", "a3vt_ddqn_latent_update", "a3vt_ddqn_latent_scratch_bytes", "a3vt_ddqn_latent_launches"):
        assert name in lib.SIGNATURES
    ld = 200 + 100 + 200 + 200 + 200 + 200 + 50
    assert L.a3vt_ddqn_latent_scratch_bytes(ctypes.byref(net()), 16) == 16 * (2 * 50 + 2 * ld) * 4
    assert L.a3vt_ddqn_latent_scratch_bytes(ctypes.byref(net()), 4096) == 4096 * (2 * 50 + 2 * ld) * 4
    for batch in (0, -1, 4097):
        assert L.a3vt_ddqn_latent_scratch_bytes(ctypes.byref(net()), batch) == 0 and f"batch={batch}" in L.a3vt_last_error().decode()
    assert L.a3vt_ddqn_latent_scratch_bytes(ctypes.byref(net(transform=1)), 16) == 0
    assert L.a3vt_ddqn_latent_scratch_bytes(None, 16) == 0


def test_a_refused_call_launches_nothing(L):
    counts(L, reset=1)
    assert counts(L) == [0, 0] and L.a3vt_ddqn_latent_launches(None, 0) == 2
    q_call(L, net(), rows=0)
    upd_call(L, net(), net(base=0x1000000), grads(), batch=0)
    assert counts(L) == [0, 0]


@pytest.mark.parametrize("kw,says", [
    (dict(n_layers=17), "n_layers=17"), (dict(n_layers=1), "n_layers=1"), (dict(concat_at=0), "concat_at=0"), (dict(concat_at=7), "concat_at=7"),
    (dict(latent_size=0), "latent_size=0"), (dict(latent_size=342), "latent_size=342"), (dict(transform=2), "transform=2"),
    (dict(transform=1), "transform=1"),
    (dict(dims=[(50, 200, 1), (200, 100, 1), (100, 200, 0), (600, 1025, 1), (1025, 50, 0)]), "out=1025"),
    (dict(dims=[(305, 200, 1), (200, 100, 1), (100, 200, 0), (600, 305, 0)]), "num_actions=305"),
    (dict(dims=[(50, 200, 1), (200, 100, 1), (100, 200, 0), (599, 50, 0)]), "layer 3 in=599"),
    (dict(latent_size=100), "layer 3 in=600"),
    (dict(weight_offset=4), "misaligned"),
])
def test_the_table_is_checked(L, kw, says):
    bad = net(**kw)
    for rc, msg in (q_call(L, bad), upd_call(L, bad, net(base=0x1000000), grads()), upd_call(L, net(), bad, grads())):
        assert rc != 0 and "ddqn_latent" in msg and says in msg, (kw, msg)


def test_online_and_target_must_agree(L):
    other = [(50, 200, 1), (200, 100, 1), (100, 200, 0), (600, 100, 1), (100, 100, 1), (100, 100, 1), (100, 50, 0)]
    rc, msg = upd_call(L, net(), net(dims=other, base=0x1000000), grads())
    assert rc != 0 and "layer 3 of the target net" in msg and "out=100" in msg
    rc, msg = upd_call(L, net(), net(dims=DIMS[:3] + [(600, 200, 1), (200, 50, 0)], base=0x1000000), grads())
    assert rc != 0 and "n_layers=5" in msg
    relu = list(DIMS)
    relu[4] = (200, 200, 0)
    rc, msg = upd_call(L, net(), net(dims=relu, base=0x1000000), grads())
    assert rc != 0 and "layer 4 of the target net" in msg
    wide = [(60, 200, 1)] + DIMS[1:]                      # the mask feeds the network AND penalises the actions: in must be A
    rc, msg = upd_call(L, net(dims=wide), net(dims=wide, base=0x1000000), grads())
    assert rc != 0 and "in=60" in msg and "num_actions=50" in msg
    assert q_call(L, net(dims=wide), rows=0)[1].count("rows=0") == 1      # (the q entry point takes such a table: refused for its rows)


def test_rows_batch_and_pointers(L):
    m, t = net(), net(base=0x1000000)
    assert q_call(L, None)[0] != 0 and "net is null" in q_call(L, None)[1]
    assert upd_call(L, None, t, grads())[0] != 0 and upd_call(L, m, None, grads())[0] != 0 and "net is null" in upd_call(L, m, None, grads())[1]
    for v in (0, -1, 4097):
        rc, msg = q_call(L, m, rows=v)
        assert rc != 0 and f"rows={v}" in msg
        rc, msg = upd_call(L, m, t, grads(), batch=v)
        assert rc != 0 and f"batch={v}" in msg
    for name in ("mask", "latent", "first_latent", "q"):
        rc, msg = q_call(L, m, **{name: None})
        assert rc != 0 and "argument check failed" in msg, name
    for missing in (("mask_penalty",), ("action",)):               # the choice needs both or neither
        rc, msg = q_call(L, m, **{k: None for k in missing})
        assert rc != 0 and "argument check failed" in msg, missing
    rc, msg = q_call(L, m, mask=Q["mask"] + 2)
    assert rc != 0 and "aligned_to" in msg
    for name in UPD_ORDER:
        if name in ("batch", "budget", "gamma", "stream", "denom"):
            continue
        rc, msg = upd_call(L, m, t, grads(), **{name: None})
        assert rc != 0 and "argument check failed" in msg, name
        rc, msg = upd_call(L, m, t, grads(), **{name: UPD[name] + 2})
        assert rc != 0 and "aligned_to" in msg, name
    rc, msg = upd_call(L, m, t, grads(), denom=UPD["denom"] + 2)     # denom may be null, not misaligned
    assert rc != 0 and "aligned_to" in msg
    assert upd_call(L, m, t, None)[0] != 0
    rc, msg = upd_call(L, m, t, grads(missing=4))
    assert rc != 0 and "layer 4 dweight" in msg


# ---- the torch forms ---------------------------------------------------------------------------------------------------------------
def _tables(A, ls, hidden, layers, seed):
    from a3vt_amd import ops
    g = torch.Generator().manual_seed(seed)
    dims = [(A, 11, 1), (11, 6, 1), (6, ls, 0)] + [((3 * ls if i == 0 else hidden), (A if i == layers - 1 else hidden), int(i < layers - 1))
                                                    for i in range(layers)]
    make = lambda: ops.PolicyTable([(torch.randn(o, i, generator=g) / np.sqrt(i), torch.randn(o, generator=g) * 0.1, r)  # noqa: E731
                                    for i, o, r in dims], 3, None)
    return make(), make()


@pytest.mark.parametrize("denom", [False, True])
@pytest.mark.parametrize("gamma", [0.0, 0.9])
def test_torch_forms_against_the_existing_torch_forms(gamma, denom):
    from a3vt_amd import ops
    A, ls, B = 7, 5, 9
    online, target = _tables(A, ls, 8, 2, 0)
    g = torch.Generator().manual_seed(1)
    mask = (torch.rand(B, A, generator=g) < 0.3).float()
    mask[0] = 1                                                   # every action taken
    mask[1] = 0
    actions = torch.randint(0, A, (B,), generator=g).float()
    actions[2], actions[3] = -2.0, A + 3.0                        # outside the table: clamped, as ops.ddqn_td
    mask_n = mask.clone()
    mask_n[torch.arange(B), actions.long().clamp(0, A - 1)] = 1
    latent, latent_n, first = (torch.randn(B, ls, generator=g) for _ in range(3))
    rewards = torch.rand(B, generator=g)
    den = 1 + torch.rand(B, generator=g) if denom else None
    # the composition of the existing forms, under autograd
    live = [p.clone().requires_grad_(True) for p in online.params()]
    t = ops.PolicyTable([(live[2 * l], live[2 * l + 1], r) for l, (_, _, r) in enumerate(online.layers)], 3, None)
    q_cur, _ = ops.latent_policy(t, mask, latent, first)
    with torch.no_grad():
        q_no, _ = ops.latent_policy(online, mask_n, latent_n, first)
        q_nt, _ = ops.latent_policy(target, mask_n, latent_n, first)
    loss, best, tgt = ops.ddqn_td(q_cur, q_no, q_nt, mask, actions, rewards, den, 4, gamma)
    loss.backward()
    grads = [(torch.full_like(w, 3.0), torch.full_like(b, 3.0)) for w, b, _ in online.layers]
    got = ops.ddqn_latent_update(online, target, grads, mask, mask_n, latent, latent_n, first, actions, rewards, den, 4, gamma)
    assert torch.equal(got[0], loss.detach()) and torch.equal(got[1], q_cur.detach()) and torch.equal(got[2], best) and torch.equal(got[3], tgt)
    assert torch.equal(got[4], q_cur.detach().gather(1, actions.long().clamp(0, A - 1)[:, None]).squeeze(1) - tgt)
    for l, (dw, db) in enumerate(grads):
        assert torch.equal(dw, live[2 * l].grad) and torch.equal(db, live[2 * l + 1].grad), l
    assert all(not x.requires_grad for x in got)
    assert best[0] == 0                                            # every action taken: index 0
    q, action = ops.ddqn_latent_q(online, mask, latent, first, mask)
    want_q, _ = ops.latent_policy(online, mask, latent, first)
    assert torch.equal(q, want_q) and action.dtype == torch.int32
    assert torch.equal(action.long(), want_q.masked_fill(mask > 0, -1e10).argmax(1)) and action[0] == 0
    assert ops.ddqn_latent_q(online, mask, latent, first)[1] is None


def test_ops_refuse_disagreeing_operands():
    from a3vt_amd import ops
    online, target = _tables(7, 5, 8, 2, 0)
    other, _ = _tables(7, 5, 9, 2, 0)
    B = 3
    mask, latent, vec = torch.zeros(B, 7), torch.zeros(B, 5), torch.zeros(B)
    grads = [(torch.zeros_like(w), torch.zeros_like(b)) for w, b, _ in online.layers]
    good = dict(mask=mask, mask_n=mask, latent=latent, latent_n=latent, first_latent=latent, actions=vec, rewards=vec, denom=None)

    def call(tgt=target, g=grads, **kw):
        a = dict(good, **kw)
        return ops.ddqn_latent_update(online, tgt, g, a["mask"], a["mask_n"], a["latent"], a["latent_n"], a["first_latent"], a["actions"],
                                      a["rewards"], a["denom"], 5, 0.0)
    call()
    for kw in (dict(mask_n=mask[:2]), dict(latent_n=latent[:, :4]), dict(actions=vec[:2]), dict(rewards=vec.double()), dict(denom=vec[:1]),
               dict(actions=vec.long())):
        with pytest.raises(RuntimeError, match="a3vt: (ddqn_latent_update|latent_policy)"):
            call(**kw)
    with pytest.raises(RuntimeError, match="same layers"):
        call(tgt=other)
    with pytest.raises(RuntimeError, match="gradient 1"):
        call(g=[grads[0], (grads[1][0][:, :2], grads[1][1])] + grads[2:])
    with pytest.raises(RuntimeError, match="one \\(dweight, dbias\\) pair per layer"):
        call(g=grads[:-1])
    with pytest.raises(RuntimeError, match="mask_penalty"):
        ops.ddqn_latent_q(online, mask, latent, latent, mask[:, :6])
    assert not ops.ddqn_latent_supported(online, mask)            # CPU operands: the torch form
