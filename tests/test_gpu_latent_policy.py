"""``ops.latent_policy`` / ``ops.action_value_loss`` (csrc/latent_policy.hip) on the GPU against ``supervised_util``, a literal
fp64 restatement of the contracts in ``include/a3vt.h``.

Shapes (``CASES``): num_actions 1, 6, 7, 50; latent_size 1, 5, 200; value-network layers 1 (a single Linear(3L -> A)), 2, 4;
hidden_dim 5, 200, 257; rows 1, 2, 3, 65; the three output transforms and none.  Between them: ``in % 4 != 0`` (7, 3, 15, 5, 257:
scalar loads), ``in < 64`` (a wave with idle lanes), 257 = one past a multiple of 256 (a lane's second column group holds one
column), the concat at offsets 1, 5 (odd) and 200, and more rows than one workgroup's worth of anything.

Tolerance, per case and per tensor: the kernel's largest error against fp64 may be at most 4 times the largest error of the torch
fp32 ops (``ops._latent_policy_torch`` on the GPU: the modules' F.linear chain, and autograd through it) against the same fp64 —
the cap the touch stem's test uses — with the contract's own bound (``supervised_util``'s docstring derives it) as the floor.
Every test prints the figures it asserts on.  Measured on an MI355X: kernel / torch ratios of 0.38 - 1.05 for the values and
0.15 - 3.9 for the 102 gradients (median 1.0), no error above 8 % of the floor."""
import functools

import numpy as np
import pytest
import torch

import supervised_util as su

pytestmark = pytest.mark.gpu

from a3vt_amd import ops  # noqa: E402

# (num_actions, latent_size, layers, hidden_dim, rows, transform)
CASES = [(50, 200, 4, 200, 3, "plain"), (50, 200, 4, 200, 65, "normalize"), (7, 5, 2, 5, 2, "use_img"), (6, 1, 1, 5, 1, "none"),
         (1, 5, 4, 257, 3, "plain"), (7, 200, 2, 257, 2, "none"), (50, 5, 4, 200, 1, "normalize"), (6, 200, 1, 200, 3, "use_img"),
         (1, 1, 2, 5, 65, "none")]
IDS = ["A%d-L%d-n%d-h%d-E%d-%s" % c for c in CASES]


@functools.lru_cache(maxsize=None)
def case(i, choice_gap=1e-3):
    A, Ls, layers, hidden, rows, tr = CASES[i]
    c = su.make_case(500 + i, rows, A, Ls, layers, hidden, su.TRANSFORMS[tr], min_choice_gap=choice_gap)
    c["dvalues"] = c["rng"].standard_normal(c["values"].shape).astype(np.float32)
    c["grads"], c["grad_bounds"] = su.backward(c["net"], c["mask"], c["latent"], c["first_latent"], c["dvalues"], c["stash"], c["bounds"])
    return c


def dev(cuda, a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(cuda)


def table(cuda, net, grad=False):
    layers, concat_at, transform = net
    return ops.PolicyTable([(dev(cuda, W).requires_grad_(grad), dev(cuda, b).requires_grad_(grad), relu) for W, b, relu in layers],
                           concat_at, transform)


def operands(cuda, c):
    return dev(cuda, c["mask"]), dev(cuda, c["latent"]), dev(cuda, c["first_latent"])


def capped(what, kernel, torch_, exact, bound):
    ek, et = float(np.abs(kernel - exact).max()), float(np.abs(torch_ - exact).max())
    floor = float(np.max(bound))
    print(f"{what}: kernel {ek:.3e}, torch {et:.3e} (ratio {ek / et if et else float('inf'):.2f}), contract bound {floor:.3e}")
    assert ek <= max(4 * et, floor), f"{what}: kernel error {ek:.3e} > max(4 x {et:.3e}, {floor:.3e})"


def test_limits_are_the_library_s():
    from a3vt_amd import lib
    L = lib.load()
    assert tuple(L.a3vt_latent_policy_limit(i) for i in range(3)) == tuple(ops.LATENT_POLICY_MAX[k] for k in ("rows", "width", "layers"))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_forward_and_choice(cuda, i):
    c = case(i)
    gap = su.eligible_gap(c["values"], c["mask"])
    assert gap >= 1e-3, f"the reference's two lowest open values are only {gap:.2e} apart"
    t = table(cuda, c["net"])
    mask, latent, first = operands(cuda, c)
    assert ops.policy_supported(t, mask)
    values, action = ops.latent_policy(t, mask, latent, first, mask)
    with torch.no_grad():
        tv, _ = ops._latent_policy_torch(t, mask, latent, first, None)
    capped(IDS[i] + " values", values.cpu().numpy().astype(np.float64), tv.cpu().numpy().astype(np.float64), c["values"], c["value_bound"])
    assert action.dtype == torch.int32 and np.array_equal(action.cpu().numpy(), su.choose(c["values"], c["mask"]))
    plain, none = ops.latent_policy(t, mask, latent, first)
    assert none is None and torch.equal(plain, values)          # (the values are unmasked either way)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_backward(cuda, i):
    c = case(i)
    mask, latent, first = operands(cuda, c)
    dvalues = dev(cuda, c["dvalues"])
    got = []
    for fused in (True, False):
        t = table(cuda, c["net"], grad=True)
        values = (ops.latent_policy if fused else ops._latent_policy_torch)(t, mask, latent, first, None)[0]
        values.backward(dvalues)
        got.append([p.grad.cpu().numpy().astype(np.float64) for p in t.params()])
    for l, ((dW, db), (bW, bb)) in enumerate(zip(c["grads"], c["grad_bounds"])):
        capped(f"{IDS[i]} dW{l}", got[0][2 * l], got[1][2 * l], dW, bW)
        capped(f"{IDS[i]} db{l}", got[0][2 * l + 1], got[1][2 * l + 1], db, bb)


def _choice(cuda, values, taken):
    """The kernel's choice over given values.  The choice is part of the forward, so the values come out of a network that
    reproduces them exactly: zero weights and the values as the last bias (0 * x + b = b for finite x, whatever b is)."""
    E, A = values.shape
    assert E == 1
    layers = [(np.zeros((4, A), np.float32), np.zeros(4, np.float32), True),
              (np.zeros((A, 4 + 2), np.float32), values[0].astype(np.float32), False)]
    t = table(cuda, (layers, 1, None))
    z = torch.zeros((1, 1), device=cuda)
    out, action = ops.latent_policy(t, dev(cuda, np.zeros((1, A), np.float32)), z, z, dev(cuda, taken))
    assert np.array_equal(out.cpu().numpy(), values.astype(np.float32), equal_nan=True)
    return int(action.cpu()[0])


def test_choice_edges(cuda):
    nan, inf = float("nan"), float("inf")
    rows = [([3.0, 1.0, 1.0, 2.0], [0, 0, 0, 0], 1),                 # an exact tie goes to the lower index
            ([-0.0, 0.0, 5.0, 5.0], [1, 0, 0, 0], 1), ([0.0, -0.0, 5.0, 5.0], [0, 0, 0, 0], 0),      # -0 == +0
            ([1.0, 2.0, 3.0, 4.0], [1, 1, 0, 1], 2),                 # all but one taken
            ([1.0, 2.0, 3.0, 4.0], [1, 1, 1, 1], -1),                # all taken
            ([nan, inf, nan, inf], [0, 0, 0, 0], 1),                 # NaN sorts after +inf
            ([nan, inf, nan, inf], [0, 1, 0, 1], 0), ([nan, -inf, 7.0, inf], [0, 0, 0, 0], 1), ([nan, -inf, 7.0, inf], [0, 1, 1, 0], 3),
            ([-1.0, -2.0, -3.0, -2.5], [0, 0, 1, 0], 3)]
    for values, taken, want in rows:
        v, t = np.array([values]), np.array([taken], dtype=np.float32)
        assert su.choose(v, t)[0] == want, (values, taken)
        assert _choice(cuda, v, t) == want, (values, taken)
        assert int(ops.choose_action_torch(torch.tensor(v, dtype=torch.float32), torch.tensor(t))[0]) == want, (values, taken)
    wide = np.zeros((1, 130))                                         # more actions than lanes: the tie still goes to the lowest
    wide[0, :3] = 1.0
    assert _choice(cuda, wide, np.zeros((1, 130), np.float32)) == 3


@pytest.mark.parametrize("i", [0, 2, 4], ids=[IDS[0], IDS[2], IDS[4]])
def test_bits_do_not_depend_on_the_rows(cuda, i):
    A, Ls, layers, hidden, _, tr = CASES[i]
    c = su.make_case(900 + i, 5, A, Ls, layers, hidden, su.TRANSFORMS[tr])
    t = table(cuda, c["net"])
    mask, latent, first = operands(cuda, c)
    run = lambda rows: ops.latent_policy(t, mask[rows], latent[rows], first[rows], mask[rows])      # noqa: E731
    every = list(range(5))
    values, action = run(every)
    again = run(every)
    assert torch.equal(values, again[0]) and torch.equal(action, again[1])                   # a second call
    for e in every:                                                                           # a row evaluated alone
        alone = run([e])
        assert torch.equal(alone[0][0], values[e]) and alone[1][0] == action[e]
    longer = run(every + [0, 3] * 40)                                                         # rows appended
    assert torch.equal(longer[0][:5], values) and torch.equal(longer[1][:5], action)
    perm = [3, 0, 4, 2, 1]                                                                    # rows permuted
    moved = run(perm)
    assert torch.equal(moved[0], values[perm]) and torch.equal(moved[1], action[perm])


@pytest.mark.parametrize("steps", [1, 5])
def test_loss(cuda, steps):
    g = np.random.default_rng(70 + steps)
    E, A = 3, 7
    values = g.standard_normal((E, A)).astype(np.float32)
    actions = g.integers(0, A, (steps, E))
    if steps > 1:
        actions[1] = actions[0]                  # repeated (e, a) pairs ...
        actions[4, 0] = actions[0, 0]            # ... also three of a kind
    targets = g.standard_normal((steps, E)).astype(np.float32)
    want_loss, want_d = su.loss(values, actions, targets)
    v = dev(cuda, values).requires_grad_(True)
    loss, dvalues = ops.action_value_loss(v, actions, dev(cuda, targets))
    el = abs(float(loss.detach()) - want_loss) / want_loss
    term = lambda v, a, t: float(np.abs(v[np.arange(v.shape[0])[None, :], a] - t).max()) * 2.0 / a.size      # noqa: E731
    ed = float(np.abs(dvalues.cpu().numpy() - want_d).max()) / (steps * term(values, actions, targets))
    print(f"T {steps}: loss error {el:.2e} relative, dvalues error {ed:.2e} of an entry's largest possible sum of terms")
    # a sum of T*E squares, and per entry of at most T terms: one rounding per difference, product, factor and addition
    assert el <= (steps * E + 4) * su.U and ed <= (steps + 4) * su.U
    loss.backward()
    assert torch.equal(v.grad, dvalues)
    again = ops.action_value_loss(v.detach(), torch.from_numpy(actions).to(cuda), dev(cuda, targets))     # (device actions: same bits)
    assert torch.equal(again[0], loss.detach()) and torch.equal(again[1], dvalues)
    big = np.random.default_rng(3)                # several workgroups of rows
    values, actions, targets = big.standard_normal((40, 50)).astype(np.float32), big.integers(0, 50, (steps, 40)), \
        big.standard_normal((steps, 40)).astype(np.float32)
    want_loss, want_d = su.loss(values, actions, targets)
    loss, dvalues = ops.action_value_loss(dev(cuda, values), actions, dev(cuda, targets))
    assert abs(float(loss) - want_loss) / want_loss <= (steps * 40 + 4) * su.U
    assert float(np.abs(dvalues.cpu().numpy() - want_d).max()) <= (steps + 4) * su.U * steps * term(values, actions, targets)


def test_loss_refusals(cuda):
    values, targets = torch.zeros((3, 7), device=cuda), torch.zeros((5, 3), device=cuda)
    ok = np.zeros((5, 3), dtype=np.int64)
    for bad in (np.full((5, 3), 7), np.full((5, 3), -1), torch.full((5, 3), 7, device=cuda)):
        with pytest.raises(RuntimeError, match="outside"):
            ops.action_value_loss(values, bad, targets)
    for v, a, t in ((values, ok[:4], targets), (values, ok, targets[:, :2]), (values[:2], ok, targets), (values, ok.astype(np.float32), targets),
                    (values, ok, targets.double()), (values, ok, targets.cpu())):
        with pytest.raises(RuntimeError):
            ops.action_value_loss(v, a, t)


def test_accumulate_and_repeat(cuda):
    c = case(2)
    t = table(cuda, c["net"])
    mask, latent, first = operands(cuda, c)
    dvalues = dev(cuda, c["dvalues"])
    _, _, stash = ops.latent_policy_fwd(t, mask, latent, first, None, stash=True)

    def grads(fill, accumulate):
        out = [(torch.full_like(w, fill), torch.full_like(b, fill)) for w, b, _ in t.layers]
        ops.latent_policy_bwd(t, mask, latent, first, dvalues, stash, out, accumulate)
        return [x for pair in out for x in pair]
    off, off2 = grads(float("nan"), False), grads(7.0, False)
    on_zero, on_three = grads(0.0, True), grads(3.0, True)
    for a, b, z, h in zip(off, off2, on_zero, on_three):
        assert torch.equal(a, b)                         # overwritten whatever was there; the same bits on a second call
        assert torch.equal(z, a)                         # accumulate onto zeros: bit for bit the overwrite
        assert torch.equal(h, a + 3.0)                   # ... and onto anything else: the previous contents plus the sum


def test_launch_counts(cuda):
    c = case(2)
    t = table(cuda, c["net"], grad=True)
    mask, latent, first = operands(cuda, c)
    ops.policy_launches(reset=True)
    with torch.no_grad():
        ops.latent_policy(t, mask, latent, first, mask)
    assert ops.policy_launches() == {"fwd": 1, "loss": 0, "bwd": 0}
    values, _ = ops.latent_policy(t, mask, latent, first, mask)
    loss, _ = ops.action_value_loss(values, np.zeros((5, mask.shape[0]), dtype=np.int64), torch.zeros((5, mask.shape[0]), device=cuda))
    loss.backward()
    assert ops.policy_launches(reset=True) == {"fwd": 2, "loss": 1, "bwd": 2}


def test_outside_the_limits_the_torch_form_runs(cuda):
    g = np.random.default_rng(5)
    net = su.make_net(g, 6, 400, 2, 8, None)              # 3 * latent_size = 1200 > 1024
    t = table(cuda, net)
    mask, latent, first = (dev(cuda, a) for a in su.make_inputs(g, 2, 6, 400))
    assert not ops.policy_supported(t, mask)
    ops.policy_launches(reset=True)
    values, action = ops.latent_policy(t, mask, latent, first, mask)
    assert ops.policy_launches()["fwd"] == 0 and values.shape == (2, 6) and action.shape == (2,)
    with pytest.raises(RuntimeError, match="latent_size=400"):
        ops.latent_policy_fwd(t, mask, latent, first)


def test_model_knob_on_against_off(cuda, tmp_path):
    """``Latent_Model`` with ``fused_policy`` against the same weights without it: output, action choice and every ``.grad``,
    both against the fp64 restatement at the cap of the kernel tests; one launch forward, two backward."""
    import json
    from types import SimpleNamespace
    from a3vt_amd.pterotactyl.policies.supervised import model as sm
    (tmp_path / "config.json").write_text(json.dumps({"encoding_size": 200, "check_point": str(tmp_path)}))
    kw = dict(auto_location=str(tmp_path) + "/", num_actions=50, hidden_dim=200, layers=4, normalize=0, use_img=False)
    torch.manual_seed(11)
    off = sm.Latent_Model(SimpleNamespace(**kw)).to(cuda)
    on = sm.Latent_Model(SimpleNamespace(fused_policy=True, **kw)).to(cuda)
    on.load_state_dict(off.state_dict())
    assert on.fused_policy and not off.fused_policy
    t = on.table()
    net = ([(w.detach().cpu().numpy(), b.detach().cpu().numpy(), relu) for w, b, relu in t.layers], t.concat_at, t.transform)
    for seed in range(64):                          # inputs by the recipe of make_case: ReLU units and the choice away from their edges
        g = np.random.default_rng(1100 + seed)
        mask, latent, first = su.make_inputs(g, 3, 50, 200)
        values, stash, bounds, vbound, gap = su.forward(net, mask, latent, first)
        if gap >= su.RELU_MARGIN and su.eligible_gap(values, mask) >= 1e-3:
            break
    assert gap >= su.RELU_MARGIN and su.eligible_gap(values, mask) >= 1e-3
    obs = {"mask": torch.from_numpy(mask), "latent": torch.from_numpy(latent), "first_latent": torch.from_numpy(first)}   # host, as the environment's
    ops.policy_launches(reset=True)
    v_on, v_off = on(obs), off(obs)
    assert ops.policy_launches() == {"fwd": 1, "loss": 0, "bwd": 0}
    capped("model values", v_on.detach().cpu().numpy().astype(np.float64), v_off.detach().cpu().numpy().astype(np.float64), values, vbound)
    dvalues = g.standard_normal(values.shape).astype(np.float32)
    v_on.backward(dev(cuda, dvalues))
    v_off.backward(dev(cuda, dvalues))
    assert ops.policy_launches() == {"fwd": 1, "loss": 0, "bwd": 2}
    grads, gbounds = su.backward(net, mask, latent, first, dvalues, stash, bounds)
    p_on, p_off = dict(on.named_parameters()), dict(off.named_parameters())
    assert list(p_on) == list(p_off) and len(p_on) == 2 * len(grads)
    wanted = [pair for (dW, db), (bW, bb) in zip(grads, gbounds) for pair in ((dW, bW), (db, bb))]        # in the parameters' order
    for (name, a), (want, bound) in zip(p_on.items(), wanted):
        capped(f"model {name}.grad", a.grad.cpu().numpy().astype(np.float64), p_off[name].grad.cpu().numpy().astype(np.float64), want, bound)
    with torch.no_grad():
        (_, a_on), (_, a_off) = on.evaluate(obs), off.evaluate(obs)
    assert np.array_equal(a_on.cpu().numpy(), su.choose(values, mask)) and torch.equal(a_on.cpu(), a_off.cpu())
