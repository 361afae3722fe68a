"""The trainer's optimizer step as one launch (a3vt_amd/optim.py -> a3vt_adam_step, csrc/adam.hip) against torch.optim.Adam — the
reference's ``optim.Adam(params, lr, weight_decay=0)`` + ``optimizer.step()``, pterotactyl/reconstruction/vision/train.py:64,148."""
import copy

import numpy as np
import pytest
import torch

import adam_ref as ar

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (3,), (4097,), (300, 300), (16, 3, 5, 5), (4096,), (8191,), (2, 4096), (300,), (448, 300)]


def _params(dev, seed, offset_views=False):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, sh in enumerate(SHAPES):
        n = 1
        for d in sh:
            n *= d
        if offset_views and i % 2 == 1:      # storage that does not start on a 16-byte boundary: the scalar path
            base = torch.randn(n + 1, generator=g).to(dev)
            p = base[1:].view(sh)
        else:
            p = torch.randn(sh, generator=g).to(dev)
        out.append(torch.nn.Parameter(p))
    return out


def _grads(params, seed):
    g = torch.Generator().manual_seed(seed)
    for p in params:
        p.grad = (torch.randn(p.shape, generator=g) * 0.1).to(p.device)


@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("offset_views", [False, True])
def test_library_adam_follows_torch_adam(weight_decay, offset_views):
    from a3vt_amd import optim as aopt
    dev = torch.device("cuda", 0)
    pa, pb = _params(dev, 0, offset_views), _params(dev, 0, offset_views)
    oa = aopt.Adam(pa, lr=3e-4, weight_decay=weight_decay)
    ob = torch.optim.Adam(pb, lr=3e-4, weight_decay=weight_decay, foreach=False, fused=False)
    for step in range(6):
        _grads(pa, 10 + step)
        _grads(pb, 10 + step)
        oa.step()
        ob.step()
    assert oa.library_steps == 6
    for a, b in zip(pa, pb):
        # the same operations in the same order; what is left is the compilers' choice of fused multiply-adds: a few ulps of the update
        torch.testing.assert_close(a.detach(), b.detach(), rtol=5e-7, atol=1e-8)     # (an ulp or two of the parameter itself)
        torch.testing.assert_close(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"], rtol=2e-6, atol=1e-8)
        torch.testing.assert_close(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"], rtol=2e-6, atol=1e-11)
        assert float(oa.state[a]["step"]) == 6.0


def test_library_adam_is_bit_repeatable_and_moves_the_parameters():
    from a3vt_amd import optim as aopt
    dev = torch.device("cuda", 0)
    runs = []
    for _ in range(2):
        ps = _params(dev, 3)
        before = [p.detach().clone() for p in ps]
        opt = aopt.Adam(ps, lr=1e-3)
        for step in range(3):
            _grads(ps, 20 + step)
            opt.step()
        runs.append([p.detach().clone() for p in ps])
        # Adam's first steps move an element by at most lr each, and by lr exactly in the very first one
        for p, b in zip(ps, before):
            d = (p.detach() - b).abs()
            assert float(d.max()) <= 3.01e-3 and float(d.mean()) > 5e-4
    assert all(torch.equal(x, y) for x, y in zip(*runs))


def test_state_dict_is_interchangeable_with_torch_adam():
    """A checkpoint of torch's Adam (plain or fused: the reference's optim file, train.py:213,262) continues in the library's and back."""
    from a3vt_amd import optim as aopt
    dev = torch.device("cuda", 0)
    for fused in (False, True):
        pt = _params(dev, 5)
        ot = torch.optim.Adam(pt, lr=3e-4, fused=fused) if fused else torch.optim.Adam(pt, lr=3e-4, foreach=False)
        for step in range(2):
            _grads(pt, 30 + step)
            ot.step()
        sd = copy.deepcopy(ot.state_dict())
        pl = [torch.nn.Parameter(p.detach().clone()) for p in pt]
        ol = aopt.Adam(pl, lr=3e-4)
        ol.load_state_dict(sd)
        _grads(pt, 40)
        _grads(pl, 40)
        ot.step()
        ol.step()
        assert ol.library_steps == 1
        for a, b in zip(pl, pt):
            torch.testing.assert_close(a.detach(), b.detach(), rtol=5e-7, atol=1e-8)
            assert float(ol.state[a]["step"]) == 3.0
        # and back: the library's state into torch's plain Adam
        pb = [torch.nn.Parameter(p.detach().clone()) for p in pl]
        ob = torch.optim.Adam(pb, lr=3e-4, foreach=False)
        ob.load_state_dict(copy.deepcopy(ol.state_dict()))
        _grads(pl, 41)
        _grads(pb, 41)
        ol.step()
        ob.step()
        for a, b in zip(pl, pb):
            torch.testing.assert_close(a.detach(), b.detach(), rtol=5e-7, atol=1e-8)


def test_parameters_without_gradients_and_late_joiners():
    from a3vt_amd import optim as aopt
    dev = torch.device("cuda", 0)
    pa, pb = _params(dev, 7), _params(dev, 7)
    oa = aopt.Adam(pa, lr=3e-4)
    ob = torch.optim.Adam(pb, lr=3e-4, foreach=False)
    for step in range(4):
        _grads(pa, 50 + step)
        _grads(pb, 50 + step)
        if step < 2:       # the last three tensors get their first gradient at step 2: their own step count from then on
            for ps in (pa, pb):
                for p in ps[-3:]:
                    p.grad = None
        oa.step()
        ob.step()
    for a, b in zip(pa, pb):
        torch.testing.assert_close(a.detach(), b.detach(), rtol=5e-7, atol=1e-8)
    assert float(oa.state[pa[-1]]["step"]) == 2.0 and float(oa.state[pa[0]]["step"]) == 4.0


# ---- one step from a prepared state against the rule in fp64 (adam_ref.py), element by element ----------------------------------------
# Parameter, gradient, exp_avg and exp_avg_sq are views into four flat buffers at offsets the test chooses; whatever lies between the
# tensors is a guard element.  One step, so errors do not compound and adam_ref.bound applies per element: the margin is
# adam_ref.margin (2 x the first-order bound + one denormal) and nothing else.
SENTINEL = 0x4B1DBEEF      # a guard's bits: a finite fp32 (1.03e7) beyond every clamp, so a stray step or a stray clamp changes them
ROLES = ("param", "grad", "exp_avg", "exp_avg_sq")


def _layout(specs):
    """specs: (numel, phase) per tensor; phase = the start's element offset modulo 4 (0: on a 16-byte boundary), None = the first
    free element -> (starts, buffer length).  At least one guard between neighbours, four in front and eight behind."""
    starts, at = [], 4
    for n, phase in specs:
        if phase is not None:
            at += (phase - at) % 4
        starts.append(at)
        at += n + 1
    return starts, at + 7


class _Step:
    """Builds the buffers, takes ONE optimizer step and keeps what went in and what came out, packed tensor after tensor."""

    def __init__(self, dev, specs, settings, seed, group_of=None, role_specs=None, poke=None, shapes=None):
        from a3vt_amd import optim as aopt
        self.sizes = [n for n, _ in specs]
        self.settings = settings
        group_of = [0] * len(specs) if group_of is None else group_of
        self.elem_group = np.repeat(np.asarray(group_of), self.sizes)
        self.bounds = np.concatenate([[0], np.cumsum(self.sizes)])
        rng = np.random.default_rng(seed)
        per = [ar.make_inputs(rng, n, settings[gi]) for n, gi in zip(self.sizes, group_of)]
        self.before = [np.concatenate([t[r] for t in per]) for r in range(4)]
        if poke is not None:
            poke(self)
        clamps = {s["grad_clamp"] for s in settings}
        assert len(clamps) == 1, "the clamp belongs to the optimizer, not to a group"
        self.grad_clamp = clamps.pop()
        layouts = [_layout(rs) for rs in (role_specs or [specs] * 4)]
        self.index, self.host, self.dev = [], [], []
        for (starts, length), packed in zip(layouts, self.before):
            idx = np.concatenate([np.arange(s, s + n) for s, n in zip(starts, self.sizes)])
            buf = np.full(length, SENTINEL, np.uint32)
            buf[idx] = packed.view(np.uint32)
            self.index.append(idx)
            self.host.append(buf)
            self.dev.append(torch.from_numpy(buf.view(np.int32)).to(dev).view(torch.float32))
        self.starts = [lay[0] for lay in layouts]
        assert all(t.data_ptr() % 16 == 0 for t in self.dev)
        shapes = shapes or [(n,) for n in self.sizes]
        views = [[self.dev[r][s:s + n].view(sh) for s, n, sh in zip(self.starts[r], self.sizes, shapes)] for r in range(4)]
        self.params = [torch.nn.Parameter(x) for x in views[0]]
        groups = []
        for gi, s in enumerate(settings):
            groups.append(dict(params=[p for p, g in zip(self.params, group_of) if g == gi], lr=s["lr"], betas=(s["beta1"], s["beta2"]),
                               eps=s["eps"], weight_decay=s["weight_decay"]))
        self.opt = aopt.Adam(groups, grad_clamp=self.grad_clamp)
        for r in range(4):
            assert [x.data_ptr() for x in views[r]] == [self.dev[r].data_ptr() + 4 * s for s in self.starts[r]]
        for p, g, m, v, gi in zip(self.params, views[1], views[2], views[3], group_of):
            p.grad = g
            self.opt.state[p] = {"step": torch.tensor(settings[gi]["step"] - 1.0), "exp_avg": m, "exp_avg_sq": v}
        self.opt.step()
        torch.cuda.synchronize()
        self.raw = [t.view(torch.int32).cpu().numpy().view(np.uint32) for t in self.dev]
        self.after = [raw[idx].view(np.float32) for raw, idx in zip(self.raw, self.index)]

    def guards_intact(self):
        ok = {}
        for role, raw, idx in zip(ROLES, self.raw, self.index):
            guard = np.ones(raw.size, bool)
            guard[idx] = False
            ok[role] = bool((raw[guard] == SENTINEL).all()) and int(guard.sum()) >= 11 + len(self.sizes)
        return ok

    def tensor_of(self, element):
        t = int(np.searchsorted(self.bounds, element, side="right") - 1)
        return f"tensor {t} (numel {self.sizes[t]}) element {int(element - self.bounds[t])}"

    def expected(self, gi, sel, **override):
        h = dict(ar.hyper(self.settings[gi]), **override)
        state = [x[sel] for x in self.before]
        return ar.step_fp64(*state, **h), ar.bound(*state, **h)

    def assert_within_margin(self, ignore=None, what=""):
        """Every element of p', m' and v' within adam_ref.margin of the fp64 rule -> the largest error / bound per output."""
        worst = [0.0, 0.0, 0.0]
        for gi, setting in enumerate(self.settings):
            sel = self.elem_group == gi
            if ignore is not None:
                sel = sel & ~ignore
            want, bnd = self.expected(gi, sel)
            where = np.flatnonzero(sel)
            for k, name in enumerate(("p", "m", "v")):
                err = np.abs(self.after[0 if k == 0 else k + 1][sel].astype(np.float64) - want[k])
                ratio = np.divide(err, bnd[k], out=np.where(err > 0, np.inf, 0.0), where=bnd[k] > 0)
                i = int(np.nanargmax(ratio)) if ratio.size else 0
                assert np.isfinite(bnd[k]).all()
                assert (err <= ar.margin(bnd[k])).all(), (f"{what}{setting['name']} {name}': error / bound {ratio[i]:.3f} at "
                                                          f"{self.tensor_of(where[i])}, {int((err > ar.margin(bnd[k])).sum())} elements outside")
                worst[k] = max(worst[k], float(ratio[i]) if ratio.size else 0.0)
        return worst


RULE_SPECS = [(1, 0), (3, 0), (4095, 0), (4096, 0), (4097, 0), (2 * 4096, 0), (8191, 0), (300 * 300, 0)]
RULE_SHAPES = [(1,), (3,), (4095,), (4096,), (4097,), (2, 4096), (8191,), (300, 300)]


@pytest.mark.parametrize("si", range(len(ar.SETTINGS)), ids=[s["name"] for s in ar.SETTINGS])
def test_one_step_follows_the_rule_in_fp64(si):
    run = _Step(torch.device("cuda", 0), RULE_SPECS, [ar.SETTINGS[si]], seed=300 + si, shapes=RULE_SHAPES)
    worst = run.assert_within_margin()
    print(f"adam {ar.SETTINGS[si]['name']}: largest error / bound  p' {worst[0]:.3f}  m' {worst[1]:.3f}  v' {worst[2]:.3f}")
    assert run.opt.library_steps == 1 and all(run.guards_intact().values())
    assert all(float(run.opt.state[p]["step"]) == ar.SETTINGS[si]["step"] for p in run.params)


# an aligned tensor of a chunk and one element; 2060 tensors of 1..7 elements at consecutive, mostly unaligned offsets; an aligned tensor
# of two chunks and five; a tensor of a chunk and three that starts one element off a 16-byte boundary.  2067 chunks for a grid of 2048
# workgroups: the chunks of the loop's second trip hold two full vector-path chunks, a ragged tail and an unaligned tensor.
WALK_SPECS = [(4096 + 1, 0)] + [(1 + i % 7, None) for i in range(2060)] + [(2 * 4096 + 5, 0), (4096 + 3, 1)]


@pytest.mark.parametrize("grad_clamp", [None, 1.0])
def test_grid_stride_walk_over_a_large_table(grad_clamp):
    from a3vt_amd import lib
    chunk = int(lib.load().a3vt_adam_chunk_elems())
    assert chunk == 4096 and sum(-(-n // chunk) for n, _ in WALK_SPECS) > 2048 + 4
    setting = dict(ar.SETTINGS[1], grad_clamp=grad_clamp)
    run = _Step(torch.device("cuda", 0), WALK_SPECS, [setting], seed=310)
    assert run.starts[0][0] % 4 == 0 and run.starts[0][-2] % 4 == 0 and run.starts[0][-1] % 4 == 1
    assert sum(s % 4 != 0 for s in run.starts[0][1:2061]) > 1500
    run.assert_within_margin(what=f"clamp {grad_clamp}: ")
    assert run.opt.library_steps == 1
    assert run.guards_intact() == dict.fromkeys(ROLES, True)
    if grad_clamp is None:
        assert np.array_equal(run.raw[1], run.host[1])                         # the gradients are read, never written
    else:
        want = torch.clamp(torch.from_numpy(run.before[1]), -grad_clamp, grad_clamp).numpy()
        assert 0.25 < float((want != run.before[1]).mean()) < 0.4
        assert np.array_equal(run.after[1].view(np.uint32), want.view(np.uint32))


ALIGNED = {}


@pytest.mark.parametrize("mix", range(16), ids=[format(m, "04b") for m in range(16)])
def test_all_sixteen_alignment_mixes(mix):
    """Bit r of ``mix`` starts role r (param, grad, exp_avg, exp_avg_sq) one element off a 16-byte boundary.  Only mix 0 may take the
    vector path; every mix gets the same numbers.  The two paths need not be bit-equal (the compiler may contract them differently):
    both lie within the margin of the fp64 rule, and within the margin of each other."""
    dev = torch.device("cuda", 0)

    def run_mix(m):
        return _Step(dev, [(4096 + 9, 0)], [ar.SETTINGS[2]], seed=320, role_specs=[[(4096 + 9, (m >> r) & 1)] for r in range(4)])
    run = run_mix(mix)
    assert [s[0] % 4 for s in run.starts] == [(mix >> r) & 1 for r in range(4)]
    run.assert_within_margin(what=f"mix {mix:04b}: ")
    assert run.guards_intact() == dict.fromkeys(ROLES, True) and np.array_equal(run.raw[1], run.host[1])
    if "run" not in ALIGNED:
        ALIGNED["run"] = run if mix == 0 else run_mix(0)
    base = ALIGNED["run"]
    assert all(np.array_equal(a, b) for a, b in zip(base.before, run.before))
    _, bnd = run.expected(0, np.ones(4096 + 9, bool))
    for k, name in enumerate(("p", "m", "v")):
        r = 0 if k == 0 else k + 1
        diff = np.abs(run.after[r].astype(np.float64) - base.after[r].astype(np.float64))
        assert (diff <= ar.margin(bnd[k])).all(), (name, float((diff / bnd[k]).max()))


def test_the_clamped_gradient_is_what_the_step_uses():
    """One step from non-zero state, a third of the gradients beyond the clamp.  From zero state Adam's update is lr * sign(g) whatever
    |g| is; from this state m', v' and p' all depend on |g|, so a kernel that wrote the clamped gradient back but stepped with the
    unclamped one is told apart: the result matches the rule on the clamped gradient and, on the clamped share, misses the rule on
    the unclamped one wherever the two rules lie further apart than both margins."""
    setting = ar.SETTINGS[4]
    c = setting["grad_clamp"]
    run = _Step(torch.device("cuda", 0), [(4096 + 9, 0), (777, 1)], [setting], seed=330)
    run.assert_within_margin()
    g = run.before[1]
    over = np.abs(g) > c
    assert 0.28 < float(over.mean()) < 0.38
    assert np.array_equal(run.after[1], np.clip(g, -c, c)) and run.guards_intact() == dict.fromkeys(ROLES, True)
    everything = np.ones(g.size, bool)
    (want_c, bnd_c), (want_u, bnd_u) = run.expected(0, everything), run.expected(0, everything, grad_clamp=None)
    for k, (name, least) in enumerate((("p", 0.10), ("m", 0.25), ("v", 0.25))):
        apart = np.abs(want_c[k] - want_u[k]) > ar.margin(bnd_c[k]) + ar.margin(bnd_u[k])
        assert not apart[~over].any() and float(apart.mean()) >= least, (name, float(apart.mean()))
        err_u = np.abs(run.after[0 if k == 0 else k + 1].astype(np.float64) - want_u[k])
        assert (err_u[apart] > ar.margin(bnd_u[k][apart])).all(), name


NONFINITE = (np.nan, np.inf, -np.inf)
# tensor 0 (aligned, a chunk and five): elements of the vector-path chunk and of its scalar tail; tensor 1 (unaligned): the scalar path
POKED = [(0, i) for i in (0, 1, 2, 2049, 2050, 2051, 4093, 4094, 4095, 4096, 4097, 4098, 4100)] + [(1, i) for i in (0, 1, 2, 297, 298, 299)]


def _poke_nonfinite(run):
    for j, (t, i) in enumerate(POKED):
        run.before[1][run.bounds[t] + i] = NONFINITE[j % 3]


def _torch_cpu_step(run, setting):
    """torch.optim.Adam (single-tensor flavour) on the CPU in fp32 from the same state, the clamp by hand in front of it."""
    p = torch.nn.Parameter(torch.from_numpy(run.before[0].copy()))
    p.grad = torch.from_numpy(run.before[1].copy())
    if setting["grad_clamp"] is not None:
        p.grad.clamp_(-setting["grad_clamp"], setting["grad_clamp"])
    opt = torch.optim.Adam([p], lr=setting["lr"], betas=(setting["beta1"], setting["beta2"]), eps=setting["eps"],
                           weight_decay=setting["weight_decay"], foreach=False)
    opt.state[p] = {"step": torch.tensor(setting["step"] - 1.0), "exp_avg": torch.from_numpy(run.before[2].copy()),
                    "exp_avg_sq": torch.from_numpy(run.before[3].copy())}
    opt.step()
    return [p.detach().numpy(), p.grad.numpy(), opt.state[p]["exp_avg"].numpy(), opt.state[p]["exp_avg_sq"].numpy()]


@pytest.mark.parametrize("grad_clamp", [None, 1.0])
def test_non_finite_gradients(grad_clamp):
    """NaN, +Inf and -Inf gradients as data.  Without the clamp they make p', m' and v' non-finite exactly where torch's Adam does.
    Under the clamp +-Inf become +-c, in the gradient tensor and in the step, and a NaN stays a NaN in the gradient and in p', m' and
    v', as ``torch.clamp`` followed by ``torch.optim.Adam`` leaves them: the kernel must not turn a diverged loss into a step."""
    setting = dict(ar.SETTINGS[1], grad_clamp=grad_clamp)
    run = _Step(torch.device("cuda", 0), [(4096 + 5, 0), (300, 1)], [setting], seed=340, poke=_poke_nonfinite)
    g = run.before[1]
    assert int(np.isnan(g).sum()) == 7 and int(np.isposinf(g).sum()) == 6 and int(np.isneginf(g).sum()) == 6
    ref = _torch_cpu_step(run, setting)
    for r in (0, 2, 3):
        for kind in (np.isnan, np.isposinf, np.isneginf):
            assert np.array_equal(kind(run.after[r]), kind(ref[r])), (ROLES[r], kind.__name__)
    # every element the rule keeps finite, within the margin: under the clamp that includes the +-Inf gradients, which step as +-c
    run.assert_within_margin(ignore=~np.isfinite(g) if grad_clamp is None else np.isnan(g))
    assert run.guards_intact() == dict.fromkeys(ROLES, True) and run.opt.library_steps == 1
    if grad_clamp is None:
        assert np.array_equal(run.raw[1], run.host[1])
        assert all(not np.isfinite(run.after[r][~np.isfinite(g)]).any() for r in (0, 2, 3))
    else:
        nan = np.isnan(g)
        assert all(np.isnan(run.after[r][nan]).all() and np.isfinite(run.after[r][~nan]).all() for r in range(4))
        assert np.array_equal(run.after[1][~nan].view(np.uint32), ref[1][~nan].view(np.uint32))
        assert np.array_equal(run.after[1][np.isposinf(g)], np.full(6, grad_clamp, np.float32))
        assert np.array_equal(run.after[1][np.isneginf(g)], np.full(6, -grad_clamp, np.float32))


def test_param_groups_step_with_their_own_settings():
    specs = [(4096 + 9, 0), (5, None), (4096, 0), (300, 1), (2 * 4096 + 1, 0), (7, None)]
    run = _Step(torch.device("cuda", 0), specs, [ar.SETTINGS[1], ar.SETTINGS[2]], seed=350, group_of=[0, 1, 1, 0, 1, 0])
    run.assert_within_margin()
    assert run.opt.library_steps == 2                    # one launch per group
    assert run.guards_intact() == dict.fromkeys(ROLES, True) and np.array_equal(run.raw[1], run.host[1])
    # the two settings are far enough apart that a group stepped with the other's would not pass
    everything = np.ones(run.before[0].size, bool)
    for gi in (0, 1):
        want, bnd = run.expected(1 - gi, everything)
        sel = run.elem_group == gi
        assert float((np.abs(run.after[0].astype(np.float64) - want[0]) > ar.margin(bnd[0]))[sel].mean()) > 0.5


def test_a_new_gradient_tensor_is_followed_and_the_old_one_left_alone():
    """The chunk table caches device pointers: a gradient that moves to another address must rebuild it."""
    from a3vt_amd import optim as aopt
    dev = torch.device("cuda", 0)
    setting = dict(ar.SETTINGS[1], step=1, zero_state=True)
    sizes = [4096 + 9, 300, 5]
    rng = np.random.default_rng(360)
    params = [torch.nn.Parameter(torch.from_numpy(ar.make_inputs(rng, n, setting)[0]).to(dev)) for n in sizes]
    opt = aopt.Adam(params, lr=setting["lr"], betas=(setting["beta1"], setting["beta2"]), eps=setting["eps"],
                    weight_decay=setting["weight_decay"])
    first = [torch.from_numpy(ar.make_inputs(rng, n, setting)[1]).to(dev) for n in sizes]
    for p, g in zip(params, first):
        p.grad = g
    opt.step()
    before = [[p.detach().cpu().numpy().copy(), None, opt.state[p]["exp_avg"].cpu().numpy().copy(),
               opt.state[p]["exp_avg_sq"].cpu().numpy().copy()] for p in params]
    fresh = torch.from_numpy(ar.make_inputs(rng, sizes[0], setting)[1]).to(dev)
    assert fresh.data_ptr() != first[0].data_ptr()
    params[0].grad = fresh
    first[0].fill_(1e30)                                   # still alive, at the address the cached table holds
    opt.step()
    torch.cuda.synchronize()
    assert opt.library_steps == 2
    assert torch.equal(first[0], torch.full_like(first[0], 1e30)) and torch.equal(params[0].grad, fresh)
    h = dict(ar.hyper(setting), step=2)
    for p, b, g in zip(params, before, [fresh] + first[1:]):
        state = (b[0], g.cpu().numpy(), b[2], b[3])
        want, bnd = ar.step_fp64(*state, **h), ar.bound(*state, **h)
        got = (p.detach().cpu().numpy(), opt.state[p]["exp_avg"].cpu().numpy(), opt.state[p]["exp_avg_sq"].cpu().numpy())
        for k in range(3):
            assert (np.abs(got[k].astype(np.float64) - want[k]) <= ar.margin(bnd[k])).all(), (p.numel(), "pmv"[k])


def test_table_cache_stays_bounded_with_split_step_counts():
    """The late-joiner scenario of test_parameters_without_gradients_and_late_joiners, then 20 more steps: the parameters keep two
    different step counts for good, and the optimizer must hold one set of device tables per partition, not one per step taken."""
    from a3vt_amd import optim as aopt
    dev = torch.device("cuda", 0)
    pa, pb = _params(dev, 7), _params(dev, 7)
    oa = aopt.Adam(pa, lr=3e-4)
    ob = torch.optim.Adam(pb, lr=3e-4, foreach=False)
    sizes = []
    for step in range(24):
        _grads(pa, 50 + step)
        _grads(pb, 50 + step)
        if step < 2:
            for ps in (pa, pb):
                for p in ps[-3:]:
                    p.grad = None
        oa.step()
        ob.step()
        sizes.append(len(oa._tables))
    assert oa.library_steps == 24
    assert float(oa.state[pa[-1]]["step"]) == 22.0 and float(oa.state[pa[0]]["step"]) == 24.0
    assert sizes[23] == sizes[3] and len(set(sizes[3:])) == 1, sizes
    # parity as in the test above.  Per step the two updates differ by a few ulps of an update of at most lr, far below an ulp of a
    # parameter of order 1, so over 24 steps a parameter's rounding flips once at the most: one ulp, 1.2e-7 relative
    for a, b in zip(pa, pb):
        torch.testing.assert_close(a.detach(), b.detach(), rtol=5e-7, atol=1e-8)
