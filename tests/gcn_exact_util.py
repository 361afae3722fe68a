"""Exactly summable inputs for the fp32 GCN stack (host only: numpy, torch on the CPU and the fp64 oracle).

Every operand is an integer times a power of two: features, weights and ``grad_update`` in {-1, 0, 1}, biases small integers,
adjacency values 1/2 and 1/4.  Every intermediate of the forward and of the backward is then an integer multiple of a known
quantum ``q = 2^-e`` (an aggregation lowers it by the largest exponent among the adjacency values, 2 here).  A sum whose terms
are multiples of ``q`` with ``sum |terms| <= 2^24 q`` has only fp32 numbers as partial sums, in EVERY order and association,
fused multiply-add or not — so a correct fp32 kernel reproduces the fp64 oracle bit for bit, whatever its tiling, split or
summation order.  ``sum |terms| <= 2^24 q`` is a precondition on the inputs, checked here per sum of the chain
(:func:`assert_exactly_summable`); it is not a tolerance.

Graphs (symmetric pattern, self loops, built from index pairs on a ring of ``n`` vertices; logical index i is vertex
``37 i mod n``, so neighbours are spread over the whole mesh slice):
  "a"  rows of 2 and 4 entries, values 1 / row length.
  "b"  rows of 2, 4, 8 and 16 entries and four hub rows of more than 64; values per EDGE, 1/2 where (row + 2 col) % 3 == 1 and
       1/4 elsewhere: they differ within a row and between A and A^T (a kernel that pairs val[e] with another col[e] shows).
"""
import collections
import functools

import numpy as np
import torch

from oracle import gcn as og

LIMIT = 2.0 ** 24
AGG_SHIFT = 2                      # every aggregation: values >= 2^-2, the quantum drops by that much
# rows and columns of the weight matrices that sit at a tile edge of some kernel: first / last of a 16 tile, the cut (99 | 100),
# the quad-major boundary (159 | 160), the last whole tile and the K tail (287 | 288 .. 299)
EDGE_INDICES = (0, 15, 16, 99, 100, 159, 160, 287, 288, 299)
IN_FEATURES = 50

Case = collections.namedtuple(
    "Case", "name graph n batch layers hidden cut w0_density w_density out_density edge_density gup_density seed backward")


def case(name, graph, n, batch, layers=3, hidden=300, cut=0.33, w0_density=0.2, w_density=0.03, out_density=0.5,
         edge_density=0.3, gup_density=1.0, seed=0, backward=True):
    """Densities of the ternary weights: layer 0, the hidden -> hidden layers, the 3-column output layer (the only way a
    hidden channel of the last layer gets a gradient), and the tile-edge rows and columns of all of them."""
    return Case(name, graph, n, batch, layers, hidden, cut, w0_density, w_density, out_density, edge_density, gup_density, seed,
                backward)


# ---- graphs ------------------------------------------------------------------------------------------------------------

Graph = collections.namedtuple("Graph", "kind n rowptr col val")


def _cycle(members, stride):
    """members[k] -- members[k + stride] around the list: two more entries in each member's row."""
    assert 0 < stride and (2 * stride) % len(members) != 0 and len(members) > 2 * stride
    return members, np.roll(members, -stride)


def hub_leaves(n):
    """Leaves of graph "b" (each linked to three of the four hubs): the hub rows hold 1 + 3/4 of them."""
    return 136 if n >= 1028 else 88


@functools.lru_cache(maxsize=None)
def graph(kind, n):
    assert kind in ("a", "b") and n % 2 == 0 and np.gcd(37, n) == 1
    ids = (np.arange(n, dtype=np.int64) * 37) % n
    pairs = []
    rest = ids
    if kind == "b":
        nl = hub_leaves(n)
        hubs, leaves, rest = ids[:4], ids[4:4 + nl], ids[4 + nl:]
        assert len(rest) % 2 == 0 and nl % 4 == 0
        for h in range(4):                                      # leaf j skips hub j % 4: self + three hubs = 4 entries
            mine = leaves[np.arange(nl) % 4 != h]
            pairs.append((np.full(len(mine), hubs[h]), mine))
    pairs.append((rest[0::2], rest[1::2]))                      # a perfect matching: every row self + partner = 2 entries
    even = rest[0::2]
    pairs.append(_cycle(even, 37))                              # ... the even ones 4
    if kind == "b":
        c8 = even[0::2]
        pairs.append(_cycle(c8, 3))
        pairs.append(_cycle(c8, 7))                             # 8 entries
        c16 = c8[0::2][:16]                                     # (distances 2 .. 8 and 24 .. 30 inside c8: none of the above)
        for t in (1, 2, 3, 4):
            pairs.append(_cycle(c16, t))                        # 16 entries
    a = np.concatenate([p[0] for p in pairs])
    b = np.concatenate([p[1] for p in pairs])
    rows = np.concatenate([ids, a, b])
    cols = np.concatenate([ids, b, a])
    key = np.unique(rows * n + cols)
    assert len(key) == len(rows), "an index pair is listed twice: the row lengths would not be the ones claimed"
    r, c = key // n, key % n
    deg = np.bincount(r, minlength=n)
    rowptr = np.zeros(n + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(deg)
    if kind == "a":
        val = 1.0 / deg[r]
    else:
        val = np.where((r + 2 * c) % 3 == 1, 0.5, 0.25)
    assert val.min() >= 2.0 ** -AGG_SHIFT
    return Graph(kind, n, rowptr, c.astype(np.int32), val.astype(np.float32))


def oracle_adj(g, absolute=False):
    """The CSR triple ``oracle.gcn.adj_matmul`` takes, values float64."""
    val = torch.from_numpy(g.val).double()
    return torch.from_numpy(g.rowptr).long(), torch.from_numpy(g.col).long(), val.abs() if absolute else val


# ---- lattice problems --------------------------------------------------------------------------------------------------

Problem = collections.namedtuple("Problem", "case graph cut_len feats weights biases grad_update")


def ternary_weight(rng, k, h, density, edge_density):
    """(k, h) in {-1, 0, 1}: ``density`` non-zeros everywhere, ``edge_density`` in the tile-edge rows and columns, and at least
    one non-zero in each of those (so a dropped edge row or column always shows)."""
    p = np.full((k, h), float(density))
    er = [i for i in EDGE_INDICES if i < k]
    ec = [j for j in EDGE_INDICES if j < h]
    p[er, :] = np.maximum(p[er, :], edge_density)
    p[:, ec] = np.maximum(p[:, ec], edge_density)
    mask = rng.random((k, h)) < p
    for i in er:
        mask[i, rng.integers(0, h)] = True
    for j in ec:
        mask[rng.integers(0, k), j] = True
    sign = rng.integers(0, 2, (k, h)) * 2 - 1
    return (mask * sign).astype(np.float32)


@functools.lru_cache(maxsize=None)
def problem(c):
    g = graph(c.graph, c.n)
    rng = np.random.default_rng(20261020 + c.seed)
    dims = [IN_FEATURES] + [c.hidden] * (c.layers - 1) + [3]
    feats = rng.integers(-1, 2, (c.batch, c.n, IN_FEATURES)).astype(np.float32)
    weights, biases = [], []
    for i in range(c.layers):
        d = c.w0_density if i == 0 else c.out_density if i == c.layers - 1 else c.w_density
        weights.append(torch.from_numpy(ternary_weight(rng, dims[i], dims[i + 1], d, max(d, c.edge_density)))[None])
        biases.append(torch.from_numpy(rng.integers(-2, 3, dims[i + 1]).astype(np.float32)))
    live = rng.random((c.batch, c.n, 1)) < c.gup_density
    gup = (rng.integers(-1, 2, (c.batch, c.n, 3)) * live).astype(np.float32)
    return Problem(c, g, og.cut_length(c.hidden, c.cut), torch.from_numpy(feats), tuple(weights), tuple(biases),
                   torch.from_numpy(gup))


# ---- the fp64 reference ------------------------------------------------------------------------------------------------

Reference = collections.namedtuple("Reference", "out grad_feats dws dbs")


def oracle_reference(p, adj=None):
    """``oracle.gcn.gcn`` in float64 and its autograd gradients (None without a backward), as float64."""
    c = p.case
    adj = oracle_adj(p.graph) if adj is None else adj
    st = {}
    for i in range(c.layers):
        st[f"g.layers.{i}.weight"] = p.weights[i].double().requires_grad_(c.backward)
        st[f"g.layers.{i}.bias"] = p.biases[i].double().requires_grad_(c.backward)
    f = p.feats.double().requires_grad_(c.backward)
    out = og.gcn(f, st, "g", adj, c.layers, c.cut)
    if not c.backward:
        return Reference(out.detach(), None, None, None)
    (out * p.grad_update.double()).sum().backward()
    return Reference(out.detach(), f.grad, tuple(st[f"g.layers.{i}.weight"].grad for i in range(c.layers)),
                     tuple(st[f"g.layers.{i}.bias"].grad for i in range(c.layers)))


@functools.lru_cache(maxsize=None)
def reference(c):
    """The reference of a case cast to fp32 (exact: every value is an fp32 number under the precondition).  Shared by the
    tests; never modified."""
    r = oracle_reference(problem(c))
    f32 = lambda t: None if t is None else t.float()  # noqa: E731
    return Reference(f32(r.out), f32(r.grad_feats), None if r.dws is None else tuple(f32(t) for t in r.dws),
                     None if r.dbs is None else tuple(f32(t) for t in r.dbs))


# ---- the precondition --------------------------------------------------------------------------------------------------

Sums = collections.namedtuple("Sums", "shares worst worst_name dz_quanta zero_fraction acts dzs")


def _on_lattice(t, e, what):
    s = t * 2.0 ** e
    assert torch.equal(s, s.round()), f"{what}: not a multiple of 2^-{e}"


def exact_sums(p):
    """Every sum of the forward and backward chain in float64, with the operands' absolute values: ``shares[name]`` =
    max over the outputs of sum |terms|, as a share of 2^24 quanta of that sum.  Also: the largest |dZ| of each hidden layer in
    quanta (the fp32x3 dW condition), the fraction of hidden pre-activations that are exactly zero, and the layer inputs and
    dZ tensors (float64) for the order-independence tests."""
    c, cl = p.case, p.cut_len
    A, absA = oracle_adj(p.graph), oracle_adj(p.graph, absolute=True)
    ws = [w[0].double() for w in p.weights]
    bs = [b.double() for b in p.biases]
    shares = {}

    def put(name, bound, e):
        shares[name] = bound.max().item() * 2.0 ** e / LIMIT

    # forward
    x, e = p.feats.double(), 0
    acts, exps, zeros, count = [x], [0], 0, 0
    for i in range(c.layers - 1):
        s = x.abs() @ ws[i].abs()
        put(f"X{i}W{i}", s, e)
        z = x @ ws[i]
        if cl:
            put(f"A(X{i}W{i})+b", og.adj_matmul(absA, s[..., :cl]) + bs[i][:cl].abs(), e + AGG_SHIFT)
            y = torch.cat((og.adj_matmul(A, z[..., :cl]) + bs[i][:cl], z[..., cl:]), dim=-1)
            e += AGG_SHIFT
        else:
            y = z
        _on_lattice(y, e, f"pre-activation {i}")
        zeros, count = zeros + int((y == 0).sum()), count + y.numel()
        x = torch.relu(y)
        acts.append(x)
        exps.append(e)
    last = c.layers - 1
    s = x.abs() @ ws[last].abs()
    put(f"X{last}W{last}", s, e)
    put(f"A(X{last}W{last})+b", og.adj_matmul(absA, s) + bs[last].abs(), e + AGG_SHIFT)
    if not c.backward:
        return _sums(shares, {}, zeros / max(count, 1), acts, [])

    # backward
    g, eg = p.grad_update.double(), 0
    put(f"db{last}", g.abs().sum((0, 1)), eg)
    put("A^T dU", og.adj_t_matmul(absA, g.abs()), eg + AGG_SHIFT)
    dz, ez = og.adj_t_matmul(A, g), eg + AGG_SHIFT
    dzs, dzq = {last: dz}, {}
    for i in range(last, -1, -1):
        x = acts[i]
        if i < last:
            if cl:
                put(f"db{i}", g[..., :cl].abs().sum((0, 1)), eg)
                put(f"A^T G{i}", og.adj_t_matmul(absA, g[..., :cl].abs()), eg + AGG_SHIFT)
                dz = torch.cat((og.adj_t_matmul(A, g[..., :cl]), g[..., cl:]), dim=-1)
                ez = eg + AGG_SHIFT
            else:
                dz, ez = g, eg
            dzs[i] = dz
            dzq[i] = dz.abs().max().item() * 2.0 ** ez
        _on_lattice(dz, ez, f"dZ{i}")
        put(f"dW{i}", torch.einsum("bnk,bnj->kj", x.abs(), dz.abs()), exps[i] + ez)
        put(f"dZ{i}W{i}^T", dz.abs() @ ws[i].abs().t(), ez)
        dx = dz @ ws[i].t()
        g, eg = (x > 0).double() * dx, ez
    return _sums(shares, dzq, zeros / max(count, 1), acts, [dzs[i] for i in range(c.layers)])


def _sums(shares, dzq, zero_fraction, acts, dzs):
    name = max(shares, key=shares.get)
    return Sums(shares, shares[name], name, dzq, zero_fraction, acts, dzs)


@functools.lru_cache(maxsize=None)
def case_sums(c):
    s = exact_sums(problem(c))
    return s._replace(acts=None, dzs=None)          # the cache keeps the figures, not the tensors


def assert_exactly_summable(p, sums=None):
    """The precondition, per sum: raises when a sum of the chain can leave the fp32 lattice (an error of the test's author,
    never a reason to skip).  Returns the worst share of 2^24."""
    sums = exact_sums(p) if sums is None else sums
    over = {k: round(v, 3) for k, v in sums.shares.items() if v > 1.0}
    assert not over, f"{p.case.name}: not exactly summable in fp32, sum |terms| / (2^24 q) = {over}"
    return sums.worst


# ---- the cases of tests/test_gpu_gcn_exact.py (the host module proves the precondition for each) -------------------------------

STACK_CASES = {c.name: c for c in (
    case("whole_tiles", "a", 1028, 12),                                     # 12 336 rows = 771 tiles of 16
    case("ragged_rows", "a", 1028, 13, seed=1),                             # 13 364 rows = 835 tiles + 4 rows
    case("six_per_thread", "a", 2564, 5, seed=2),                           # n > 4 * 512: six vertices per thread; 12 820 rows
    # four layers: each further layer costs dW of the output layer a factor; sparser weights and grad_update keep it below 2^24,
    # and |dZ| of both hidden -> hidden layers within 255 quanta (the fp32x3 dW condition)
    case("four_layers", "a", 1028, 12, layers=4, w_density=0.02, out_density=0.02, edge_density=0.1, gup_density=0.25,
         seed=3),
    case("hub_rows", "b", 1028, 12, edge_density=0.15, seed=4),             # rows <= 8, 9 .. 64 and > 64
    case("cut_004", "a", 1028, 12, cut=0.04, seed=5),                       # cut_len 12
    case("cut_05", "a", 1028, 12, cut=0.5, seed=6),                         # cut_len 150
    case("small_h300", "b", 260, 3, seed=7),                                # 780 rows: below the hybrid threshold
    case("small_h32", "b", 260, 3, hidden=32, w_density=0.25, seed=8),
    # the forward alone has far more room: every weight +-1
    case("forward_dense", "a", 1028, 12, w0_density=1.0, w_density=1.0, out_density=1.0, seed=9, backward=False),
)}


# ---- one layer on its own (ops.gcn_layer) ------------------------------------------------------------------------------------

LayerCase = collections.namedtuple("LayerCase", "name n batch kin nout cut relu density seed")   # cut None: no cut
LAYER_CASES = {c.name: c for c in (
    LayerCase("hidden", 260, 3, 300, 300, 0.33, True, 0.03, 20),
    LayerCase("odd_sizes", 260, 3, 37, 30, 0.5, False, 0.5, 21),
    LayerCase("thin_output", 260, 3, 300, 3, None, False, 0.3, 22),
)}
LayerProblem = collections.namedtuple("LayerProblem", "case graph cut_len x weight bias grad_y")


@functools.lru_cache(maxsize=None)
def layer_problem(c):
    rng = np.random.default_rng(20261020 + c.seed)
    x = rng.integers(-1, 2, (c.batch, c.n, c.kin)).astype(np.float32)
    w = ternary_weight(rng, c.kin, c.nout, c.density, max(c.density, 0.3))
    b = rng.integers(-2, 3, c.nout).astype(np.float32)
    gy = rng.integers(-1, 2, (c.batch, c.n, c.nout)).astype(np.float32)
    cl = c.nout if c.cut is None else og.cut_length(c.nout, c.cut)
    return LayerProblem(c, graph("b", c.n), cl, torch.from_numpy(x), torch.from_numpy(w)[None], torch.from_numpy(b),
                        torch.from_numpy(gy))


@functools.lru_cache(maxsize=None)
def layer_reference(c):
    """(y, grad_x, grad_weight, grad_bias) of ``oracle.gcn.gcn_layer`` in float64, cast to fp32."""
    p = layer_problem(c)
    x, w, b = (t.double().requires_grad_(True) for t in (p.x, p.weight, p.bias))
    y = og.gcn_layer(x, w, b, oracle_adj(p.graph), c.cut if c.cut is not None else 0.0, c.cut is not None, c.relu)
    (y * p.grad_y.double()).sum().backward()
    return y.detach().float(), x.grad.float(), w.grad.float(), b.grad.float()


def layer_sums(p):
    """The sums of one layer, forward and backward, as :func:`exact_sums` states them.  Returns {name: share of 2^24}."""
    c, cl = p.case, p.cut_len
    A, absA = oracle_adj(p.graph), oracle_adj(p.graph, absolute=True)
    x, w, b, gy = p.x.double(), p.weight[0].double(), p.bias.double(), p.grad_y.double()
    s = x.abs() @ w.abs()
    z = x @ w
    y = torch.cat((og.adj_matmul(A, z[..., :cl]) + b[:cl], z[..., cl:]), dim=-1)
    g = gy * (y > 0).double() if c.relu else gy
    dz = torch.cat((og.adj_t_matmul(A, g[..., :cl]), g[..., cl:]), dim=-1)
    _on_lattice(y, AGG_SHIFT, "pre-activation")
    _on_lattice(dz, AGG_SHIFT, "dZ")
    q = 2.0 ** AGG_SHIFT
    return {"XW": s.max().item() / LIMIT,
            "A(XW)+b": (og.adj_matmul(absA, s[..., :cl]) + b[:cl].abs()).max().item() * q / LIMIT,
            "db": g[..., :cl].abs().sum((0, 1)).max().item() / LIMIT,
            "A^T G": og.adj_t_matmul(absA, g[..., :cl].abs()).max().item() * q / LIMIT,
            "dW": torch.einsum("bnk,bnj->kj", x.abs(), dz.abs()).max().item() * q / LIMIT,
            "dZ W^T": (dz.abs() @ w.abs().t()).max().item() * q / LIMIT}
