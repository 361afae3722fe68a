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
Graph "s" / "sc" is built by PHYSICAL vertex index instead: ``diag(s) (P + J)`` for the P + bipartite split kernels, P with
rows of 1 .. 12 entries, J the complete block S x C, values 1/2 and 1/4 per ROW (:func:`_split_build`).
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
    "Case", "name graph n batch layers hidden cut w0_density w_density out_density edge_density gup_density seed backward "
            "feat_density")


def case(name, graph, n, batch, layers=3, hidden=300, cut=0.33, w0_density=0.2, w_density=0.03, out_density=0.5,
         edge_density=0.3, gup_density=1.0, seed=0, backward=True, feat_density=1.0):
    """Densities of the ternary weights: layer 0, the hidden -> hidden layers, the 3-column output layer (the only way a
    hidden channel of the last layer gets a gradient), and the tile-edge rows and columns of all of them.  ``feat_density``
    below 1 thins the ternary features as well (the class sums of a large split graph)."""
    return Case(name, graph, n, batch, layers, hidden, cut, w0_density, w_density, out_density, edge_density, gup_density, seed,
                backward, feat_density)


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
    if kind in SPLIT_KINDS:
        return _split_build(kind, n)[0]
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


# ---- the split graph: diag(s) (P + J), by PHYSICAL vertex index -------------------------------------------------------

SPLIT_KINDS = ("s", "sc")           # vertex n-1 in S / in C
QS_THREADS = 512                    # the workgroup of csrqs_kernel: vertex v is held by thread v % 512 as its slot v // 512
SplitArrays = collections.namedtuple("SplitArrays", "p_rowptr p_col scale cls")


def split_centres(n):
    """Four centres with v % 4 == 2 (so never in S = {v % 4 == 1}): in different per-thread slots ``v // 512`` as far as the mesh
    has four, and in different waves ``(v % 512) >> 6`` as far as their slots have them."""
    slots = -(-n // QS_THREADS)
    out = []
    for j in range(4):
        k0 = j * (slots - 1) // 3 if slots >= 4 else j % slots
        for dk in range(slots):
            lo = (k0 + dk) % slots * QS_THREADS
            hi = min(n, lo + QS_THREADS)
            waves = -(-(hi - lo) // 64)
            cand = [u for u in range(lo + 2, hi, 4) if u not in out]
            pick = [u for u in cand if (u - lo) >> 6 == (j + 1) % waves] or cand
            if pick:
                out.append(pick[0])
                break
    assert len(out) == 4
    return out


@functools.lru_cache(maxsize=None)
def _split_build(kind, n):
    """``(Graph, SplitArrays)`` of graph "s" / "sc".  Not row-normalised, on purpose: the split kernels take ``scale`` as data.

    P (symmetric 0/1, a self loop everywhere): vertices 0 .. 63 keep the self loop alone (one wave of csrqs_kernel walks one
    slot pair while the others walk up to six).  The rest, i = v - 64: four vertices in two pairs (2 entries); a ring over the
    others (3); rings with stride 3 over the multiples of 2, 4, 8 and 16 (+ 2 each: 5, 7, 9, 11); and the multiples of 3 matched
    in pairs (+ 1: every even length up to 12).  S = {v % 4 == 1}, C = four centres (:func:`split_centres`); vertex n-1 joins
    S (kind "s") or takes the place of the centre of its own slot ("sc").  An S-C pair of the rule above is left out of P: it is in J."""
    assert kind in SPLIT_KINDS and n % 4 == 0 and n >= 96
    v = np.arange(n, dtype=np.int64)
    cls = np.where(v % 4 == 1, 1, 0).astype(np.uint8)
    centres = split_centres(n)
    if kind == "sc":                                                           # in place of the centre of its own slot
        centres[[u // QS_THREADS for u in centres].index((n - 1) // QS_THREADS)] = n - 1
    else:
        cls[n - 1] = 1
    cls[centres] = 2
    i = np.arange(n - 64, dtype=np.int64)
    lone = np.array([1, 5, 7, 11])
    pairs = [(lone[0::2], lone[1::2]), _cycle(np.setdiff1d(i, lone), 1)]
    for t in (1, 2, 3, 4):
        members = i[i % (1 << t) == 0]
        if len(members) > 6:
            pairs.append(_cycle(members, 3))
    third = i[i % 3 == 0]
    third = third[:len(third) // 2 * 2]
    pairs.append((third[0::2], third[1::2]))
    a = np.concatenate([p[0] for p in pairs]) + 64
    b = np.concatenate([p[1] for p in pairs]) + 64
    rows, cols = np.concatenate([v, a, b]), np.concatenate([v, b, a])
    pkey = np.unique(rows * n + cols)
    assert len(pkey) == len(rows), "an index pair is listed twice: the row lengths would not be the ones claimed"
    pkey = pkey[cls[pkey // n].astype(int) * cls[pkey % n] != 2]               # classes 1 x 2: the bipartite block's
    s_idx, c_idx = np.flatnonzero(cls == 1), np.flatnonzero(cls == 2)
    sc = (s_idx[:, None] * n + c_idx[None, :]).ravel()
    cs = (c_idx[:, None] * n + s_idx[None, :]).ravel()
    key = np.unique(np.concatenate([pkey, sc, cs]))
    assert len(key) == len(pkey) + 2 * len(sc)
    scale = np.where(v % 3 == 1, 0.5, 0.25).astype(np.float32)
    assert scale.min() >= 2.0 ** -AGG_SHIFT

    def csr(k):
        rowptr = np.zeros(n + 1, dtype=np.int32)
        rowptr[1:] = np.cumsum(np.bincount(k // n, minlength=n))
        return rowptr, (k % n).astype(np.int32)
    rowptr, col = csr(key)
    p_rowptr, p_col = csr(pkey)
    return Graph(kind, n, rowptr, col, scale[key // n]), SplitArrays(p_rowptr, p_col, scale, cls)


def split_arrays(g):
    """``(p_rowptr, p_col, scale, cls)`` of a split graph: what ``a3vt_adj_split`` carries next to the full CSR."""
    return _split_build(g.kind, g.n)[1]


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


def _keep_class_sums_alive(rng, cut_len, cls, feats, weights, biases):
    """The split graph only: sigma_C has four terms, and without care it is exactly zero in all four channels of some
    (mesh, quad), or equal to sigma_S there — a kernel that dropped or swapped the bipartite term in that quad would not
    show.  tests/test_gcn_exact_host.py asserts that this never happens; these arrangements of the inputs (and, for what they
    leave to chance, the choice of the seeds) make it so.

    1. Layer 0 forward.  Per mesh and input channel the features of S sum to an odd number and those of C to 2 or -2; the even
       aggregated columns of W_0 hold an odd number of non-zeros.  sigma_S is then odd and sigma_C = 2 (mod 4).
    2. All centres receive the same sigma_S, which outweighs their few P terms, so a channel is dead behind the ReLU at every
       centre at once (and from layer 1 on the same holds for S and sigma_C).  The aggregated channels of a hidden layer
       therefore come in pairs (2m, 2m + 1) with opposite weight columns and biases >= 1: the pre-activations are ``t + b``
       and ``-t + b'`` (the aggregation is linear and exact), one of them is positive at EVERY vertex, and both halves of a
       quad keep a live channel for the backward.
    3. The gradient of such a channel is dZ . (its row of the next layer's weights).  With the ReLU pattern shared by a whole
       class, the backward class sum of channel k is (row k) . D, D = the class sum of dZ.  Hidden next layer: dZ is dense in
       the aggregated channels only, so every such row gets two non-zeros there.  Output layer (D has three entries): the rows
       of a quad are +-e0, +-e1, +-e2 and +-e0 +- e1, so the live channels of its two halves never rest on the same entry."""
    cl, last = cut_len, len(weights) - 1
    even = torch.arange(0, cl - 1, 2)
    sign = lambda size: torch.from_numpy(rng.integers(0, 2, size) * 2.0 - 1.0).float()  # noqa: E731
    for i in range(1, last):
        w = weights[i][0]
        for k in range(cl):
            short = 2 - int((w[k, even] != 0).sum())
            if short > 0:
                free = even[w[k, even] == 0]
                w[k, free[torch.from_numpy(rng.permutation(len(free))[:short])]] = sign(short)
    out = weights[last][0]
    out[:cl] = 0
    k = torch.arange(cl)
    out[k, torch.where(k % 4 == 3, 0, k % 4)] = sign(cl)
    k3 = k[k % 4 == 3]
    out[k3, 1] = sign(len(k3))
    w0 = weights[0][0]
    for k in even.tolist():
        if int((w0[:, k] != 0).sum()) % 2 == 0:
            w0[int(torch.nonzero(w0[:, k] == 0)[0]), k] = 1.0
    for i in range(last):
        w = weights[i][0]
        w[:, even + 1] = -w[:, even]
        biases[i][:2 * len(even)] = torch.from_numpy(rng.integers(1, 3, 2 * len(even)).astype(np.float32))
    seam, centres = np.flatnonzero(cls == 1), np.flatnonzero(cls == 2)
    tot, own = feats[:, seam, :].sum(1), feats[:, seam[-1], :]
    feats[:, seam[-1], :] = np.where(tot % 2 == 0, np.where(own == 0, 1.0, 0.0), own)
    x2 = feats[:, centres[2], :]
    u = feats[:, centres[0], :] + feats[:, centres[1], :] + x2
    feats[:, centres[2], :] = x2 = np.where(u == 0, np.where(x2 == 0, 1.0, 0.0), x2)
    u = feats[:, centres[0], :] + feats[:, centres[1], :] + x2                 # 1 .. 3 in magnitude: the fourth makes it 2
    feats[:, centres[3], :] = np.where(np.abs(u) == 1, u, np.where(np.abs(u) == 2, 0.0, -np.sign(u)))


@functools.lru_cache(maxsize=None)
def problem(c):
    g = graph(c.graph, c.n)
    rng = np.random.default_rng(20261020 + c.seed)
    dims = [IN_FEATURES] + [c.hidden] * (c.layers - 1) + [3]
    feats = rng.integers(-1, 2, (c.batch, c.n, IN_FEATURES)).astype(np.float32)
    if c.feat_density < 1.0:                                # (a stream of its own: the other draws stay what they were)
        feats *= np.random.default_rng(977 + c.seed).random(feats.shape) < c.feat_density
    weights, biases = [], []
    for i in range(c.layers):
        d = c.w0_density if i == 0 else c.out_density if i == c.layers - 1 else c.w_density
        weights.append(torch.from_numpy(ternary_weight(rng, dims[i], dims[i + 1], d, max(d, c.edge_density)))[None])
        biases.append(torch.from_numpy(rng.integers(-2, 3, dims[i + 1]).astype(np.float32)))
    if c.graph in SPLIT_KINDS:
        _keep_class_sums_alive(rng, og.cut_length(c.hidden, c.cut), split_arrays(g).cls, feats, weights, biases)
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


# the split graph (csrqs_kernel, csrqs_image_kernel, csr3s_kernel).  Class sums of ~n/4 terms and dW over batch * n rows: the
# densities and seeds are chosen per case so that the host module proves the precondition and the discrimination of the class sums.
# The un-normalised class sums feed on each other (sigma_S makes the centres large, sigma_C hands that to every vertex of S,
# which the next sigma_S adds up coherently): the larger the mesh, the thinner the inputs
_THIN = dict(w0_density=0.1, w_density=0.02, out_density=0.15, edge_density=0.08, gup_density=0.25)
_THINNER = dict(w0_density=0.05, w_density=0.01, out_density=0.1, edge_density=0.03, gup_density=0.1, feat_density=0.5)
SPLIT_CASES = {c.name: c for c in (
    case("split_last_in_s", "s", 1028, 12, seed=10, **_THIN),               # four vertices per thread, the third slot holds four
    case("split_last_in_c", "sc", 1028, 12, seed=31, **_THIN),
    case("split_uneven_parts", "s", 516, 24, seed=42, **_THIN),             # 10 parts over 25 quads
    case("split_small_mesh", "sc", 96, 136, edge_density=0.15, seed=13),    # one part: 25 quads in one loop
    case("split_six_per_thread", "sc", 2564, 5, seed=34, **_THINNER),
    case("split_cut_12", "s", 1028, 12, cut=0.04, seed=15, **_THIN),
    case("split_cut_128", "s", 1028, 12, cut=0.4267, seed=16, **_THIN),
    case("split_cut_132", "s", 1028, 12, cut=0.44, seed=17, **_THIN),       # wider than the split kernels take
    case("split_forward_only", "s", 1028, 12, seed=18, backward=False),     # ordinary densities
    case("split_below_threshold", "s", 260, 3, seed=19),                    # 780 rows
    case("split_past_lds", "s", 3844, 1, seed=20, **_THINNER),              # 3844 * 16 bytes > 60 KB
)}


def split_forward32(p, drop_member=None, twice=None, swap=False, drop_last_of=None, scale_tail=False, last_again=False):
    """The stack forward in fp32 on the CPU in the split's own association: per aggregated channel the sum over the row of P,
    plus the class sum (sigma_C for a vertex of S, sigma_S for a centre), then times ``scale``.  The keyword arguments are the
    mutations of tests/test_gcn_exact_host.py: a member of S left out of sigma_S, a centre counted twice in sigma_C, the two
    sums swapped, the last P entry of one row dropped, the pass-through channels of the last quad scaled, the last vertex added
    once more to its class sum."""
    g, sp = p.graph, split_arrays(p.graph)
    n = g.n
    prow = torch.from_numpy(np.repeat(np.arange(n), np.diff(sp.p_rowptr))).long()
    pcol = torch.from_numpy(sp.p_col).long()
    if drop_last_of is not None:
        keep = torch.arange(len(pcol)) != int(sp.p_rowptr[drop_last_of + 1]) - 1
        prow, pcol = prow[keep], pcol[keep]
    scale = torch.from_numpy(sp.scale)[:, None]
    cls = torch.from_numpy(sp.cls.astype(np.int64))
    in_s, in_c = (cls == 1).float()[:, None], (cls == 2).float()[:, None]
    ws, wc = in_s.clone(), in_c.clone()                     # the weight of each vertex in sigma_S and in sigma_C
    if drop_member is not None:
        ws[drop_member] = 0
    if twice is not None:
        wc[twice] = 2
    if last_again:
        (ws if cls[n - 1] == 1 else wc)[n - 1] += 1

    def aggregate(z):
        acc = torch.zeros_like(z).index_add_(1, prow, z[:, pcol])
        sig_s, sig_c = (z * ws).sum(1, keepdim=True), (z * wc).sum(1, keepdim=True)
        if swap:
            sig_s, sig_c = sig_c, sig_s
        return scale * (acc + in_s * sig_c + in_c * sig_s)

    x = p.feats.clone()
    for i in range(p.case.layers):
        last = i == p.case.layers - 1
        w, b = p.weights[i][0], p.biases[i]
        cl = w.shape[1] if last else p.cut_len
        z = x @ w
        rest = z[..., cl:].clone()
        if scale_tail and not last:
            rest[..., :(-cl) % 4] *= scale                  # the channels that share the last aggregated quad
        y = torch.cat((aggregate(z[..., :cl]) + b[:cl], rest), dim=-1)
        x = y if last else torch.relu(y)
    return x


def split_class_sums(p, sums):
    """sigma_S and sigma_C (float64) of every aggregation that csrqs_kernel runs for a stack: the hidden layers' forward inputs
    (raw products, channels < cut_len; the pass-through channels of the last quad count as zero here) and their backward
    inputs (the masked gradients times ``scale``).  A list of ``(name, sigma_S, sigma_C)``, each (batch, quads, 4)."""
    sp, c, cl = split_arrays(p.graph), p.case, p.cut_len
    cpad = (cl + 3) // 4 * 4
    in_s = torch.from_numpy(sp.cls == 1).double()[:, None]
    in_c = torch.from_numpy(sp.cls == 2).double()[:, None]
    scale = torch.from_numpy(sp.scale).double()[:, None]
    out = []
    for i in range(c.layers - 1):
        z = torch.nn.functional.pad((sums.acts[i] @ p.weights[i][0].double())[..., :cl], (0, cpad - cl))
        out.append((f"forward {i}", (z * in_s).sum(1).reshape(c.batch, -1, 4), (z * in_c).sum(1).reshape(c.batch, -1, 4)))
        if c.backward:
            # dZ_{i+1} W^T masked by the ReLU = the gradient at this layer's output; csrqs_kernel<1> scales the aggregated
            # channels on their way into LDS
            gr = (sums.dzs[i + 1] @ p.weights[i + 1][0].double().t()) * (sums.acts[i + 1] > 0)
            gr = torch.nn.functional.pad(gr[..., :cl] * scale, (0, cpad - cl))
            out.append((f"backward {i}", (gr * in_s).sum(1).reshape(c.batch, -1, 4),
                        (gr * in_c).sum(1).reshape(c.batch, -1, 4)))
    return out


# ---- one layer on its own (ops.gcn_layer) -----------------------------------------------------------------------------------

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
