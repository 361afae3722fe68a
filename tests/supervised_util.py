"""What the supervised-policy tests share: a literal fp64 NumPy restatement of the three contracts of ``include/a3vt.h``
(``a3vt_latent_policy_fwd`` with its action choice, ``a3vt_action_value_loss``, ``a3vt_latent_policy_bwd``), the contracts' own
fp32 error bounds, and the recipe of the random networks and inputs the kernel tests run on.

A network is ``(layers, concat_at, transform)``: ``layers`` = [(W (out, in) float32, b (out,) float32, relu), ..]; the input of
layer ``concat_at`` is cat(previous output, latent, first_latent); ``transform`` None or ``(scale, offset)``.

Error bounds (u = 2^-24).  Every sum of the contract is a fixed-order fp32 sum of n products; each of its roundings is relative
to a partial sum no larger than ``S = sum |terms|``.  The worst-case bound ``n u S`` (Higham, Accuracy and Stability, eq. 3.5)
takes all n roundings as aligned and, carried through seven layers of 200 columns, reaches 14 for values whose fp32 error is
1e-5: it bounds nothing.  The bounds here are the probabilistic ones of Higham and Mary (SIAM J. Sci. Comput. 41, 2019, thm. 2.4):
with rounding errors of mean zero ``|computed - exact| <= LAMBDA sqrt(n) u S`` except with probability 2 n exp(-LAMBDA^2 / 2),
2e-5 per sum of 200 terms at LAMBDA = 6 (the bias is one more term, n + 2 covers the butterfly's depth as well); and the errors
``dx`` already in the inputs, independent of each other under the same model, pass through a weight row in quadrature,
``sqrt(sum_i W[o][i]^2 dx[i]^2)``.  ReLU is 1-Lipschitz.  The sigmoid has slope <= 1/4 and is evaluated as ``1 / (1 + expf(-z))``:
expf within 2 ulp, one addition, one division: relative error below 8 u.  ``s * scale - offset`` adds one rounding each.  The
backward bounds follow the same rules through ``W^T`` and the sums over e, with the forward's bound standing in for the error of
the stashed activations.  A ReLU unit whose fp32 pre-activation falls on the other side of zero switches, which no bound on a
smooth function covers.  The worst-case bound, which takes every rounding as aligned, exceeds the distance of the nearest of a
case's ten thousand units to zero in every draw, so ``make_case`` keeps every unit ``RELU_MARGIN`` = 2^-16 = 256 u away from
zero instead: pre-activations are of order one, and the errors the tests measure on them are below 4 u.
"""
import numpy as np

U = 2.0 ** -24
RELU_MARGIN = 2.0 ** -16
TRANSFORMS = {"none": None, "normalize": (2.0, 1.0), "use_img": (6.0, 3.0), "plain": (200.0, 100.0)}


LAMBDA = 6.0


def gamma(n):
    return LAMBDA * np.sqrt(n) * U


def through(d, W):
    """Independent errors ``d`` (E, in) through the rows of ``W`` (out, in): sqrt(sum_i W[o][i]^2 d[e][i]^2)."""
    return np.sqrt((d * d) @ (W * W).T)


def make_net(rng, num_actions, latent_size, layers, hidden_dim, transform):
    """``Latent_Model``'s shapes with torch's default Linear initialisation range (uniform in +-1/sqrt(in))."""
    dims = [(num_actions, 200, True), (200, 100, True), (100, latent_size, False)]
    sizes = [3 * latent_size] + [hidden_dim] * (layers - 1) + [num_actions]
    dims += [(sizes[i], sizes[i + 1], i < layers - 1) for i in range(layers)]
    net = []
    for n_in, n_out, relu in dims:
        k = 1.0 / np.sqrt(n_in)
        net.append((rng.uniform(-k, k, (n_out, n_in)).astype(np.float32), rng.uniform(-k, k, n_out).astype(np.float32), relu))
    return net, 3, transform


def make_inputs(rng, rows, num_actions, latent_size):
    mask = (rng.random((rows, num_actions)) < 0.2).astype(np.float32)
    return mask, rng.standard_normal((rows, latent_size)).astype(np.float32), rng.standard_normal((rows, latent_size)).astype(np.float32)


def forward(net, mask, latent, first_latent):
    """The forward contract in fp64 -> (values (E, A), stash: per layer the post-activation rows (the last: sigmoid(z) under a
    transform), bound: per layer the error bound of that stash entry, value_bound (E, A), relu_gap: the smallest |z| over the ReLU
    units)."""
    layers, concat_at, transform = net
    x = mask.astype(np.float64)
    dx = np.zeros_like(x)
    stash, bounds, gap = [], [], np.inf
    for l, (W, b, relu) in enumerate(layers):
        W, b = W.astype(np.float64), b.astype(np.float64)
        if l == concat_at:
            x = np.concatenate((x, latent.astype(np.float64), first_latent.astype(np.float64)), axis=1)
            dx = np.concatenate((dx, np.zeros((x.shape[0], 2 * latent.shape[1]))), axis=1)
        z = x @ W.T + b                                   # z[e][o] = sum_i W[o][i] x[e][i] + b[o]
        dz = through(dx, W) + gamma(W.shape[1] + 2) * ((np.abs(x) + dx) @ np.abs(W).T + np.abs(b))
        if relu:
            gap = min(gap, float(np.min(np.abs(z))))
            z = np.where(z < 0, 0.0, z)
        x, dx = z, dz
        if l == len(layers) - 1 and transform is not None:
            x = 1.0 / (1.0 + np.exp(-z))
            dx = dz / 4 + 8 * U * x
        stash.append(x)
        bounds.append(dx)
    values, dv = x, dx
    if transform is not None:
        scale, offset = transform
        values = x * scale - offset
        dv = scale * dx + U * np.abs(x * scale) + U * np.abs(values)
    return values, stash, bounds, dv, gap


def choose(values, taken):
    """The action choice, literally: the lowest value among taken == 0; a tie to the lower index; NaN after +inf; -1 when none."""
    out = np.full(values.shape[0], -1, dtype=np.int64)
    for e in range(values.shape[0]):
        best = None
        for a in range(values.shape[1]):
            if taken[e, a] != 0:
                continue
            v = values[e, a]
            key = (1, 0.0) if np.isnan(v) else (0, float(v))
            if best is None or key < best:          # (strict: an equal value leaves the lower index)
                best, out[e] = key, a
    return out


def eligible_gap(values, taken):
    """The smallest relative distance between the two lowest open values of a row (inf with fewer than two)."""
    gap = np.inf
    for e in range(values.shape[0]):
        v = np.sort(values[e][taken[e] == 0])
        if v.size >= 2:
            gap = min(gap, (v[1] - v[0]) / max(abs(v[0]), abs(v[1]), 1e-30))
    return gap


def loss(values, actions, targets):
    """``a3vt_action_value_loss`` in fp64 -> (loss, dvalues)."""
    values = np.asarray(values, dtype=np.float64)
    T, E = actions.shape
    total, dvalues = 0.0, np.zeros_like(values)
    for t in range(T):
        for e in range(E):
            a = int(actions[t, e])
            d = float(targets[t, e]) - values[e, a]
            total += d * d
            dvalues[e, a] += (values[e, a] - float(targets[t, e])) * (2.0 / (T * E))
    return total / (T * E), dvalues


def backward(net, mask, latent, first_latent, dvalues, stash, bounds):
    """``a3vt_latent_policy_bwd`` in fp64 -> per layer (dW, db) and per layer their error bounds (bW, bb)."""
    layers, concat_at, transform = net
    n, E = len(layers), mask.shape[0]
    dvalues = np.asarray(dvalues, dtype=np.float64)
    if transform is not None:
        s = stash[-1]
        delta = dvalues * transform[0] * s * (1.0 - s)
        dd = np.abs(dvalues) * transform[0] * np.abs(1 - 2 * s) * bounds[-1] + 4 * U * np.abs(delta)
    else:
        delta, dd = dvalues.copy(), np.zeros_like(dvalues)
    if layers[-1][2]:
        delta, dd = delta * (stash[-1] > 0), dd * (stash[-1] > 0)
    grads, gbounds = [None] * n, [None] * n
    for l in range(n - 1, -1, -1):
        W = layers[l][0].astype(np.float64)
        if l == 0:
            x, dx = mask.astype(np.float64), np.zeros(mask.shape)
        elif l == concat_at:
            x = np.concatenate((stash[l - 1], latent.astype(np.float64), first_latent.astype(np.float64)), axis=1)
            dx = np.concatenate((bounds[l - 1], np.zeros((E, 2 * latent.shape[1]))), axis=1)
        else:
            x, dx = stash[l - 1], bounds[l - 1]
        dW, db = np.zeros_like(W), np.zeros(W.shape[0])
        for e in range(E):
            dW += np.outer(delta[e], x[e])
            db += delta[e]
        bW = np.sqrt((dd * dd).T @ ((np.abs(x) + dx) ** 2) + (delta * delta).T @ (dx * dx)) + gamma(E + 1) * ((np.abs(delta) + dd).T @ (np.abs(x) + dx))
        bb = np.sqrt((dd * dd).sum(0)) + gamma(E) * (np.abs(delta) + dd).sum(0)
        grads[l], gbounds[l] = (dW, db), (bW, bb)
        if l > 0:
            p = layers[l - 1][0].shape[0]
            back = delta @ W[:, :p]
            dback = through(dd, W[:, :p].T) + gamma(W.shape[0] + 1) * ((np.abs(delta) + dd) @ np.abs(W[:, :p]))
            if layers[l - 1][2]:
                back, dback = back * (stash[l - 1] > 0), dback * (stash[l - 1] > 0)
            delta, dd = back, dback
    return grads, gbounds


def make_case(seed, rows, num_actions, latent_size, layers, hidden_dim, transform, min_choice_gap=None):
    """A network and inputs, re-drawn (seed, seed + 1000, ..) until every ReLU unit is ``RELU_MARGIN`` from zero and, with
    ``min_choice_gap``, the two lowest open values of every row are that far apart (relative).  -> dict."""
    for attempt in range(512):
        rng = np.random.default_rng(seed + 1000 * attempt)
        net = make_net(rng, num_actions, latent_size, layers, hidden_dim, transform)
        mask, latent, first = make_inputs(rng, rows, num_actions, latent_size)
        values, stash, bounds, vbound, gap = forward(net, mask, latent, first)
        if gap < RELU_MARGIN:
            continue
        if min_choice_gap is not None and eligible_gap(values, mask) < min_choice_gap:
            continue
        return dict(net=net, mask=mask, latent=latent, first_latent=first, values=values, stash=stash, bounds=bounds, value_bound=vbound,
                    rng=rng)
    raise AssertionError("no gapped case in 512 draws")


# ---- the recipe of g20_supervised.npz ---------------------------------------------------------------------------------------
# env_util's case "b" models (four fingers, latent 200) with 50 actions, E = 2, budget 2, 700 surface points and a small policy
# (hidden_dim 40, layers 3).  Step 0 trains on two batches (two iterations: the second shows the gradient that is never zeroed),
# step 1 on one batch (model 0 moves first), then one validation batch plays a whole episode.  Everything below is what the
# generator (which drives the REFERENCE engine) and the tests (which drive this package's) must build alike.

FIXTURE = "g20_supervised.npz"
ENV_CASE = "b"
NUM_ACTIONS, BUDGET, HIDDEN_DIM, LAYERS = 50, 2, 40, 3
TRAIN_BATCHES, VALID_BATCHES = 3, 1            # train batches 0, 1 -> step 0; train batch 2 -> step 1
NP_SEED = 2000                                 # np.random.seed(NP_SEED + step) before each train call
MIN_CHOICE_GAP = 1e-2                          # the generator's condition on the two lowest open values of every decision
STORED_WEIGHTS = ("model.2.0.weight", "action_model.0.0.bias", "model.0.0.bias")


BASE_SEED = 2000
COUNTS = {"train": TRAIN_BATCHES, "valid": VALID_BATCHES}


def status_tables():
    """Per batch the (E, NUM_ACTIONS, 4) codes into ``env_util.STATUS``, all three codes present (no idle rule)."""
    import env_util as eu
    return eu.status_tables(BASE_SEED, COUNTS, NUM_ACTIONS, idle_rule=False)


def records(tables):
    """Every batch's sensor records ``{(object id, action): record}``."""
    import env_util as eu
    return eu.batch_records(BASE_SEED, COUNTS, NUM_ACTIONS, tables)


def batches(kind):
    """The ``kind`` ("train" / "valid") loader as a list of batches."""
    import env_util as eu
    return eu.batches(BASE_SEED, kind, COUNTS[kind])


def engine_args(**kw):
    """``env_util.env_args`` of the case with the fixture's sizes plus what the engine and the model read."""
    import env_util as eu
    d = dict(eval=False, num_actions=NUM_ACTIONS, budget=BUDGET, exp_type="g20", exp_id="fixture", pretrained=False, visualize=False,
             use_recon=False, hidden_dim=HIDDEN_DIM, layers=LAYERS, normalize=0, lr=0.001, patience=25, epoch=1, train_steps=2,
             training_actions=5)
    d.update(kw)
    return eu.env_args(ENV_CASE, **d)


def weight_sums(t):
    """What the fixture keeps of a stepped tensor it does not store whole: (sum, sum of |.|, sum of squares) in fp64."""
    t = np.asarray(t, dtype=np.float64)
    return np.array([t.sum(), np.abs(t).sum(), (t * t).sum()])
