"""Helpers shared by the nearest-neighbour policy's tests and ``golden/make_golden_nn.py``: a literal NumPy restatement of the
contract of ``a3vt_latent_nearest`` (``include/a3vt.h``) in fp64, the gapped banks the kernel tests run on, a literal
restatement of the reference's per-element walk (``policies/NearestNeighbor/train.py:114-137``), and the recipe of the fixture
``g19_nearest_neighbor.npz`` — what the generator (which drives the REFERENCE engine) and the tests (which drive this
package's) must build alike."""
import numpy as np

import env_util as eu

FIXTURE = "g19_nearest_neighbor.npz"
CASE = "b"                 # env_util's case: four fingers, latent, E = 2, 6 actions, budget 3, greedy_checks 3
TRAIN_BATCHES = 3          # int(3 * 0.4) = 1 of them is swept
VALID_BATCHES = 2
BANK_ROWS = 40             # the validate case's bank
BANK_SEED = 1902
MIN_GAP = 1e-2             # the generator's condition on consecutive fp64 distances among the k + 1 nearest


def distances64(bank, query):
    """fp64 mean squared difference of one query to every row (of the fp32 values as they are)."""
    return ((np.asarray(bank, dtype=np.float64) - np.asarray(query, dtype=np.float64)[None]) ** 2).mean(axis=1)


def contract(bank, bank_actions, queries, taken, k):
    """``a3vt_latent_nearest`` word for word, in fp64: (idx (E, k) int32, dist (E, k) float64, action (E,), rank (E,))."""
    M, E = len(bank), len(queries)
    k_eff = min(k, M)
    idx, dist = np.full((E, k), -1, dtype=np.int32), np.full((E, k), np.inf)
    action, rank = np.full(E, -1, dtype=np.int32), np.full(E, -1, dtype=np.int32)
    for e in range(E):
        d = distances64(bank, queries[e])
        order = np.argsort(d, kind="stable")[:k_eff]          # ties to the lower row; NaN after every number
        idx[e, :k_eff], dist[e, :k_eff] = order, d[order]
        if bank_actions is None:
            continue
        for p, j in enumerate(order):
            a = int(bank_actions[j])
            num_actions = taken.shape[1] if taken is not None else 304
            if 0 <= a < num_actions and (taken is None or taken[e, a] == 0):
                action[e], rank[e] = a, p
                break
    return idx, dist, action, rank


def smallest_gap(dist_row, upto):
    """Smallest relative gap between consecutive entries of a sorted row of distances, over its first ``upto`` entries."""
    d = np.asarray(dist_row, dtype=np.float64)[:upto]
    d = d[np.isfinite(d)]
    if len(d) < 2:
        return np.inf
    return float(((d[1:] - d[:-1]) / np.maximum(d[1:], 1e-300)).min())


def gapped_bank(bank_rows, dim, n_queries, near, seed):
    """``(bank (M, D) float32, queries (E, D) float32)``: per query ``min(near, M // E)`` rows ``q + r_j u_j`` with unit
    directions ``u_j`` and radii ``r_j = 0.05 * 1.02^j`` (consecutive distances 4 % apart), the rest standard-normal rows, the
    whole bank shuffled."""
    g = np.random.default_rng(seed)
    queries = g.standard_normal((n_queries, dim)).astype(np.float32)
    n_near = min(near, bank_rows // n_queries)
    rows = []
    for e in range(n_queries):
        u = g.standard_normal((n_near, dim))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        r = 0.05 * 1.02 ** np.arange(n_near)
        rows.append(queries[e].astype(np.float64)[None] + r[:, None] * u)
    rows.append(g.standard_normal((bank_rows - n_near * n_queries, dim)) * 1.0 + 4.0 * np.sign(g.standard_normal((1, dim))))
    bank = np.concatenate(rows).astype(np.float32)
    return np.ascontiguousarray(bank[g.permutation(bank_rows)]), queries


def reference_walk(latents, actions, query, seen_actions, k):
    """Reference lines 114-137 for one element, on NumPy in fp64: the k smallest mean squared differences in order, then the
    first of them whose action is not among ``seen_actions``.  Returns the action, or None when the walk finds none (the
    reference then builds a short action array)."""
    d = distances64(latents, query)
    for j in np.argsort(d, kind="stable")[:k]:
        if len(seen_actions) == 0 or actions[j] not in seen_actions:
            return int(actions[j])
    return None


# ---- the recipe of g19_nearest_neighbor.npz -------------------------------------------------------------------------------
# env_util's case "b" (models, settings, surface draws); every batch has its own two objects, sensor records and clouds, so the
# batches differ in what the policy observes.

BASE_SEED = 1900
COUNTS = {"train": TRAIN_BATCHES, "valid": VALID_BATCHES}


def records():
    """Every batch's sensor records in one mapping ``{(object id, action): record}``, tables under the idle rule."""
    n = eu.CASES[CASE]["num_actions"]
    return eu.batch_records(BASE_SEED, COUNTS, n, eu.status_tables(BASE_SEED, COUNTS, n))


def batches(kind):
    """The ``kind`` ("train" / "valid") loader as a list of batches."""
    return eu.batches(BASE_SEED, kind, COUNTS[kind])


def engine_args(evaluate, **kw):
    """``env_util.env_args`` of the case plus what the engine reads."""
    c = eu.CASES[CASE]
    return eu.env_args(CASE, eval=evaluate, greedy_checks=c["greedy_checks"], exp_type="g19", pretrained=False, visualize=False,
                       use_recon=False, **kw)


NEAR = 0.02                # how far the bank's three placed entries lie from the latents they are placed at


def validate_bank(first_latent):
    """The first 38 entries of the ``validate`` case's bank.  37 lie around the latent every episode starts from (a mesh without
    touches): ``first_latent + r_j u_j`` with seeded unit directions and radii ``|first_latent| * 1.1^j`` — consecutive distances
    21 % apart, the nearest four times as far as an episode's latents move — with seeded actions, shuffled.  The 38th lies
    ``NEAR`` from ``first_latent`` and carries action 0: it decides every episode's first step.
    Returns (latents (38, D) float32, actions (38,) int64)."""
    g = np.random.default_rng(BANK_SEED)
    n = BANK_ROWS - 3
    first = np.asarray(first_latent, dtype=np.float64)
    u = g.standard_normal((n + 1, first.shape[0]))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = np.linalg.norm(first) * 1.1 ** np.arange(n)
    order = g.permutation(n)
    latents = np.concatenate([(first[None] + r[:, None] * u[:n])[order], first[None] + NEAR * u[n:]]).astype(np.float32)
    return latents, np.concatenate([g.integers(0, eu.CASES[CASE]["num_actions"], n), [0]]).astype(np.int64)


def placed_near(observed, seed):
    """One of the bank's last two entries, which make the two elements of a batch choose differently: ``NEAR`` from ``observed``
    (the latent one element reaches after its first step) in a seeded direction, so each element finds its own first."""
    u = np.random.default_rng(seed).standard_normal(len(observed))
    return (np.asarray(observed, dtype=np.float64) + NEAR * u / np.linalg.norm(u)).astype(np.float32)
