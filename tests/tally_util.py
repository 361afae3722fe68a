"""Shared by the candidate-tally and dataset-specific-policy tests and by ``tests/golden/make_golden_dataset_specific.py``: a literal
restatement of the contract of ``a3vt_candidate_tally`` (``include/a3vt.h``) in NumPy — the division is ``np.float32 / np.float32``,
the add is ``np.float64(np.float32(sum) + r)``, every order is an explicit Python loop — the cases the kernel and its host form are
run on, and the recipe of the g22 fixture (what is drawn from which seed), so that the generator and the tests build the same
batches, models and surface draws."""
import math

import numpy as np

UNVISITED, CHOSEN, CHOSEN_VOTES = 1e10, 1e20, -1e20


def comes_before(s2, s1):
    """Does score ``s2`` rank strictly before ``s1``?  Numbers by value (-0 == +0), +inf after them, a NaN after +inf."""
    n1, n2 = math.isnan(s1), math.isnan(s2)
    if n1 or n2:
        return n1 and not n2
    return s2 < s1


def contract(scores, candidates, first_score, taken, A, sums=None, checks=None, votes=None, unvisited=UNVISITED):
    """``a3vt_candidate_tally`` word for word -> ``(best (E,) int32, best_score (E,) float32, sums, checks, votes)``; the state
    arrays are updated copies (None where none was given)."""
    scores, candidates = np.asarray(scores, dtype=np.float32), np.asarray(candidates, dtype=np.int32)
    K, E = scores.shape
    sums, checks, votes = (None if x is None else np.array(x, dtype=np.float64) for x in (sums, checks, votes))
    best, best_score = np.full(E, -1, dtype=np.int32), np.full(E, np.inf, dtype=np.float32)
    for e in range(E):
        found = False
        for k in range(K):
            a = int(candidates[k, e])
            if a < 0 or a >= A:
                continue
            if taken is not None and taken[e, a] != 0:
                continue
            if not found or comes_before(float(scores[k, e]), float(best_score[e])):
                found, best[e], best_score[e] = True, a, scores[k, e]
    if sums is not None:
        for k in range(K):
            for e in range(E):
                a = int(candidates[k, e])
                if a < 0 or a >= A:
                    continue
                r = np.float32(scores[k, e]) / np.float32(first_score[e])
                if sums[a] == np.float64(unvisited):
                    sums[a] = np.float64(r)
                else:
                    sums[a] = np.float64(np.float32(sums[a]) + r)
                checks[a] += 1.0
    if votes is not None:
        for e in range(E):
            if best[e] >= 0:
                votes[best[e]] += 1.0
    return best, best_score, sums, checks, votes


def state(A, rng):
    """Per-action state that already holds unvisited, visited and chosen entries: ``(sums, checks, votes)`` float64."""
    kind = rng.integers(0, 3, size=A)
    if A >= 3:
        kind[:3] = rng.permutation(3)
    visited = rng.uniform(0.5, 40.0, size=A).astype(np.float32).astype(np.float64)      # (a running fp32 sum)
    sums = np.where(kind == 0, UNVISITED, np.where(kind == 1, visited, CHOSEN))
    checks = np.where(kind == 1, 1.0 + rng.integers(1, 40, size=A), 1.0)
    votes = np.where(kind == 2, CHOSEN_VOTES, np.where(kind == 1, rng.integers(1, 9, size=A).astype(np.float64), 0.0))
    return sums, checks, votes


def table(K, E, A, rng, per_element=False, taken_share=0.3):
    """A random case: ``scores`` (K, E) and ``first_score`` (E,) float32 inside the normal range, ``candidates`` (K, E) int32
    in [0, A) (``per_element``: every element its own sample without replacement where K <= A, the limited search) and
    ``taken`` (E, A) float32."""
    scores = rng.uniform(0.05, 30.0, size=(K, E)).astype(np.float32)
    first = rng.uniform(1.0, 40.0, size=E).astype(np.float32)
    if per_element and K <= A:
        candidates = np.stack([rng.permutation(A)[:K] for _ in range(E)], axis=1).astype(np.int32)
    elif K == A and not per_element:
        candidates = np.repeat(np.arange(A, dtype=np.int32)[:, None], E, axis=1)      # the full search
    else:
        candidates = rng.integers(0, A, size=(K, E)).astype(np.int32)
    taken = (rng.random((E, A)) < taken_share).astype(np.float32)
    return scores, candidates, first, taken


SHAPES = [(1, 1, 1), (6, 2, 6), (50, 3, 50), (3, 70, 5), (304, 5, 304), (7, 1024, 304)]


def bits(x):
    """An array's bytes as unsigned integers: equal exactly when the arrays are bit-equal (NaN payloads and the sign of zero
    included)."""
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _case(name, scores, candidates, first, taken, A, mode="all", seed=7):
    sums, checks, votes = state(A, np.random.default_rng(seed))
    return dict(id=name, scores=np.asarray(scores, dtype=np.float32), candidates=np.asarray(candidates, dtype=np.int32),
                first=np.asarray(first, dtype=np.float32), taken=None if taken is None else np.asarray(taken, dtype=np.float32), A=A,
                sums=sums if mode in ("all", "sums") else None, checks=checks if mode in ("all", "sums") else None,
                votes=votes if mode in ("all", "votes") else None)


def cases():
    """The cases the kernel (``test_gpu_candidate_tally.py``) and the host form (``test_dataset_specific_host.py``) are compared
    with ``contract`` on; every candidate is inside [0, A)."""
    rng = np.random.default_rng(2203)
    out = []
    for K, E, A in SHAPES:
        sc, ca, fi, ta = table(K, E, A, rng)
        if (K, E, A) == (3, 70, 5):
            ca[:] = rng.integers(0, 2, size=ca.shape)                     # every action many times within one k row
        if E >= 3:
            sc[rng.integers(0, K), 1] = np.inf
        out.append(_case(f"shape-{K}x{E}x{A}", sc, ca, fi, ta, A, seed=K + E))
    sc, ca, fi, ta = table(3, 4, 9, rng, per_element=True)
    out.append(_case("limited-search", sc, ca, fi, ta, 9))
    sc, ca, fi, ta = table(50, 3, 50, rng)
    out.append(_case("taken-none", sc, ca, fi, None, 50))
    out.append(_case("only-sums", sc, ca, fi, ta, 50, mode="sums"))
    out.append(_case("only-votes", sc, ca, fi, ta, 50, mode="votes"))
    out.append(_case("pure-choice", sc, ca, fi, ta, 50, mode="none"))
    # two elements try the same action in one row, in both e orders: in fp32 (1 + 2^24) + 1 = 2^24 but (1 + 1) + 2^24 = 2^24 + 2
    big, small = 16777216.0, 1.0
    for name, row in (("same-action-big-first", [big, small]), ("same-action-small-first", [small, big])):
        c = _case(name, [row, [1.0, 2.0]], [[1, 1], [0, 2]], [1.0, 1.0], np.zeros((2, 3)), 3)
        c["sums"][:], c["checks"][:] = [UNVISITED, 1.0, CHOSEN], [1.0, 5.0, 1.0]
        out.append(c)
    c = _case("sentinel-met-twice", [[2.0, 3.0], [5.0, 7.0]], [[0, 0], [0, 1]], [4.0, 8.0], np.zeros((2, 2)), 2)
    c["sums"][:], c["checks"][:] = [UNVISITED, UNVISITED], [1.0, 1.0]
    out.append(c)
    sc, ca, fi, ta = table(6, 3, 6, rng, taken_share=0.0)
    sc[1:4, 0], sc[:, 1], sc[4:, 2] = sc[1, 0], 2.5, sc[0, 2]
    sc[1:4, 0] = sc.min() / 2                                             # the tied scores are element 0's lowest
    out.append(_case("ties-across-k", sc, ca, fi, ta, 6))
    sc = np.array([[0.0, -0.0, 1.0], [-0.0, 0.0, -0.0], [3.0, 3.0, 0.0]], dtype=np.float32)
    out.append(_case("signed-zeros", sc, [[0, 1, 2], [1, 2, 0], [2, 0, 1]], [1.0, 2.0, 3.0], np.zeros((3, 3)), 3))
    nan, inf = np.nan, np.inf
    sc = np.array([[nan, inf, nan, nan, 4.0], [inf, nan, nan, 2.0, nan], [nan, inf, nan, nan, inf], [inf, 3.0, nan, 2.0, nan]],
                  dtype=np.float32)
    ta = np.zeros((5, 4))
    ta[3, 1] = 1                                                          # element 3: its first 2.0 is taken, the later one wins
    out.append(_case("inf-and-nan", sc, np.repeat(np.arange(4)[:, None], 5, axis=1), np.ones(5), ta, 4, mode="votes"))
    sc, ca, fi, ta = table(6, 2, 6, rng)
    ta[1, :] = 1.0
    out.append(_case("every-action-taken", sc, ca, fi, ta, 6))
    return out


# ---- the recipe of g22_dataset_specific.npz ---------------------------------------------------------------------------------------
# env_util's case "b" (models, settings, surface draws: four fingers, E = 2, 6 actions); batches, sensor records and clouds in the
# manner of nn_policy_util, every batch its own two objects.  Five train batches, so int(5 * 0.4) = 2 are swept.  ``seed`` is the
# one the generator settled on (it re-seeds until the reference's own decisions have the gaps it asserts) and is stored in the file.
FIXTURE = "g22_dataset_specific.npz"
CASE = "b"
TRAIN_BATCHES, VALID_BATCHES = 5, 2
SWEEPS = 3
GREEDY_CHECKS = (6, 3, 6)          # per sweep: full search, limited search, full search
SEED = 12400       # the first of 2200, 2300, .. the generator's conditions hold for (smallest gaps: greedy 1.05e-2, LEBA 2.0e-2)
MIN_GAP = 1e-2


COUNTS = {"train": TRAIN_BATCHES, "valid": VALID_BATCHES}


def records(seed):
    """Every batch's sensor records in one mapping ``{(object id, action): record}``, tables under the idle rule."""
    import env_util as eu
    n = eu.CASES[CASE]["num_actions"]
    return eu.batch_records(seed, COUNTS, n, eu.status_tables(seed, COUNTS, n))


def batches(seed, kind):
    """The ``kind`` ("train" / "valid") loader as a list of batches."""
    import env_util as eu
    return eu.batches(seed, kind, COUNTS[kind])


def engine_args(evaluate, **kw):
    """``env_util.env_args`` of the case plus what the engines read."""
    import env_util as eu
    return eu.env_args(CASE, eval=evaluate, greedy_checks=GREEDY_CHECKS[0], exp_type="g22", pretrained=False, visualize=False,
                       use_recon=False, **kw)
