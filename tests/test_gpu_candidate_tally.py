"""``a3vt_candidate_tally`` (csrc/candidate_tally.hip) on the GPU against ``tally_util.contract``, a literal NumPy restatement of the
contract in ``include/a3vt.h``.  Everything is compared bit for bit: ``best``, ``sums``, ``checks`` and ``votes`` with
``np.array_equal``, ``best_score`` through its bit patterns (so a NaN equals a NaN and -0 differs from +0).  The cases are
``tally_util.cases()`` — the shapes at which the launch geometry changes ((3, 70, 5): an element's lanes no longer fill a wave;
(304, 5, 304): K * E exceeds the 1024-pair tile; (7, 1024, 304): one lane per element) and the contract's edges — every one on a
state that already holds unvisited, visited and chosen entries."""
import numpy as np
import pytest
import torch

import tally_util as tu

pytestmark = pytest.mark.gpu

CASES = tu.cases()


def dev(x, dtype):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


def c_entry(c, state=None, unvisited=tu.UNVISITED):
    """The C entry on a case (no Python-side checks) -> (best, best_score, sums, checks, votes) NumPy; ``state``: device state
    tensors to go on from instead of the case's."""
    from a3vt_amd import lib, ops
    L = lib.load()
    K, E = c["scores"].shape
    scores, cand = dev(c["scores"], torch.float32), dev(c["candidates"], torch.int32)
    first, taken = dev(c["first"], torch.float32), dev(c["taken"], torch.float32)
    sums, checks, votes = state if state is not None else (dev(c[n], torch.float64) for n in ("sums", "checks", "votes"))
    best = torch.full((E,), -7, dtype=torch.int32, device="cuda")
    best_score = torch.full((E,), -7.0, dtype=torch.float32, device="cuda")
    lib.check(L.a3vt_candidate_tally(lib.ptr(scores), lib.ptr(cand), lib.ptr(first if sums is not None else None), lib.ptr(taken),
                                     K, E, c["A"], unvisited, lib.ptr(sums), lib.ptr(checks), lib.ptr(votes), lib.ptr(best),
                                     lib.ptr(best_score), ops._stream()), "candidate_tally")
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (best, best_score, sums, checks, votes)), (sums, checks, votes)


def want_of(c, sums=None, checks=None, votes=None):
    sums, checks, votes = (c[n] if x is None else x for n, x in (("sums", sums), ("checks", checks), ("votes", votes)))
    return tu.contract(c["scores"], c["candidates"], c["first"], c["taken"], c["A"], sums, checks, votes)


def assert_same(got, want, where):
    for name, g, w in zip(("best", "best_score", "sums", "checks", "votes"), got, want):
        assert (g is None) == (w is None), (where, name)
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (where, name, g.dtype, w.dtype)
        same = np.array_equal(tu.bits(g), tu.bits(w)) if name == "best_score" else np.array_equal(g, w)
        assert same, f"{where}: {name} differs at {np.where(tu.bits(g) != tu.bits(w))[0][:8]}: {g[:8]} vs {w[:8]}"


@pytest.fixture(scope="module")
def wanted():
    """The restatement's answer to every case, computed once."""
    return {c["id"]: want_of(c) for c in CASES}


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_matches_the_restatement_bit_for_bit(cuda, wanted, c):
    got, _ = c_entry(c)
    assert_same(got, wanted[c["id"]], c["id"])
    again, _ = c_entry(c)
    assert_same(again, got, c["id"] + " (second run)")                     # the same bits on every call


def test_the_cases_reach_the_edges(wanted):
    """The restatement's answers show that the cases are what their names say."""
    by = {c["id"]: c for c in CASES}
    assert wanted["every-action-taken"][0][1] == -1 and np.isinf(wanted["every-action-taken"][1][1])
    assert wanted["every-action-taken"][4].sum() == by["every-action-taken"]["votes"].sum() + 1          # no vote for element 1
    best, score = wanted["inf-and-nan"][:2]
    assert list(best) == [1, 3, 0, 3, 0] and np.isnan(score[2]) and np.isinf(score[0])
    assert list(tu.bits(wanted["signed-zeros"][1])) == [0, 0x80000000, 0x80000000] and list(wanted["signed-zeros"][0]) == [0, 1, 0]
    assert wanted["same-action-big-first"][2][1] != wanted["same-action-small-first"][2][1]               # the e order shows
    assert list(wanted["sentinel-met-twice"][2]) == [2.125, 0.875] and list(wanted["sentinel-met-twice"][3]) == [4.0, 2.0]
    assert wanted["ties-across-k"][0][0] == by["ties-across-k"]["candidates"][1, 0]
    for c in CASES[:6]:
        if c["A"] >= 3:
            assert {tu.UNVISITED, tu.CHOSEN} <= set(c["sums"]) and tu.CHOSEN_VOTES in c["votes"] and (c["checks"] > 1).any()


@pytest.mark.parametrize("outside", [-1, "A"])
def test_a_candidate_outside_the_range_is_skipped(cuda, outside):
    """Straight to the C entry (``ops.candidate_tally`` refuses such a table): the pair is skipped by the choice, the tally and
    the votes, and everything else is as if the pair were not there."""
    c = dict(next(c for c in CASES if c["id"] == "shape-6x2x6"))
    bad = -1 if outside == -1 else c["A"]
    cand = c["candidates"].copy()
    cand[0, 0], cand[3, 1], cand[5, 1] = bad, bad, bad
    c["candidates"] = cand
    got, _ = c_entry(c)
    assert_same(got, want_of(c), f"candidate {bad}")
    assert got[0].min() >= -1 and got[0].max() < c["A"]
    assert got[3].sum() == c["checks"].sum() + cand.size - 3                                             # every other pair counted once


def test_three_calls_accumulate(cuda):
    c = next(c for c in CASES if c["id"] == "shape-50x3x50")
    want, state = None, None
    for call in range(3):
        got, state = c_entry(c, state=state)
        want = want_of(c) if want is None else want_of(c, *want[2:])
        assert_same(got, want, f"call {call}")


def test_ops_runs_the_kernel_and_refuses_what_the_contract_excludes(cuda):
    from a3vt_amd import ops
    c = next(c for c in CASES if c["id"] == "limited-search")
    sums, checks, votes = (dev(c[n], torch.float64) for n in ("sums", "checks", "votes"))
    best, best_score = ops.candidate_tally(dev(c["scores"], torch.float32), torch.from_numpy(c["candidates"]), dev(c["first"], torch.float32),
                                           dev(c["taken"], torch.float32), sums=sums, checks=checks, votes=votes)
    assert best.is_cuda and best_score.is_cuda
    assert_same(tuple(t.cpu().numpy() for t in (best, best_score, sums, checks, votes)), want_of(c), "ops")
    cand = c["candidates"].copy()
    cand[1, 2] = c["A"]
    with pytest.raises(ValueError, match="candidates outside"):
        ops.candidate_tally(dev(c["scores"], torch.float32), dev(cand, torch.int32), dev(c["first"], torch.float32),
                            dev(c["taken"], torch.float32), votes=votes)
