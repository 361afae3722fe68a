"""CPU tests (no GPU, no compute): ``a3vt_candidate_tally`` refuses what the contract in ``include/a3vt.h`` excludes with an error code
and a message that names the argument, before anything is launched — every call below passes fake device addresses that must
never be dereferenced on the host (the manner of ``test_latent_nn_capi.py``)."""
import pytest

FAKE = 0x7F0000001000        # a "device pointer": 16-byte aligned, never mapped on the host
GOOD = dict(scores=FAKE, candidates=FAKE + 0x1000, first_score=FAKE + 0x2000, taken=FAKE + 0x3000, K=50, E=3, A=50, unvisited=1e10,
            sums=FAKE + 0x4000, checks=FAKE + 0x5000, votes=FAKE + 0x6000, best=FAKE + 0x7000, best_score=FAKE + 0x8000, stream=None)
ORDER = ("scores", "candidates", "first_score", "taken", "K", "E", "A", "unvisited", "sums", "checks", "votes", "best", "best_score",
         "stream")


@pytest.fixture(scope="module")
def L():
    from a3vt_amd import lib
    return lib.load()


def call(L, **changes):
    a = dict(GOOD, **changes)
    return L.a3vt_candidate_tally(*(a[name] for name in ORDER)), L.a3vt_last_error().decode()


@pytest.mark.parametrize("name,values", [("K", (0, -1, 305)), ("E", (0, -2, 1025)), ("A", (0, -1, 305))])
def test_limits_outside(L, name, values):
    for v in values:
        rc, msg = call(L, **{name: v})
        assert rc != 0 and "candidate_tally" in msg and f"{name}={v}" in msg, (name, v, msg)


@pytest.mark.parametrize("name", ["scores", "candidates"])
def test_required_pointers(L, name):
    rc, msg = call(L, **{name: None})
    assert rc != 0 and f"{name}=NULL" in msg, msg


def test_pointers_that_go_together(L):
    rc, msg = call(L, checks=None)
    assert rc != 0 and "checks=NULL" in msg and "together" in msg, msg
    rc, msg = call(L, sums=None)
    assert rc != 0 and "sums=NULL" in msg and "together" in msg, msg
    rc, msg = call(L, best=None)
    assert rc != 0 and "best=NULL" in msg and "votes" in msg, msg
    rc, msg = call(L, first_score=None)
    assert rc != 0 and "first_score=NULL" in msg and "sums" in msg, msg


@pytest.mark.parametrize("name,align", [("scores", 4), ("candidates", 4), ("first_score", 4), ("taken", 4), ("best", 4), ("best_score", 4),
                                        ("sums", 8), ("checks", 8), ("votes", 8)])
def test_alignment(L, name, align):
    for off in (1, 2) + ((4,) if align == 8 else ()):
        rc, msg = call(L, **{name: GOOD[name] + off})
        assert rc != 0 and f"{name}=0x" in msg and f"{align}-byte aligned" in msg, (name, off, msg)


def test_the_tally_is_in_the_build():
    from a3vt_amd import lib
    assert "candidate_tally.hip" in lib.SOURCES and "a3vt_candidate_tally" in lib.SIGNATURES
