"""CPU tests of tests/philox_ref.py, the host emulations that tests/test_gpu_sampling.py holds csrc/sample.hip to: the
Philox4x32-10 against the published Random123 known answers, the draw emulation's counter / key / search conventions, and
the fp32 summation order of face_cdf_kernel — with its chunks joined it never steps down and gives a zero-area face no
interval of its own; the plain scan it replaces did both."""
import numpy as np
import pytest

import philox_ref as pr

# Random123 kat_vectors, philox4x32 with 10 rounds: counter, key -> output
KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,out", KAT, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(ctr, key, out):
    assert tuple(int(x) for x in pr.philox4x32_10(ctr, key)) == out


def test_philox_is_vectorised_over_the_counter():
    """A batch of counters gives what one counter at a time gives, in words below 2^32."""
    rng = np.random.default_rng(0)
    c = rng.integers(0, 2 ** 32, (50, 4), dtype=np.uint64)
    c[:3] = [k[0] for k in KAT]
    key = (0xa4093822, 0x299f31d0)
    r = pr.philox4x32_10(c, key)
    assert r.shape == (50, 4) and r.dtype == np.uint64 and (r < 2 ** 32).all()
    assert all(np.array_equal(r[i], pr.philox4x32_10(c[i], key)) for i in range(50))
    assert tuple(int(x) for x in r[2]) == KAT[2][2]


def test_counters_carry_and_wrap():
    c = pr.counters(2 ** 32 - 3, 6)
    assert c[:, 0].tolist() == [2 ** 32 - 3, 2 ** 32 - 2, 2 ** 32 - 1, 0, 1, 2] and c[:, 1].tolist() == [0, 0, 0, 1, 1, 1]
    c = pr.counters(2 ** 64 - 5, 8)
    assert c[:, 0].tolist() == [2 ** 32 - 5 + i for i in range(5)] + [0, 1, 2]
    assert c[:, 1].tolist() == [2 ** 32 - 1] * 5 + [0] * 3 and not c[:, 2:].any()


def test_u01_keeps_the_top_24_bits():
    x = np.array([0, 0xff, 0x100, 0xffffffff, 0xe169c58d], dtype=np.uint64)
    u = pr.u01(x)
    assert u.dtype == np.float32
    assert u.tolist() == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 0xe169c5 * 2.0 ** -24]


def test_emulate_draws_conventions():
    """Sample 0 of seed 0 / offset 0 is the first known answer; the mesh of sample i is (i // num) % batch; the seed's two
    halves are the key; a tied (zero-width) face is never returned, whatever the total; a one-face CDF returns face 0."""
    cdf = np.array([[0.0, 0.0, 0.25, 0.25, 0.25, 1.0, 1.0], [0.0, 0.0, 0.925, 0.925, 0.925, 3.7, 3.7]], dtype=np.float32)
    f, u, v = pr.emulate_draws(cdf, 0, 0, 2, 2, 700)
    assert f.shape == u.shape == v.shape == (2, 2, 700) and f.dtype == np.int32 and u.dtype == v.dtype == np.float32
    assert u[0, 0, 0] == np.float32((0xe169c58d >> 8) * 2.0 ** -24) and v[0, 0, 0] == np.float32((0xbc57ac4c >> 8) * 2.0 ** -24)
    assert f[0, 0, 0] == 5                                   # u01(0x6627e8d5) = 0.399...: past 0.25
    assert set(np.unique(f)) == {2, 5}
    assert not np.array_equal(u[:, 0], u[:, 1])              # every sample has a counter of its own
    # the flat order is (draw, mesh, sample): a second call that starts one mesh later sees the same stream shifted
    f2, u2, _ = pr.emulate_draws(cdf, 0, 700, 1, 2, 700)
    assert np.array_equal(u2[0, 0], u[0, 1]) and np.array_equal(u2[0, 1], u[1, 0])
    # the key: seed = k0 + 2^32 k1
    r = pr.philox4x32_10(pr.counters(0, 1), KAT[2][1])
    _, u3, _ = pr.emulate_draws(cdf, KAT[2][1][0] + (KAT[2][1][1] << 32), 0, 1, 2, 1)
    assert u3[0, 0, 0] == pr.u01(r[0, 1])
    f1, _, _ = pr.emulate_draws(np.array([[1.0]] * 3, dtype=np.float32), 5, 9, 2, 3, 10)
    assert not f1.any()
    with pytest.raises(AssertionError):
        pr.emulate_draws(np.array([[0.5, 0.25, 1.0]], dtype=np.float32), 0, 0, 1, 1, 4)


def soup_probabilities(F, seed):
    """fp32 probabilities of a random triangle soup whose every chunk starts (and ends) with a zero-area face."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.05, 1.0, F).astype(np.float32)
    per = pr.chunk_size(F)
    zero = np.zeros(F, dtype=bool)
    zero[::per] = True
    zero[per - 1::per] = True
    a[zero] = 0
    return a / a.sum(dtype=np.float32), zero, per


@pytest.mark.parametrize("F", [1000, 1280, 5120, 20480])
def test_cdf_order_is_monotone_with_zero_steps_and_the_old_one_was_not(F):
    """The scan with its chunks joined: no step down anywhere, a zero-probability face repeats its predecessor bit for bit
    (20 soups).  The plain scan it replaces, on the same numbers: both kinds of step at chunk starts — the fault that
    test_gpu_sampling's CDF assertions are there to catch.  On probabilities without zeros the two agree in every bit."""
    up = down = checked = 0
    for seed in range(20):
        p, zero, per = soup_probabilities(F, seed)
        new = pr.emulate_cdf(p)
        assert (np.diff(new) >= 0).all()
        prev = np.concatenate([[np.float32(0)], new[:-1]])
        assert np.array_equal(new[zero], prev[zero])
        assert abs(float(new[-1]) - 1.0) < 1e-4
        old = pr.emulate_cdf(p, old=True)
        starts = np.arange(per, F, per)                      # chunk starts other than face 0: all of zero area
        step = old[starts].astype(np.float64) - old[starts - 1]
        up, down, checked = up + int((step > 0).sum()), down + int((step < 0).sum()), checked + starts.size
    # and where no chunk starts with a zero-area face and the plain scan is monotone, the join changes none of its bits
    for seed in range(5):
        q = np.random.default_rng(seed).uniform(0.05, 1.0, F).astype(np.float32)
        q = q / q.sum(dtype=np.float32)
        plain = pr.emulate_cdf(q, old=True)
        assert (np.diff(plain) >= 0).all() and np.array_equal(pr.emulate_cdf(q), plain)
    print(f"old order, F={F}: of {checked} zero-area chunk starts the CDF stepped up at {up} and down at {down}")
    assert up > 0 and down > 0
