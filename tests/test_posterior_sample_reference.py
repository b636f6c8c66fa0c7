"""The posterior sample of include/abcdez_spec.h ("posterior summaries", POSTERIOR SAMPLE) as abcdez_amd.summary.sample_reference
restates it: integer masses, n strata over the total mass M, one Philox point per stratum (purpose ABZ_RNG_SAMPLE), the position
under the point.  No GPU: this file pins the DEFINITION (the Philox restatement against published vectors and the oracle's export,
the consequences the spec states as exact integers, the refusals) and the drivers' ``sample`` keyword through the CPU test engine;
tests/test_gpu_posterior_sample.py then holds the device to this reference exactly."""
import math

import numpy as np
import pytest

from abcdez_amd import summary as S
from abcdez_amd.summary import abz_rng, philox4x32, sample_options, sample_reference, stratum_bits, weight_fix
from test_spec_math import KAT, c_philox

SEED = 0x0123456789ABCDEF


# ------------------------------------------------------------------ the Philox restatement
@pytest.mark.parametrize("ctr,key,expect", KAT)
def test_philox_restatement_gives_the_published_known_answers(ctr, key, expect):
    assert philox4x32(ctr, key, rounds=10) == expect


def test_philox_restatement_is_the_oracles_export(oracle):
    rng = np.random.default_rng(5)
    for _ in range(200):
        ctr = [int(v) for v in rng.integers(0, 1 << 32, 4)]
        key = [int(v) for v in rng.integers(0, 1 << 32, 2)]
        assert philox4x32(ctr, key, rounds=oracle.lib().orc_philox_rounds()) == c_philox(oracle, ctr, key)
        for r in (1, 7, 10):
            assert philox4x32(ctr, key, rounds=r) == c_philox(oracle, ctr, key, rounds=r)


def test_abz_rng_packs_the_words_and_splits_the_seed_like_the_spec():
    r = philox4x32([7, 11, 0, S.RNG_SAMPLE], [0x89ABCDEF, 0x01234567])
    assert S.RNG_SAMPLE == 10
    assert abz_rng(SEED, 7, 11, 0, S.RNG_SAMPLE) == ((r[1] << 32) | r[0], (r[3] << 32) | r[2])


# ------------------------------------------------------------------ sample_reference
def weights(N, kind, seed=1):
    rng = np.random.default_rng(seed)
    if kind == "epa":                      # unequal positive weights with dead particles in between
        w = rng.random(N) * (rng.random(N) < 0.7)
        w[N // 3] += 0.5                   # (never all dead)
    elif kind == "indicator":              # equal weights on a prefix
        w = np.zeros(N)
        w[:max(1, (2 * N) // 3)] = 1.0
    elif kind == "heavy":                  # one position holds almost all the mass
        w = np.full(N, 1e-9)
        w[N // 2] = 1.0
    else:
        raise AssertionError(kind)
    return w / w.sum()


def counts_of(index, N):
    return np.bincount(index, minlength=N).tolist()


@pytest.mark.parametrize("kind", ["epa", "indicator", "heavy"])
@pytest.mark.parametrize("N,n", [(1, 1), (1, 5), (37, 7), (37, 37), (37, 112), (2049, 100), (300, 1000)])
def test_indices_are_sorted_count_and_obey_the_two_count_bounds(kind, N, n):
    w = weights(N, kind)
    index, M, n_mass = sample_reference(N, w, n, SEED, draw=3)
    m = weight_fix(w, N)
    assert M == sum(m) and n_mass == sum(1 for x in m if x >= 1)
    assert index.dtype == np.int64 and index.shape == (n,)
    assert np.all(np.diff(index) >= 0)                                   # non-decreasing in the stratum
    assert all(m[i] >= 1 for i in index.tolist())                        # only counting positions are drawn
    q = M // n
    for i, c in enumerate(counts_of(index, N)):                          # the spec's bounds, exact integers
        lo = max(0, m[i] // (q + 1) - 1)
        hi = -(-m[i] // q) + 1
        assert lo <= c <= hi, (i, c, lo, hi)
        assert m[i] >= 1 or c == 0


def test_the_index_is_the_definition_spelled_out():
    """every stratum by hand: a_s, h_s, the 128-bit product, the linear walk over the inclusive sums"""
    N, n, draw = 23, 9, 2
    w = weights(N, "epa", seed=4)
    m = weight_fix(w, N)
    M = sum(m)
    q, r = divmod(M, n)
    assert sum(q + (s < r) for s in range(n)) == M
    expect = []
    for s in range(n):
        a, h = s * q + min(s, r), q + (1 if s < r else 0)
        R = a + ((abz_rng(SEED, s, draw, 0, 10)[0] * h) >> 64)
        assert a <= R < a + h
        c = 0
        for i in range(N):
            c += m[i]
            if c > R:
                expect.append(i)
                break
    assert sample_reference(N, w, n, SEED, draw)[0].tolist() == expect


def test_equal_masses_give_the_identity_and_exact_multiples():
    N = 64                                                               # 1 / 32 on 32 positions: m = 2^41 each, k = 2 divides it
    w = np.zeros(N)
    live = np.arange(5, 37)
    w[live] = 1.0 / live.size
    m = weight_fix(w, N)
    assert set(m) == {0, 1 << 41}
    index, M, n_mass = sample_reference(N, w, live.size, SEED)
    assert n_mass == live.size and index.tolist() == live.tolist()       # n = n_mass: the identity over the counting positions
    index2 = sample_reference(N, w, 2 * live.size, SEED, draw=1)[0]
    assert index2.tolist() == np.repeat(live, 2).tolist()                # n = 2 n_mass: every position twice
    # an odd number of counting positions, masses that 1 does divide: still the identity
    w = np.zeros(50)
    w[3:44] = 1.0 / 41
    assert sample_reference(50, w, 41, SEED)[0].tolist() == list(range(3, 44))


def test_unit_masses_take_the_closed_form():
    for N, n in ((10, 10), (10, 40), (5000, 7), (7, 3)):
        index, M, n_mass = sample_reference(N, None, n, SEED, draw=9)
        b = stratum_bits(N)
        assert (M, n_mass) == (N << b, N)
        ones = sample_reference(N, np.full(N, 1.0 / N), n, SEED, draw=9)     # the same masses through the scan
        if weight_fix(np.full(N, 1.0 / N), N) == [1 << b] * N:
            assert ones[0].tolist() == index.tolist()
    assert sample_reference(10, None, 10, SEED)[0].tolist() == list(range(10))
    assert sample_reference(10, None, 40, SEED)[0].tolist() == np.repeat(np.arange(10), 4).tolist()


def test_zero_negative_and_nan_weights_are_never_drawn():
    w = np.array([0.0, 0.25, -0.5, 0.25, math.nan, 0.5, 0.0, 1e-30])
    index, M, n_mass = sample_reference(8, w, 500, SEED)
    assert n_mass == 3 and set(index.tolist()) == {1, 3, 5}              # 1e-30 is below half a unit of mass: it does not count
    c = counts_of(index, 8)
    assert (c[1], c[3], c[5]) == (125, 125, 250)                         # dyadic masses, n a multiple: exact shares


def test_draw_and_seed_change_the_points():
    w = weights(400, "epa")
    a = sample_reference(400, w, 300, SEED, draw=0)[0]
    assert np.array_equal(a, sample_reference(400, w, 300, SEED, draw=0)[0])
    assert not np.array_equal(a, sample_reference(400, w, 300, SEED, draw=1)[0])
    assert not np.array_equal(a, sample_reference(400, w, 300, SEED + 1, draw=0)[0])
    assert not np.array_equal(a, sample_reference(400, w, 300, SEED, draw=0, rounds=7)[0])
    assert np.array_equal(sample_reference(np.zeros((400, 3)), w, 300, SEED)[0], a)      # P only gives N


def test_refusals():
    w = weights(10, "epa")
    for bad in (0, -1, 1 << 31):
        with pytest.raises(ValueError, match="n must be"):
            sample_reference(10, w, bad, SEED)
    with pytest.raises(ValueError, match="carries mass"):
        sample_reference(4, np.array([0.0, -1.0, math.nan, 1e-40]), 3, SEED)
    with pytest.raises(ValueError, match="2\\^63"):
        sample_reference(4, np.full(4, 1e6), 3, SEED)                    # never normalised: 4 x 2^63 (saturated) would wrap
    with pytest.raises(ValueError, match="2\\^63"):
        sample_reference(1 << 23, None, 3, SEED)                         # 2^23 positions of 2^40
    with pytest.raises(ValueError, match="exceeds"):
        sample_reference(1, np.array([2.0 ** -39]), 3, SEED)             # M = 2
    with pytest.raises(ValueError, match="one weight per particle"):
        sample_reference(5, np.ones(4) / 4, 3, SEED)


def test_option_validation():
    assert sample_options(7) == dict(n=7, draw=0, blobs=None)
    assert sample_options(dict(n=np.int64(3), draw=5, blobs=False)) == dict(n=3, draw=5, blobs=False)
    for bad in (True, 2.5, "7", [7], dict(draw=1), dict(n=0), dict(n=1 << 31), dict(n=2.0), dict(n=True), dict(n=3, draw=-1),
                dict(n=3, draw=1 << 32), dict(n=3, blobs=1.5), dict(n=3, rows=2)):
        with pytest.raises(ValueError, match="sample"):
            sample_options(bad)


# ------------------------------------------------------------------ the drivers' keyword through the CPU test engine
def test_driver_keyword_gives_the_indexed_result(oracle):
    import abcdez_amd as A

    r = A.abcdesmc(A.Factored(A.Normal(0, 2), A.Normal(1, 2), A.DiscreteUniform(0, 6)), A.MVNormal((1.0, 2.0, 3.0)), 1.5, None,
                   nparticles=300, verbose=False, rng=11, ABCk=A.Epa0toeps, engine=oracle.oracle_engine, sample=dict(n=77, draw=2))
    s = r.sample
    assert (s.n, s.draw) == (77, 2) and s.blobs is None
    index, M, n_mass = sample_reference(r.P, r.Wns, 77, 11, draw=2, rounds=oracle.lib().orc_philox_rounds())
    assert np.array_equal(s.index, index) and (s.M, s.n_mass) == (M, n_mass)
    assert np.array_equal(s.P, r.P[s.index]) and np.array_equal(s.C, r.C[s.index])
    assert np.unique(r.Wns[r.Wns > 0]).size > 1 and np.all(r.Wns[s.index] > 0)

    r1 = A.abcdesmc(A.Normal(0, math.sqrt(10)), A.Normal1D(3.0), 0.5, None, nparticles=200, verbose=False, rng=3,
                    engine=oracle.oracle_engine, sample=50)
    assert r1.sample.P.shape == (50,) and np.array_equal(r1.sample.P, r1.P[r1.sample.index])      # squeezed like r.P

    m = A.abcdemc(A.Normal(0, math.sqrt(10)), A.Normal1D(3.0), 0.5, None, nparticles=40, generations=5, verbose=False, rng=3,
                  engine=oracle.oracle_engine, sample=dict(n=80))
    assert m.sample.index.tolist() == np.repeat(np.arange(40), 2).tolist() and np.array_equal(m.sample.P, m.P[m.sample.index])


def test_driver_keyword_validation_and_download_false(oracle):
    import abcdez_amd as A

    kw = dict(nparticles=100, verbose=False, rng=3, engine=oracle.oracle_engine)
    args = (A.Normal(0, math.sqrt(10)), A.Normal1D(3.0), 0.5, None)
    with pytest.raises(ValueError, match="sample"):
        A.abcdesmc(*args, sample=dict(n=0), **kw)
    with pytest.raises(ValueError, match="sample"):
        A.abcdemc(*args, sample="all", **kw)
    with pytest.raises(ValueError, match="download=False needs summary"):         # the message of old when neither is given
        A.abcdesmc(*args, download=False, **kw)
    with pytest.raises(ValueError, match="blobs=True needs"):
        A.abcdesmc(*args, sample=dict(n=5, blobs=True), **kw)
    r = A.abcdesmc(*args, download=False, sample=30, **kw)
    full = A.abcdesmc(*args, **kw)
    assert r.P is None and r.Wns is None and r.C is None and not hasattr(r, "summary")
    assert np.array_equal(r.sample.P, full.P[r.sample.index]) and np.array_equal(r.sample.C, full.C[r.sample.index])
