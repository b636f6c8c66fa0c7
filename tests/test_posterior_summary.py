"""Posterior summaries, the parts that need no GPU: the numpy restatement of the summary arithmetic
(abcdez_amd/summary.py; include/abcdez_spec.h, "posterior summaries") against the CPU oracle's tile tree and against numpy's own
weighted mean / covariance / quantile, and the drivers' ``summary`` / ``download`` keywords through the oracle engine."""
import math

import numpy as np
import pytest

import abcdez_amd as A
from abcdez_amd.summary import order_keys, summary_reference, tile_tree_sum

U = 2.0 ** -53
PROBS = (0.0, 0.025, 0.5, 0.975, 1.0)


def spread(rng, n):
    """mixed signs, magnitudes spread over 20 binades"""
    return rng.choice([-1.0, 1.0], n) * np.exp2(rng.uniform(-10.0, 10.0, n)) * (1.0 + rng.random(n))


@pytest.mark.parametrize("n", [1, 2, 511, 2047, 2048, 2049, 4099, 2048 * 3 + 1, 2 ** 22 + 5])
def test_numpy_tile_tree_is_the_oracles_bit_for_bit(oracle, n):
    """2^22 + 5 > 2048^2: 2049 partials, so the tree reaches level 2"""
    x = spread(np.random.default_rng(n), n)
    got = tile_tree_sum(x)
    want = oracle.lib().orc_tree_sum(x.ctypes.data, x.size)
    assert np.float64(got).tobytes() == np.float64(want).tobytes(), (n, got, want)
    assert abs(got - math.fsum(x)) <= 64 * U * np.abs(x).sum()


def test_tile_tree_sums_the_columns_of_a_matrix_like_single_vectors():
    x = spread(np.random.default_rng(5), 3 * 5000).reshape(5000, 3)
    cols = tile_tree_sum(x)
    for k in range(3):
        assert cols[k].tobytes() == np.float64(tile_tree_sum(x[:, k])).tobytes()
    assert math.copysign(1.0, tile_tree_sum(np.array([-0.0]))) == 1.0          # the missing elements of a tile are +0.0


@pytest.mark.parametrize("N,d,weights", [(300, 1, "uniform"), (5001, 3, "uniform"), (5001, 3, "varied"), (2049, 2, "unit")])
def test_reference_against_numpy_mean_and_cov(N, d, weights):
    """every sum within 64 * 2^-53 * sum|term| of numpy's (the pairwise-summation bound with room for the divisions)"""
    rng = np.random.default_rng(N + d)
    X = 1.0 + 2.0 * rng.standard_normal((N, d))
    if weights == "unit":
        w, Wns = np.ones(N), None
    else:
        alive = rng.random(N) < 0.7
        w = np.where(alive, (1.0 / alive.sum()) if weights == "uniform" else rng.random(N), 0.0)
        Wns = w
        X[~alive] = np.nan                               # dead rows may hold anything
    live = w > 0
    s = summary_reference(X if d > 1 else X[:, 0], Wns, cov=True, corrected=True)
    assert s.n_pos == live.sum() and s.mean.shape == (d,) and s.cov.shape == (d, d)
    Xl, wl = X[live], w[live]
    assert abs(s.W - math.fsum(wl)) <= 64 * U * wl.sum() and abs(s.Q - math.fsum(wl * wl)) <= 64 * U * (wl * wl).sum()
    assert s.ess == s.W * s.W / s.Q
    want_mean = np.average(Xl, axis=0, weights=wl)
    for k in range(d):
        tol = 64 * U * np.abs(wl * Xl[:, k]).sum() / s.W
        print("mean", k, abs(s.mean[k] - want_mean[k]), tol)
        assert abs(s.mean[k] - want_mean[k]) <= tol
    for corrected, ddof in ((True, 1), (False, 0)):
        sc = summary_reference(X, Wns, cov=True, corrected=corrected)
        want_cov = np.atleast_2d(np.cov(Xl.T, aweights=wl, ddof=ddof))
        den = s.W - s.Q / s.W if corrected else s.W
        C = Xl - s.mean
        for j in range(d):
            for k in range(d):
                tol = 64 * U * np.abs(wl * C[:, j] * C[:, k]).sum() / den
                print("cov", corrected, j, k, abs(sc.cov[j, k] - want_cov[j, k]), tol)
                assert abs(sc.cov[j, k] - want_cov[j, k]) <= tol
                assert sc.cov[j, k] == sc.cov[k, j]
    assert summary_reference(X, Wns, cov=False).cov is None


@pytest.mark.parametrize("n", [1, 11, 201, 401, 2001])
def test_reference_quantiles_are_numpys_exactly(n):
    """type 7 is numpy's default ("linear").  The spec interpolates as v_j + g (v_j+1 - v_j) (Julia's formula, as at smc:301),
    numpy as a lerp with another rounding sequence; on values that are multiples of 2^-10 below 2^10 and positions (n - 1) p whose
    fraction is a multiple of 2^-2 every operation of either formula is exact, so the two must agree exactly -- sizes with
    (n - 1) a multiple of 200 or of 10, plus the degenerate ones."""
    rng = np.random.default_rng(n)
    N = n + 40
    X = rng.integers(-2 ** 19, 2 ** 19, (N, 2)).astype(np.float64) / 1024.0
    w = np.zeros(N)
    pos = rng.permutation(N)[:n]
    w[pos] = 1.0 / n
    X[w == 0] = np.inf
    s = summary_reference(X, w, cov=False, quantiles=PROBS)
    assert s.quantiles.shape == (len(PROBS), 2)
    for i, p in enumerate(PROBS):
        frac = ((n - 1) * p) % 1.0
        assert frac * 4 == int(frac * 4), "the sizes of this test make the interpolation exact"
        for k in range(2):
            assert s.quantiles[i, k] == np.quantile(X[w > 0, k], p), (n, p, k)
    for k in range(2):
        assert s.quantiles[0, k] == X[w > 0, k].min() and s.quantiles[-1, k] == X[w > 0, k].max()
    two = summary_reference(np.array([7.25, np.nan, -1.5]), np.array([0.5, 0.0, 0.5]), cov=False, quantiles=(0.0, 0.5, 1.0))
    assert list(two.quantiles[:, 0]) == [-1.5, 2.875, 7.25]                      # n = 2: j stays 1


def test_reference_orders_negative_values_and_signed_zeros_like_the_device_select():
    v = np.array([3.0, -0.0, 0.0, -2.5, -1e-300, 1e-300, -np.inf, np.inf])
    k = order_keys(v)
    assert list(v[np.argsort(k)]) == [-np.inf, -2.5, -1e-300, 0.0, 0.0, 1e-300, 3.0, np.inf]
    assert np.signbit(v[np.argsort(k)][3]) and not np.signbit(v[np.argsort(k)][4])       # -0.0 below +0.0
    s = summary_reference(np.array([0.5, -0.0, -0.25, 0.0, -0.0]), None, cov=False, quantiles=(0.0, 0.25, 0.5, 0.75, 1.0))
    assert list(s.quantiles[:, 0]) == [-0.25, 0.0, 0.0, 0.0, 0.5]


def test_reference_refusals():
    X = np.arange(10.0)
    with pytest.raises(ValueError, match="no particle has a positive weight"):
        summary_reference(X, np.zeros(10))
    with pytest.raises(ValueError, match="weighted quantiles are not provided"):
        summary_reference(X, np.arange(10.0), quantiles=(0.5,))
    with pytest.raises(ValueError, match=r"p must be in \[0, 1\]"):
        summary_reference(X, None, quantiles=(1.5,))
    assert summary_reference(X, np.arange(10.0)).mean[0] == pytest.approx(np.average(X, weights=np.arange(10.0)))


PRIOR, SIM = A.Normal(0, math.sqrt(10)), A.Normal1D(3.0)


def test_drivers_summary_and_download_keywords(oracle):
    kw = dict(nparticles=400, verbose=False, engine=oracle.oracle_engine, rng=11)
    r0 = A.abcdesmc(PRIOR, SIM, 0.3, None, **kw)
    r = A.abcdesmc(PRIOR, SIM, 0.3, None, summary=True, **kw)
    rn = A.abcdesmc(PRIOR, SIM, 0.3, None, summary=None, **kw)
    # summary=None: the result object as before, field for field
    assert not hasattr(r0, "summary") and not hasattr(rn, "summary")
    assert sorted(vars(rn)) == sorted(vars(r0)) and sorted(set(vars(r)) - set(vars(r0))) == ["summary"]
    for f in ("P", "Wns", "C"):
        assert np.array_equal(getattr(r0, f), getattr(r, f)) and np.array_equal(getattr(r0, f), getattr(rn, f))
    assert r0.logZ == r.logZ == rn.logZ
    live = r.Wns > 0
    s = r.summary
    tol = 64 * U * np.abs(r.Wns[live] * r.P[live]).sum() / s.W
    print("mean", s.mean[0], r.P[live].mean(), tol)
    assert abs(s.mean[0] - r.P[live].mean()) <= tol             # test/runtests.jl:159-162
    assert s.n_pos == live.sum() and s.cov.shape == (1, 1) and s.quantiles.shape == (0, 1)
    assert abs(s.cov[0, 0] - r.P[live].var(ddof=1)) <= 64 * U * s.cov[0, 0]      # every term of S is positive: sum|term| = S
    assert abs(s.ess - s.n_pos) <= 1e-9 * s.n_pos              # uniform weights
    # options, and the result without the rows
    r2 = A.abcdesmc(PRIOR, SIM, 0.3, None, summary=dict(cov=False, quantiles=(0.025, 0.975)), download=False, **kw)
    assert r2.P is None and r2.Wns is None and r2.C is None and r2.blobs is None and r2.logZ == r.logZ
    assert r2.summary.cov is None and r2.summary.mean[0] == s.mean[0]
    assert list(r2.summary.quantiles[:, 0]) == list(summary_reference(r.P, r.Wns, cov=False, quantiles=(0.025, 0.975)).quantiles[:, 0])
    with pytest.raises(ValueError, match="download=False needs summary"):
        A.abcdesmc(PRIOR, SIM, 0.3, None, download=False, **kw)
    with pytest.raises(ValueError, match="unknown option"):
        A.abcdesmc(PRIOR, SIM, 0.3, None, summary=dict(median=True), **kw)
    # abcdemc: no weights, every particle counts once
    mkw = dict(nparticles=200, generations=5, verbose=False, engine=oracle.oracle_engine, rng=11)
    m0 = A.abcdemc(PRIOR, SIM, 0.3, None, **mkw)
    m = A.abcdemc(PRIOR, SIM, 0.3, None, summary=dict(quantiles=(0.5,)), **mkw)
    assert sorted(set(vars(m)) - set(vars(m0))) == ["summary"] and np.array_equal(m.P, m0.P)
    assert m.summary.n_pos == 200 and m.summary.W == 200.0 and m.summary.quantiles[0, 0] == summary_reference(m.P, None, quantiles=(0.5,)).quantiles[0, 0]
    assert abs(m.summary.mean[0] - m.P.mean()) <= 64 * U * np.abs(m.P).sum() / 200
    with pytest.raises(ValueError, match="download=False needs summary"):
        A.abcdemc(PRIOR, SIM, 0.3, None, download=False, **mkw)
