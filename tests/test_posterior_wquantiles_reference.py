"""The weighted marginal quantile of include/abcdez_spec.h ("posterior summaries", weighted quantiles) as
abcdez_amd.summary.summary_reference(..., wquantiles=) restates it literally: sort by (order key, mass), Python integers.  No GPU:
this file pins the DEFINITION (worked cases, a plain double-precision restatement, the unweighted type-7 quantile for equal
weights, the edge cases); tests/test_gpu_posterior_wquantiles.py then holds the device to this reference bit for bit."""
import math

import numpy as np
import pytest

from abcdez_amd.summary import (order_keys, stratum_bits, summary_options, summary_reference, weight_fix, wquantile_column,
                                wquantiles_reference)

SHAPES = (300, 2048, 5001)
PROBS27 = tuple(float(p) for p in np.r_[np.linspace(0.0, 1.0, 21), [0.025, 0.975, 1e-9, 1.0 - 1e-9, 1.0 / 3.0, 0.999]])


def wq(values, weights, probs, N=None):
    values = np.asarray(values, dtype=np.float64)
    r = summary_reference(values, np.asarray(weights, dtype=np.float64), cov=False, wquantiles=probs)
    assert r.wquantiles.shape == (len(probs), 1) and r.wprobs == tuple(probs)
    return r.wquantiles[:, 0], r


def test_the_worked_cases_exactly():
    q, r = wq([1.0, 2.0, 4.0], [0.25, 0.25, 0.5], (0.0, 0.5, 1.0))
    assert q.tolist() == [1.0, 2.5, 4.0]
    assert r.n_mass == 3 and r.M == 3 << 40 and stratum_bits(3) == 40
    q, r = wq([2.0, 1.0, 2.0, 4.0], [0.125, 0.25, 0.125, 0.5], (0.5,))
    assert q.tolist() == [2.5] and r.M == 4 << 40
    # by hand: masses (2, 1, 1, 1) 2^39 in the order (1, 2, 2, 4) -> S = (2, 3, 4, 8) 2^39, H = 2^40 + floor(0.5 * 3 * 2^40) = 5 2^39
    # -> k = 4, g = (5 - 4) / 4, q = 2 + 0.25 * 2


def test_masses_are_the_resamplers_fixed_point():
    assert [stratum_bits(n) for n in (1, 2, 3, 2 ** 23, 2 ** 23 + 1, 2 ** 25, 2 ** 31 - 1)] == [40, 40, 40, 40, 39, 38, 32]
    assert weight_fix([0.25, 0.0, -1.0, np.nan, 2.0 ** -70, np.inf, 1.0], 4) == [1 << 40, 0, 0, 0, 0, 1 << 63, 4 << 40]
    assert weight_fix([1.5 * 2.0 ** -42, 2.5 * 2.0 ** -42], 4) == [2, 2]          # round half to even


def float_restatement(values, masses, p):
    """the same formula in plain double precision, no floor: cumulative sum in sorted order"""
    keys = order_keys(values)
    order = np.lexsort((masses, keys))
    v, m = values[order], masses[order].astype(np.float64)
    cs = np.cumsum(m)
    h = m[0] + p * (cs[-1] - m[0])
    k = int(np.searchsorted(cs, h, side="right"))
    if len(v) == 1 or k >= len(v):
        return v[-1]
    return v[k - 1] + ((h - cs[k - 1]) / m[k]) * (v[k] - v[k - 1])


@pytest.mark.parametrize("N", SHAPES)
def test_against_a_float_restatement(N):
    """Weights k_i / 2^s with k_i < 2^20 and 2^s >= sum(k): the masses k_i N 2^(40 - s) are exact integers below 2^53 and so is
    every partial sum, hence the float cumulative sum rounds NOTHING here.  What is left:
      * the target: the integer definition drops the fraction of p (M - m_(1)) (< 1), the float form rounds m_(1) + p (M - m_(1))
        once more (<= 1/2, the sum is below 2^53): |H - h| < 3/2;
      * q as a function of the target is continuous and piecewise linear with slope (v_k - v_k-1) / m_(k) <= range / m_min, so
        the targets contribute at most 1.5 range / m_min, whichever segment either lands in;
      * evaluating g and q in doubles: one division, one product, one sum, each within 2^-53 relative, on magnitudes <= range +
        max|v| <= 3 max|v|: together below 2^-49 max|v|."""
    rng = np.random.default_rng(N)
    values = rng.standard_normal(N)
    values[rng.integers(0, N, 20)] = values[rng.integers(0, N, 20)]              # some ties
    k = rng.integers(1, 1 << 20, N)
    k[rng.random(N) < 0.3] = 0
    k[0] = max(k[0], 1)
    s = math.ceil(math.log2(int(k.sum())))
    w = k / 2.0 ** s
    masses = np.array(weight_fix(w, N), dtype=object)
    assert all(int(m) == int(kk) * N * (1 << 40) >> s and (int(kk) * N << 40) % (1 << s) == 0 for m, kk in zip(masses, k))
    q, r = wq(values, w, PROBS27)
    live = k > 0
    assert r.n_mass == live.sum() and r.M == sum(int(m) for m in masses) < 1 << 53
    vl, ml = values[live], np.array([int(m) for m in masses[live]], dtype=np.int64)
    bound = 1.5 * (vl.max() - vl.min()) / float(ml.min()) + 2.0 ** -49 * np.abs(vl).max()
    worst = 0.0
    for i, p in enumerate(PROBS27):
        err = abs(q[i] - float_restatement(vl, ml, p))
        worst = max(worst, err)
        assert err <= bound, (p, q[i], err, bound)
    print("N", N, "worst |integer - float|", worst, "bound", bound)


@pytest.mark.parametrize("N", SHAPES)
@pytest.mark.parametrize("share", [1.0, 0.6])
def test_equal_weights_are_the_type7_quantile(N, share):
    """n of N positions at weight 1 / n: |wquantile - type-7 quantile| <= 2^-38 (max - min of the column).  |delta g| <= 1 / m +
    n 2^-52 with m >= 2^40 and n <= 5001, and q is continuous in g across the change of j."""
    rng = np.random.default_rng(N + int(10 * share))
    live = np.ones(N, dtype=bool) if share == 1.0 else rng.random(N) < share
    n = int(live.sum())
    w = np.where(live, 1.0 / n, 0.0)
    X = rng.standard_normal((N, 2))
    r = summary_reference(X, w, cov=False, quantiles=PROBS27, wquantiles=PROBS27)
    assert r.n_mass == r.n_pos == n and r.M >= n << 40
    span = X[live].max(axis=0) - X[live].min(axis=0)
    err = np.abs(r.wquantiles - r.quantiles) / span
    print("N", N, "n", n, "worst |wquantile - type 7| / range", err.max())
    assert (err <= 2.0 ** -38).all()
    assert np.array_equal(r.wquantiles[0], X[live].min(axis=0)) and np.array_equal(r.wquantiles[20], X[live].max(axis=0))   # p = 0, 1


def test_ties_with_different_masses():
    """values (1, 2, 2, 4) with masses (2, 1, 3, 2) 2^39 at N = 4: S = (2, 3, 6, 8) 2^39, M - m_(1) = 6 2^39.
    p = 1/12: H = 2.5 -> crossing in the FIRST element of the tie group {2, 2}: q = 1 + 0.5 (2 - 1)
    p = 1/3:  H = 4   -> crossing in its second element: v_k-1 = v_k = 2, q = 2 whatever g
    p = 5/6:  H = 7   -> k = 4: q = 2 + (7 - 6) / 2 (4 - 2) = 3"""
    vals, w = [2.0, 1.0, 4.0, 2.0], [0.375, 0.25, 0.25, 0.125]
    # H = 2^40 + floor(p 6 2^39); p = 1/12 and 1/3 are not dyadic: take the probabilities from the wanted targets instead
    q, r = wq(vals, w, (0.0, 0.09, 0.25, 0.5, 0.75, 1.0))
    assert r.M == 4 << 40 and r.n_mass == 4
    # p = 0.25: H = 2 + 1.5 = 3.5 (2^39) -> S_2 = 3 <= H < S_3 = 6: second element of the group: q = 2
    # p = 0.5: H = 5 -> still the second element: q = 2;  p = 0.75: H = 6.5 -> k = 4, g = 0.25: q = 2.5;  p = 0: H = 2 -> k = 2, g = 0
    assert q[0] == 1.0 and q[2] == 2.0 and q[3] == 2.0 and q[4] == 2.5 and q[5] == 4.0
    # p = 0.09: H = 2 + floor(0.54 * 2^39) / 2^39: the first element of the group (mass 1): q = 1 + g, g = floor(0.54 2^39) / 2^39
    g = math.floor(0.09 * float(6 << 39)) / float(1 << 39)
    assert 0.5 < g < 1.0 and q[1] == 1.0 + g * (2.0 - 1.0)
    # the same values with the masses of the tie group swapped in position: indistinguishable
    q2, _ = wq([2.0, 1.0, 4.0, 2.0], [0.125, 0.25, 0.25, 0.375], (0.0, 0.09, 0.25, 0.5, 0.75, 1.0))
    assert np.array_equal(q, q2)


def test_signed_zeros_are_ordered():
    """-0.0 below +0.0.  v_n is returned as it is (p = 1): +0.0 where both are there, -0.0 where it is the largest value; an
    interpolated -0.0 + g (+0.0 - -0.0) is +0.0 by IEEE addition.  The order shows in the masses: (-1, -0.0, +0.0) with the masses
    (0.75, 1.5, 0.75) 2^40, p = 0.2: H = 0.75 + floor(0.45 2^40) / 2^40, k = 2 is -0.0 with g = (H - 0.75) / 1.5, so q = -1 + g
    (were the zeros tied, the lighter +0.0 would come first and g would be twice that)"""
    for vals in ([0.0, -0.0], [-0.0, 0.0]):
        q, _ = wq(vals, [0.5, 0.5], (0.0, 0.5, 1.0))
        assert (q == 0).all() and not np.signbit(q).any()
    q, _ = wq([-0.0, -1.0], [0.5, 0.5], (1.0,))
    assert q[0] == 0 and np.signbit(q[0])
    for vals, w in (([0.0, -1.0, -0.0], [0.25, 0.25, 0.5]), ([-0.0, 0.0, -1.0], [0.5, 0.25, 0.25])):
        q, r = wq(vals, w, (0.2,))
        g = float(math.floor(0.2 * float(9 << 38))) / float(3 << 39)
        assert r.M == 3 << 40 and 0.29 < g < 0.31 and q[0] == -1.0 + g * (-0.0 - -1.0)


def test_a_positive_weight_without_mass_does_not_count():
    w = np.array([0.5, 2.0 ** -70, 0.25, 0.0, 0.25])
    q, r = wq([3.0, -7.0, 1.0, 9.0, 2.0], w, (0.0, 0.5, 1.0))
    assert r.n_mass == 3 and r.n_pos == 4 and r.n_mass < (w > 0).sum()
    assert q[0] == 1.0 and q[2] == 3.0                      # -7 (weight 2^-70) and 9 (weight 0) are not there
    assert weight_fix([2.0 ** -70], 5) == [0] and weight_fix([2.0 ** -41 / 5], 5)[0] in (0, 1)


def test_all_mass_on_one_position_and_n_mass_one():
    q, r = wq([3.0, 5.0, 1.0], [0.0, 1.0, 0.0], (0.0, 0.3, 1.0))
    assert r.n_mass == 1 and q.tolist() == [5.0, 5.0, 5.0] and r.M == 3 << 40
    q, r = wq([3.0, 5.0, 1.0], [2.0 ** -70, 1.0, 2.0 ** -70], (0.0, 0.3, 1.0))
    assert r.n_mass == 1 and r.n_pos == 3 and q.tolist() == [5.0, 5.0, 5.0]
    q, r = wq([-0.0], [1.0], (0.0, 0.5, 1.0))
    assert r.n_mass == 1 and np.signbit(q).all()
    # nearly all mass on one position among many
    w = np.full(300, 2.0 ** -30)
    w[7] = 1.0 - 299 * 2.0 ** -30
    vals = np.arange(300.0)
    q, r = wq(vals, w, (0.0, 0.5, 1.0))
    assert q[0] == 0.0 and q[2] == 299.0 and 6.0 <= q[1] <= 7.0


def test_p_zero_and_one_are_the_extremes_of_the_counting_values():
    rng = np.random.default_rng(1)
    for N in SHAPES:
        X = rng.standard_normal((N, 3))
        w = rng.random(N) * (rng.random(N) < 0.7)
        w /= w.sum()
        r = summary_reference(X, w, cov=False, wquantiles=(0.0, 1.0))
        live = np.array(weight_fix(w, N)) >= 1
        assert np.array_equal(r.wquantiles[0], X[live].min(axis=0)) and np.array_equal(r.wquantiles[1], X[live].max(axis=0))


def test_no_weight_array_is_one_over_n():
    rng = np.random.default_rng(2)
    X = rng.standard_normal((300, 2))
    a = summary_reference(X, None, cov=False, wquantiles=PROBS27)
    assert a.M == 300 << 40 and a.n_mass == 300
    q, M, n = wquantiles_reference(X, None, PROBS27)
    assert np.array_equal(q, a.wquantiles) and (M, n) == (a.M, a.n_mass)
    col = wquantile_column(X[:, 0], [1 << 40] * 300, PROBS27)
    assert col == a.wquantiles[:, 0].tolist()


def test_refusals():
    X = np.arange(6.0)
    with pytest.raises(ValueError, match="not normalised"):
        summary_reference(X, np.full(6, 1e6), cov=False, wquantiles=(0.5,))
    with pytest.raises(ValueError, match="no particle has a positive weight"):
        summary_reference(X, np.full(6, 2.0 ** -70), cov=False, wquantiles=(0.5,))
    with pytest.raises(ValueError, match="no particle has a positive weight"):
        summary_reference(X, np.zeros(6), cov=False, wquantiles=(0.5,))
    with pytest.raises(ValueError, match=r"p must be in \[0, 1\]"):
        summary_reference(X, None, cov=False, wquantiles=(1.5,))
    # the unweighted quantile keeps its refusal next to it
    with pytest.raises(ValueError, match="weighted quantiles are not provided"):
        summary_reference(X, np.array([.1, .2, .3, .2, .1, .1]), cov=False, quantiles=(0.5,), wquantiles=(0.5,))


def test_summary_options_and_the_record():
    assert summary_options(dict(wquantiles=(0.5,), cov=False)) == dict(wquantiles=(0.5,), cov=False)
    with pytest.raises(ValueError, match="unknown option"):
        summary_options(dict(wquantile=(0.5,)))
    with pytest.raises(ValueError, match="unknown option"):
        summary_options(dict(wquantiles=(0.5,), median=True))
    r = summary_reference(np.arange(6.0), None)                # nothing asked for: the fields are there, empty
    assert r.wquantiles.shape == (0, 1) and r.wprobs == () and r.M is None and r.n_mass is None and r.quantiles.shape == (0, 1)


def test_driver_keyword_reaches_the_reference_engine(oracle):
    import abcdez_amd as A

    r = A.abcdesmc(A.Normal(0, math.sqrt(10)), A.Normal1D(3.0), 0.5, None, nparticles=300, verbose=False, rng=3, ABCk=A.Epa0toϵ,
                   engine=oracle.oracle_engine, summary=dict(cov=False, wquantiles=(0.025, 0.5, 0.975)))
    ref = summary_reference(r.P, r.Wns, cov=False, wquantiles=(0.025, 0.5, 0.975))
    assert np.array_equal(r.summary.wquantiles, ref.wquantiles) and r.summary.M == ref.M and r.summary.n_mass == ref.n_mass
    assert np.unique(r.Wns[r.Wns > 0]).size > 1 and np.all(np.diff(r.summary.wquantiles[:, 0]) > 0)
