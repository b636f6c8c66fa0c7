"""Posterior summaries, the parts that need no GPU: the numpy restatement of the summary arithmetic
(abcdez_amd/summary.py; include/abcdez_spec.h, "posterior summaries") against the CPU oracle's tile tree and against numpy's own
weighted mean / covariance / quantile, and the drivers' ``summary`` / ``download`` keywords through the oracle engine."""
import math
from fractions import Fraction

import numpy as np
import pytest

import abcdez_amd as A
from abcdez_amd import summary as S
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


def yardstick_population():
    """(X, w) for the exact-arithmetic yardstick: N = 5001 (three tiles, the last ragged), d = 2, about 30 % of the positions dead,
    unequal weights; column 0 = 1e8 + 1e-3 normal -- a one-pass sum(w x^2) - W mean^2 loses every digit of its variance (1e-6
    against terms of 1e16), and so does a centring by a mean that is off by more than its own rounding -- column 1 = a standard
    normal.  The dead rows are left finite here; the callers overwrite them."""
    rng = np.random.default_rng(20260)
    N = 5001
    X = np.stack([1e8 + 1e-3 * rng.standard_normal(N), rng.standard_normal(N)], axis=1)
    w = rng.random(N)
    w[rng.random(N) < 0.3] = 0.0
    return X, w


def exact_yardstick(X, w, s):
    """The record ``s`` (mean, S, W of :func:`summary_reference` or of the device) against exact rational arithmetic on the
    rows X and weights w.  Returns [(what, |error|, bound)] with error and bound as exact Fractions.

    The bounds are derived (first order in u = 2^-53, the +6 / +2 left over paying for every higher-order term), not measured.
    L = 11 + ceil(log2(#tiles)) is the number of additions a term passes through on its way to the root of the tile tree: 3 inside
    a slot's eight terms, 8 over the 256 slots of a tile, and the same pairing over the tile partials above.  A sum of n terms
    along a tree of depth L has an error of at most L u sum|term| (every addition rounds a partial sum whose magnitude is at most
    sum|term| of its leaves, and a leaf lies under L additions).
      mean_k = fl(T(fl(w x_k)) / T(w)).  Numerator: one rounding per product + the tree, (L + 1) u sum|w x_k|.  Denominator: the
        weights are exact and positive, L u W.  Carried through the quotient, plus the division's own rounding u |mean_k|, and with
        |mean_k| W <= sum|w x_k|:  |mean_k - exact| <= ((L + 1) + L + 1) u sum|w x_k| / W = (2 L + 2) u ...  <= (2 L + 6) u sum|w x_k| / W.
      S_jk = T(fl(w fl(fl(x_j - m_j) fl(x_k - m_k)))) with m the COMPUTED mean taken as exact rationals (the statistic is defined
        around the mean the call returns): two subtractions, two products, 4 u relative per term, + L u for the tree:
        |S_jk - exact| <= (L + 4) u sum|w c_j c_k| <= (L + 6) u sum|w c_j c_k|,  c = x - m exactly.
    (No product here comes near the subnormal range, where a rounding is no longer relative.)"""
    F = Fraction
    X = np.asarray(X, dtype=np.float64)
    N, d = X.shape
    live = np.flatnonzero(np.asarray(w) > 0.0)
    L = 11 + math.ceil(math.log2(-(-N // 2048))) if N > 2048 else 11
    u = F(1, 2 ** 53)
    wl = [F(float(w[i])) for i in live]
    xl = [[F(float(X[i, k])) for i in live] for k in range(d)]
    W = sum(wl)
    out = [("W", abs(F(float(s.W)) - W), L * u * W)]
    for k in range(d):
        exact = sum(a * b for a, b in zip(wl, xl[k])) / W
        out.append((f"mean[{k}]", abs(F(float(s.mean[k])) - exact), (2 * L + 6) * u * sum(abs(a * b) for a, b in zip(wl, xl[k])) / W))
    m = [F(float(v)) for v in s.mean]
    c = [[x - m[k] for x in xl[k]] for k in range(d)]
    for j in range(d):
        for k in range(j, d):
            terms = [a * cj * ck for a, cj, ck in zip(wl, c[j], c[k])]
            out.append((f"S[{j},{k}]", abs(F(float(s.S[j, k])) - sum(terms)), (L + 6) * u * sum(abs(t) for t in terms)))
    return out


def test_reference_meets_derived_bounds_against_exact_arithmetic():
    """the centred two-pass second moment of the restatement against Fractions, on an input a one-pass formula cannot survive"""
    X, w = yardstick_population()
    live = w > 0.0
    assert 0.25 < 1.0 - live.mean() < 0.35 and np.unique(w[live]).size > 3000
    Xn = X.copy()
    Xn[~live] = np.nan
    s = summary_reference(Xn, w)
    worst = 0.0
    for what, err, bound in exact_yardstick(X, w, s):
        print(what, float(err), float(bound), float(err / bound))
        assert err <= bound, what
        worst = max(worst, float(err / bound))
    print("worst error / bound", worst)
    # the input has teeth: the one-pass variance of column 0, in the same double arithmetic, misses the same bound by far
    x0, wl = X[live, 0], w[live]
    one_pass = math.fsum(wl * x0 * x0) - s.W * s.mean[0] * s.mean[0]
    m0 = Fraction(float(s.mean[0]))
    terms = [Fraction(float(a)) * (Fraction(float(b)) - m0) ** 2 for a, b in zip(wl, x0)]
    assert abs(Fraction(one_pass) - sum(terms)) > 10 ** 6 * (13 + 6) * Fraction(1, 2 ** 53) * sum(terms)
    assert np.array_equal(s.S, s.S.T)


def test_reference_with_a_single_positive_weight():
    """n_pos = 1, the live position the last of a ragged tile: the mean is the row, S is identically zero (the centred row is
    zero), the corrected denominator W - Q / W is 0 and cov = 0 / 0, and every quantile equals the row.
    A -0.0 component comes out as +0.0, in the mean (-0.0 plus the +0.0 terms of the other positions) and in the quantile: the
    order statistic is -0.0, but the type-7 formula of the spec, v_j + g (v_j+1 - v_j) with v_j+1 = v_j, is -0.0 + g * (+0.0) =
    +0.0 in IEEE arithmetic for every g >= 0 -- as in Julia's quantile, whose formula this is (smc:301).  Pinned here so that the
    device, which is compared with this restatement bit for bit, cannot drift either way."""
    N = 4099
    row = np.array([1.5, -0.0, -2.25e-300])
    X = np.full((N, 3), np.nan)
    X[1::2] = np.inf
    X[2::3] = -np.inf
    X[N - 1] = row
    w = np.zeros(N)
    w[N - 1] = 1.0
    with np.errstate(invalid="ignore"):
        s = summary_reference(X, w, quantiles=(0.0, 0.3, 0.5, 1.0))
    assert s.n_pos == 1 and s.W == 1.0 and s.Q == 1.0 and s.ess == 1.0
    assert np.array_equal(s.mean, row) and not np.signbit(s.mean[1])                # +0.0 terms of the dead positions: -0.0 + 0.0
    assert np.array_equal(s.S, np.zeros((3, 3))) and np.isnan(s.cov).all()
    assert s.quantiles.shape == (4, 3)
    for i in range(4):
        assert np.array_equal(s.quantiles[i], row)
        assert s.quantiles[i, [0, 2]].tobytes() == row[[0, 2]].tobytes() and not np.signbit(s.quantiles[i, 1])
    unc = summary_reference(X, w, corrected=False)
    assert np.array_equal(unc.cov, np.zeros((3, 3)))


def test_reference_with_two_positive_weights_in_different_tiles():
    """n_pos = 2 at positions 0 and 2048; values on which every operation is exact, so the results are asserted directly"""
    N = 4099
    X = np.full((N, 2), np.nan)
    X[1:2048] = np.inf
    X[0] = (1.0, -4.0)
    X[2048] = (3.0, 8.0)
    w = np.zeros(N)
    w[[0, 2048]] = 0.5
    s = summary_reference(X, w, quantiles=(0.0, 0.3, 0.5, 1.0))
    assert s.n_pos == 2 and s.W == 1.0 and s.Q == 0.5 and s.ess == 2.0
    assert list(s.mean) == [2.0, 2.0]
    assert s.S.tolist() == [[1.0, 6.0], [6.0, 36.0]]                               # 0.5 ((-1)(-1) + 1 1), 0.5 ((-1)(-6) + 1 6), ...
    assert s.cov.tolist() == [[2.0, 12.0], [12.0, 72.0]]                           # / (W - Q / W) = 0.5: the n - 1 estimator
    g = (0.3 + 1.0) - 1.0                                                          # h = (n - 1) p + 1, j = 1, g = h - 1: not 0.3
    assert s.quantiles[:, 0].tolist() == [1.0, 1.0 + g * 2.0, 2.0, 3.0]            # v1 + g (v2 - v1)
    assert s.quantiles[:, 1].tolist() == [-4.0, -4.0 + g * 12.0, 2.0, 8.0]


def test_reference_never_reads_a_dead_row_or_a_weight_that_does_not_count():
    """NaN / +-inf in the rows of dead positions, and weights of -0.0, -1.0, NaN and +0.0 between live ones: the result is that
    of the live rows alone"""
    rng = np.random.default_rng(77)
    N = 2 * 2048 + 77
    X = rng.standard_normal((N, 3))
    w = np.full(N, 1.0 / N)
    dead = rng.permutation(N)[:N // 2]
    w[dead] = np.resize(np.array([-0.0, -1.0, np.nan, 0.0]), dead.size)
    clean = summary_reference(np.where((w > 0)[:, None], X, 0.0), np.where(w > 0, w, 0.0), quantiles=PROBS)
    X[dead] = np.resize(np.array([np.nan, np.inf, -np.inf]), (dead.size, 3))
    s = summary_reference(X, w, quantiles=PROBS)
    assert s.n_pos == N - N // 2 == clean.n_pos and s.W == clean.W and s.Q == clean.Q
    for f in ("mean", "S", "cov", "quantiles"):
        assert np.isfinite(getattr(s, f)).all() and getattr(s, f).tobytes() == getattr(clean, f).tobytes(), f
    live = w > 0
    assert abs(s.mean[0] - X[live, 0].mean()) <= 64 * U * np.abs(X[live, 0]).mean()
    assert s.quantiles[0, 1] == X[live, 1].min() and s.quantiles[-1, 1] == X[live, 1].max()


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


# ------------------------------------------------------------------------------------------ refusals, character for character
def bare_ops(d=3):
    """a HipOps that never loaded the library: enough for the checks the bindings make on the host before they call it"""
    from types import SimpleNamespace

    from abcdez_amd.engine import HipOps

    ops = object.__new__(HipOps)
    ops.spec = SimpleNamespace(d=d)
    return ops


def blob_engine(oracle, n=16):
    spec = A.ModelSpec(A.Normal(0.0, 2.0), A.Normal1D(1.5, 1.0, blobs=True), A.Epa0toeps, seed=3)
    return oracle.oracle_engine(spec, n)


def f64(*shape):
    import torch

    return torch.zeros(shape, dtype=torch.float64)


def rerun_with_another_distance(oracle):
    eng = blob_engine(oracle)
    eng.init_population()
    eng.reset_weights()
    honest = eng.ops.blob_eval

    def blob_eval(theta, stamp, blob, delta_out):
        honest(theta, stamp, blob, delta_out)
        delta_out[3] += 1.0
    eng.ops.blob_eval = blob_eval
    eng.result()


def fake_engine_sample(oracle):
    from types import SimpleNamespace

    res = dict(P=np.arange(4.0), C=np.zeros(4), Wns=np.full(4, 0.25), blobs=None)
    S.engine_sample(SimpleNamespace(result=lambda: res, spec=SimpleNamespace(seed=1)), 2, blobs=True)


REFUSALS = {
    "summary option": (lambda o: S.summary_options(dict(bins=1, median=True)), ValueError,
                       "summary: unknown option(s) ['bins', 'median'] (cov, corrected, quantiles, wquantiles, hist)"),
    "summary type": (lambda o: S.summary_options(3), ValueError,
                     "summary must be None, True or a dict of the options cov, corrected, quantiles, wquantiles, hist"),
    "predictive option": (lambda o: S.predictive_options(dict(quantiles=(0.5,))), ValueError,
                          "predictive: unknown option(s) ['quantiles'] (cov, corrected, wquantiles, hist)"),
    "predictive type": (lambda o: S.predictive_options(False), ValueError,
                        "predictive must be None, True or a dict of the options cov, corrected, wquantiles, hist"),
    "adjust option": (lambda o: S.adjust_options(dict(quantiles=(0.5,), bins=2)), ValueError,
                      "adjust: unknown option(s) ['bins', 'quantiles'] (columns, target, ridge, cov, corrected, wquantiles, hist, rows)"),
    "adjust type": (lambda o: S.adjust_options("all"), ValueError,
                    "adjust must be None, True or a dict of the options columns, target, ridge, cov, corrected, wquantiles, hist, rows"),
    "sample type": (lambda o: S.sample_options(True), ValueError,
                    "sample must be None, an integer n or a dict of the options n, draw, blobs"),
    "summary p": (lambda o: blob_engine(o).posterior_summary(quantiles=(0.5,), wquantiles=(1.5,)), ValueError, "summary: p must be in [0, 1]"),
    "summary p, unweighted": (lambda o: blob_engine(o).posterior_summary(quantiles=(-0.5,)), ValueError, "summary: p must be in [0, 1]"),
    "predictive p": (lambda o: blob_engine(o).posterior_predictive(wquantiles=(0.5, math.nan)), ValueError,
                     "predictive: p must be in [0, 1]"),
    "adjust p": (lambda o: blob_engine(o).posterior_adjusted(wquantiles=(2.0,)), ValueError, "adjust: p must be in [0, 1]"),
    "posterior range": (lambda o: bare_ops().posterior_histograms(None, None, None, None, 5, range=[0.0, 1.0]), ValueError,
                        "posterior_histograms: range must hold (lo, hi) per requested column"),
    "columns range": (lambda o: bare_ops().columns_histograms(f64(5, 4), None, m=3, columns=[0, 2], range=[0.0, 1.0]), ValueError,
                      "columns_histograms: range must hold (lo, hi) per requested column"),
    "columns view": (lambda o: bare_ops()._columns_view(f64(5, 4).float(), None), ValueError,
                     "columns: X must be a contiguous float64 matrix N x ldx"),
    "columns view, through a call": (lambda o: bare_ops().columns_moments(f64(5, 4)[:, :2], None), ValueError,
                                     "columns: X must be a contiguous float64 matrix N x ldx"),
    "adjust blobs": (lambda o: bare_ops()._adjust_blobs(f64(5), None), ValueError, "adjust: Sb must be a contiguous float64 matrix N x lds"),
    "adjust cross means": (lambda o: bare_ops().adjust_cross(None, None, None, None, 5, f64(5, 2), None, [0.0], [0.0] * 3), ValueError,
                           "adjust: s_mean must hold one mean per chosen column and x_mean one per parameter"),
    "adjust apply target": (lambda o: bare_ops().adjust_apply(None, None, None, None, 5, f64(5, 2), [1], [0.0], np.zeros((2, 3))), ValueError,
                            "adjust: target must hold one number per chosen column and beta be c x d"),
    "adjust apply Y": (lambda o: bare_ops().adjust_apply(None, None, None, None, 5, f64(5, 2), [1], [0.0], np.zeros((1, 3)), Y=f64(4, 3)),
                       ValueError, "adjust: Y must be a contiguous float64 matrix N x ldy"),
    "blob re-run": (rerun_with_another_distance, RuntimeError, "blobs: a re-run simulation does not reproduce the stored distance"),
    "sample blobs": (fake_engine_sample, ValueError, "sample: blobs=True needs a simulator that returns blobs"),
    "predictive matrix": (lambda o: S.predictive_reference(np.zeros((2, 2, 2))), ValueError,
                          "predictive: blobs must be one row of numbers per particle"),
    "adjust matrices": (lambda o: S.adjust_reference(np.zeros((3, 2)), np.zeros(4)), ValueError,
                        "adjust: P and blobs must hold one row per particle"),
    "summary weights": (lambda o: S.summary_reference(np.zeros(3), np.zeros(4)), ValueError, "summary: one weight per particle expected"),
    "empty result": (lambda o: A.abcdesmc(PRIOR, SIM, 0.3, None, download=False, summary=False, engine=o.oracle_engine), ValueError,
                     "download=False needs summary: the result would be empty"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusal_strings_of_the_posterior_calls(oracle, name):
    """the text of every refusal the host side of the posterior calls makes itself, as it stood before that code was shared"""
    call, kind, text = REFUSALS[name]
    with pytest.raises(kind) as e:
        call(oracle)
    assert type(e.value) is kind and str(e.value) == text


def test_driver_keywords_are_checked_in_the_order_sample_predictive_adjust_summary(oracle):
    bad = dict(sample=True, predictive=3, adjust="all", summary=3)
    for first, prefix in (("sample", "sample must be"), ("predictive", "predictive must be"), ("adjust", "adjust must be"),
                          ("summary", "summary must be")):
        for run in (lambda **k: A.abcdesmc(PRIOR, SIM, 0.3, None, engine=oracle.oracle_engine, **k),
                    lambda **k: A.abcdemc(PRIOR, SIM, 0.3, None, engine=oracle.oracle_engine, **k)):
            with pytest.raises(ValueError) as e:
                run(**bad)
            assert str(e.value).startswith(prefix), (first, str(e.value))
        del bad[first]


def test_an_engine_object_without_the_posterior_calls_gets_the_restatements():
    """the fallback of summary.engine_summary / _sample / _predictive / _adjusted: anything with result() and spec"""
    from types import SimpleNamespace

    rng = np.random.default_rng(4)
    N = 300
    P, B = rng.standard_normal((N, 2)), rng.standard_normal((N, 3))
    w = rng.random(N) * (rng.random(N) > 0.2)
    w /= w.sum()
    res = dict(P=P, C=rng.random(N), Wns=w, blobs=B)
    eng = SimpleNamespace(result=lambda: res, spec=SimpleNamespace(seed=7, sim=SimpleNamespace(data=lambda: (0.5, 0.0, -0.5))))
    opts = dict(cov=True, wquantiles=(0.1, 0.9), hist=dict(bins=7))
    for got, want in ((S.engine_summary(eng, **opts), S.summary_reference(P, w, **opts)),
                      (S.engine_predictive(eng, **opts), S.predictive_reference(B, w, **opts)),
                      (S.engine_adjusted(eng, **opts), S.adjust_reference(P, B, w, target=(0.5, 0.0, -0.5), **opts))):
        for f in ("mean", "S", "cov", "wquantiles"):
            assert getattr(got, f).tobytes() == getattr(want, f).tobytes(), f
        assert (got.W, got.Q, got.n_pos, got.M, got.n_mass) == (want.W, want.Q, want.n_pos, want.M, want.n_mass)
        assert np.array_equal(got.hist.mass1, want.hist.mass1)
    s = S.engine_sample(eng, 11, draw=2)
    index, M, n_mass = S.sample_reference(P, w, 11, 7, 2)
    assert np.array_equal(s.index, index) and (s.M, s.n_mass, s.n, s.draw) == (M, n_mass, 11, 2)
    assert np.array_equal(s.P, P[index]) and np.array_equal(s.C, res["C"][index]) and np.array_equal(s.blobs, B[index])
    assert S.engine_sample(eng, 11, blobs=False).blobs is None
    res["blobs"] = None
    with pytest.raises(ValueError, match=r"predictive: needs a simulator that returns blobs \(blobs=True\)"):
        S.engine_predictive(eng)
    with pytest.raises(ValueError, match=r"adjust: needs a simulator that returns blobs \(blobs=True\)"):
        S.engine_adjusted(eng)
