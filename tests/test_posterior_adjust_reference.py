"""The regression-adjusted posterior without a GPU (include/abcdez_spec.h, "REGRESSION ADJUSTMENT"): the single solve
(abcdez_amd.summary.adjust_solve) and the apply order against small integer examples worked by hand, a noise-free linear blob that
the adjustment must invert, the law of the adjusted sample in the conjugate normal model, the options and the refusals, and the
drivers' keyword on the CPU test engine, which computes the restatement on its downloaded result."""
import math

import numpy as np
import pytest

import abcdez_amd as A
from abcdez_amd.summary import (adjust_apply, adjust_options, adjust_reference, adjust_solve, summary_reference, tile_tree_sum)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------ worked examples
def test_solve_worked_by_hand():
    """A = [[4, 2], [2, 5]] = L L^T with L = [[2, 0], [1, 2]]; B = A [[1, -1], [2, 3]]: every intermediate is a small integer"""
    A_ = np.array([[4.0, 2.0], [2.0, 5.0]])
    beta = np.array([[1.0, -1.0], [2.0, 3.0]])
    B = A_ @ beta
    assert B.tolist() == [[8.0, 2.0], [12.0, 13.0]]
    got = adjust_solve(A_, B)
    # forward: z_0 = b_0 / 2 = (4, 1), z_1 = (b_1 - 1 z_0) / 2 = (4, 6); back: beta_1 = z_1 / 2 = (2, 3), beta_0 = (z_0 - 1 beta_1) / 2
    assert got.tolist() == beta.tolist()
    # one regressor, one parameter: a division
    assert adjust_solve([[16.0]], [6.0]).tolist() == [[0.375]]          # L = 4: (6 / 4) / 4
    # ridge scales the diagonal only, by one multiplication: [[4 * 1.25, 2], [2, 5 * 1.25]] = [[5, 2], [2, 6.25]]
    r = adjust_solve(A_, B, ridge=0.25)
    L00 = math.sqrt(5.0)
    L10 = 2.0 / L00
    L11 = math.sqrt(6.25 - L10 * L10)
    z0 = B[0] / L00
    z1 = (B[1] - L10 * z0) / L11
    b1 = z1 / L11
    b0 = (z0 - L10 * b1) / L00
    assert np.array_equal(bits(r), bits(np.array([b0, b1])))
    assert np.allclose(np.array([[5.0, 2.0], [2.0, 6.25]]) @ r, B, rtol=1e-14)


def test_apply_order_worked_by_hand():
    """acc = ((0 + b_0 (s_0 - t_0)) + b_1 (s_1 - t_1)) + b_2 (s_2 - t_2), then y = x - acc: with 2^53 in the middle term the
    ascending order loses the first term and keeps the last; any other order gives another result"""
    big = 2.0 ** 53
    X = np.array([[10.0], [7.0], [np.nan]])
    Bm = np.array([[1.0, big, -big + 1.0], [3.0, 2.0, 1.0], [np.nan, np.nan, np.nan]])
    live = np.array([True, True, False])
    t = np.array([0.0, 0.0, 1.0])
    beta = np.array([[1.0], [1.0], [1.0]])
    Y = adjust_apply(X, Bm, live, t, beta)
    # row 0: (0 + 1) + 2^53 = 2^53 (the 1 is lost), + (-2^53 + 1 - 1) = 0 -> y = 10; row 1: 3 + 2 + 0 = 5 -> y = 2; row 2: +0.0
    assert Y.tolist() == [[10.0], [2.0], [0.0]] and not np.signbit(Y[2, 0])
    assert (1.0 + (big + (-big))) == 1.0        # what a descending order would have subtracted instead
    # two parameters, integer coefficients
    Y2 = adjust_apply(np.array([[1.0, 2.0]]), np.array([[3.0, 5.0]]), np.array([True]), np.array([1.0, 1.0]),
                      np.array([[2.0, -1.0], [0.5, 4.0]]))
    assert Y2.tolist() == [[1.0 - (2.0 * 2.0 + 0.5 * 4.0), 2.0 - (-1.0 * 2.0 + 4.0 * 4.0)]]


def test_reference_worked_by_hand():
    """four particles, one dead and poisoned; s = 2 x exactly, dyadic weights: every sum is exact"""
    P = np.array([-1.0, np.nan, 3.0, 7.0])
    Bl = np.array([-2.0, np.nan, 6.0, 14.0])
    w = np.array([0.125, 0.0, 0.75, 0.125])
    r = adjust_reference(P, Bl, w, target=[4.0], rows=True, corrected=False)
    # means 3 and 6; S_ss = .125 64 + 0 + .125 64 = 16 (L = 4), S_sx = .125 32 + .125 32 = 8 -> beta = (8 / 4) / 4; y = x - 0.5 (2 x - 4) = 2
    assert r.x_mean.tolist() == [3.0] and r.s_mean.tolist() == [6.0] and r.S_sx.tolist() == [[8.0]] and r.beta.tolist() == [[0.5]]
    assert r.P.tolist() == [[2.0], [0.0], [2.0], [2.0]] and r.mean.tolist() == [2.0] and r.S.tolist() == [[0.0]]
    assert r.columns == (0,) and r.target.tolist() == [4.0] and r.ridge == 0.0 and r.n_pos == 3 and r.W == 1.0
    assert r.quantiles.shape == (0, 1) and r.hist is None and r.M is None


# ------------------------------------------------------------------------------------------ noise-free linear blob
@pytest.mark.parametrize("c", [1, 2, 4])
def test_a_noise_free_linear_blob_is_inverted(c):
    """s_k = a_k x_k + b_k, c = d: beta is diag(1 / a), and every adjusted row is (t - b) / a"""
    rng = np.random.default_rng(7 + c)
    N = 3000
    X = rng.standard_normal((N, c)) * np.array([1.0, 3.0, 0.5, 2.0])[:c] + np.array([0.5, -2.0, 4.0, 1.0])[:c]
    a = np.array([2.0, -0.5, 4.0, 1.5])[:c]
    b = np.array([1.0, 0.25, -3.0, 2.0])[:c]
    Bl = a * X + b
    w = rng.random(N)
    w[rng.random(N) < 0.2] = 0.0
    w /= w.sum()
    t = np.array([0.75, -1.0, 2.0, 0.5])[:c]
    r = adjust_reference(X, Bl, w, target=t, rows=True)
    assert np.allclose(r.beta, np.diag(1.0 / a), rtol=0, atol=1e-12)
    want = (t - b) / a
    xmax = np.abs(X[w > 0]).max()
    ulp = np.spacing(xmax)
    err = np.abs(r.P[w > 0] - want).max()
    print("c", c, "largest error", err / ulp, "ulp of |x|max")
    assert err <= 64 * ulp
    assert (r.P[w == 0] == 0).all()
    assert np.abs(r.mean - want).max() <= 64 * ulp


# ------------------------------------------------------------------------------------------ the law
SIGMA0, SIGMA, TARGET = 2.0, 1.0, 1.5
EPS = 2.0                      # two sigma each side: about half of the prior predictive mass is accepted; chosen on the CPU so
                               # that the raw mean of the accepted sample misses the posterior mean by about 30 standard errors
POST_MEAN = TARGET * SIGMA0 ** 2 / (SIGMA0 ** 2 + SIGMA ** 2)          # 1.2
POST_VAR = SIGMA0 ** 2 * SIGMA ** 2 / (SIGMA0 ** 2 + SIGMA ** 2)       # 0.8


def check_law(adj, raw_mean, what):
    """the adjusted weighted mean within 5 standard errors sqrt(post. var / n_pos) of the posterior mean, the adjusted variance
    within 5 of its own standard errors var sqrt(2 / (n_pos - 1)) of the posterior variance, the raw mean outside"""
    n = adj.n_pos
    se = math.sqrt(POST_VAR / n)
    se_var = POST_VAR * math.sqrt(2.0 / (n - 1))
    print(what, "n_pos", n, "adjusted mean", adj.mean[0], "raw mean", raw_mean, "se", se, "adjusted var", adj.cov[0, 0], "se", se_var)
    assert abs(adj.mean[0] - POST_MEAN) <= 5 * se, what
    assert abs(adj.cov[0, 0] - POST_VAR) <= 5 * se_var, what
    assert abs(raw_mean - POST_MEAN) > 5 * se, what


def test_the_adjusted_sample_has_the_posterior_law():
    """theta ~ N(0, sigma0^2), s = theta + N(0, sigma^2), accepted iff |s - t| <= eps.  Selection on s does not bias the regression
    of theta on s, so theta - beta (s - t) has the posterior's mean and variance although eps is several sigma wide"""
    rng = np.random.default_rng(20021)
    N = 20000
    th = rng.normal(0.0, SIGMA0, N)
    s = th + rng.normal(0.0, SIGMA, N)
    w = (np.abs(s - TARGET) <= EPS).astype(np.float64)
    w /= w.sum()
    adj = adjust_reference(th, s, w, target=[TARGET])
    raw = summary_reference(th, w)
    assert abs(adj.beta[0, 0] - SIGMA0 ** 2 / (SIGMA0 ** 2 + SIGMA ** 2)) < 0.03
    check_law(adj, raw.mean[0], "numpy")
    assert np.array_equal(bits(adj.x_mean), bits(raw.mean))


def test_the_law_through_the_driver_on_the_cpu_engine(oracle):
    r = A.abcdesmc(A.Normal(0.0, SIGMA0), A.Normal1D(TARGET, SIGMA, blobs=True), EPS, None, nparticles=4000, verbose=False, rng=11,
                   engine=oracle.oracle_engine, adjust=True, summary=True)
    assert r.blobs.shape == (4000,) and r.eps <= EPS
    check_law(r.adjusted, r.summary.mean[0], "abcdesmc")
    ref = adjust_reference(r.P, r.blobs, r.Wns, target=[TARGET])          # the default target is the simulator's data
    for f in ("mean", "S", "cov", "beta", "S_sx", "s_mean", "x_mean", "target"):
        assert np.array_equal(bits(getattr(r.adjusted, f)), bits(getattr(ref, f))), f
    assert r.adjusted.columns == (0,) and r.adjusted.P is None and r.adjusted.n_pos == ref.n_pos
    # download=False goes with it, and the engine call takes the other options
    kw = dict(nparticles=500, verbose=False, rng=11, engine=oracle.oracle_engine)
    bare = A.abcdesmc(A.Normal(0.0, SIGMA0), A.Normal1D(TARGET, SIGMA, blobs=True), EPS, None, download=False,
                      adjust=dict(wquantiles=(0.025, 0.975), rows=True, ridge=0.5, hist=dict(bins=4)), **kw)
    assert bare.P is None and bare.blobs is None and bare.adjusted.P.shape == (500, 1) and bare.adjusted.ridge == 0.5
    assert bare.adjusted.wquantiles.shape == (2, 1) and bare.adjusted.hist.mass1.shape == (1, 4)
    full = bare.engine.result()
    ref = adjust_reference(full["P"], full["blobs"], full["Wns"], target=[TARGET], wquantiles=(0.025, 0.975), rows=True, ridge=0.5)
    for f in ("mean", "beta", "P", "wquantiles"):
        assert np.array_equal(bits(getattr(bare.adjusted, f)), bits(getattr(ref, f))), f
    assert not hasattr(A.abcdesmc(A.Normal(0.0, SIGMA0), A.Normal1D(TARGET, SIGMA, blobs=True), EPS, None, **kw), "adjusted")
    # abcdemc: unit weights
    m = A.abcdemc(A.Normal(0.0, SIGMA0), A.Normal1D(TARGET, SIGMA, blobs=True), EPS, None, nparticles=300, generations=10, verbose=False,
                  rng=3, engine=oracle.oracle_engine, adjust=dict(rows=True))
    ref = adjust_reference(m.P, m.blobs, None, target=[TARGET], rows=True)
    assert m.adjusted.n_pos == 300 and m.adjusted.W == 300.0
    for f in ("mean", "beta", "P", "S"):
        assert np.array_equal(bits(getattr(m.adjusted, f)), bits(getattr(ref, f))), f


# ------------------------------------------------------------------------------------------ options and refusals
def crafted(N=500, d=2, nb=5, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, d))
    Bl = X @ rng.standard_normal((d, nb)) + 0.3 * rng.standard_normal((N, nb))
    w = rng.random(N)
    w[rng.random(N) < 0.25] = 0.0
    return X, Bl, w / w.sum(), rng.standard_normal(nb)


def test_options_accepts_and_refuses():
    assert adjust_options(True) == {}
    opts = dict(columns=(0, 2), target=(1.0, 2.0), ridge=0.1, cov=False, corrected=False, wquantiles=(0.5,), hist=True, rows=True)
    got = adjust_options(opts)
    assert got == opts and got is not opts
    with pytest.raises(ValueError, match=r"adjust: unknown option\(s\) \['quantiles'\]"):
        adjust_options(dict(quantiles=(0.5,)))
    for bad in (None, False, 3, "all"):
        with pytest.raises(ValueError, match="adjust must be None, True or a dict"):
            adjust_options(bad)


def test_columns_subsets_are_slicing_by_hand():
    X, Bl, w, t = crafted()
    cols = [1, 3, 4]
    sub = adjust_reference(X, Bl, w, target=t[cols], columns=cols, rows=True, wquantiles=(0.1, 0.9))
    hand = adjust_reference(X, Bl[:, cols], w, target=t[cols], rows=True, wquantiles=(0.1, 0.9))
    for f in ("mean", "S", "cov", "beta", "S_sx", "s_mean", "x_mean", "P", "wquantiles"):
        assert np.array_equal(bits(getattr(sub, f)), bits(getattr(hand, f))), f
    assert sub.columns == (1, 3, 4) and hand.columns == (0, 1, 2) and sub.beta.shape == (3, 2)
    # the default target: the simulator's data, one number per blob column, restricted to the columns
    dflt = adjust_reference(X, Bl, w, columns=cols, data=tuple(t), rows=True)
    assert np.array_equal(bits(dflt.P), bits(sub.P)) and np.array_equal(dflt.target, t[cols])
    for bad in ([], [3, 1], [1, 1], [-1, 2], [0, 5]):
        with pytest.raises(ValueError, match="adjust: columns must be strictly increasing"):
            adjust_reference(X, Bl, w, target=t[:len(bad)] if bad else t[:1], columns=bad)


def test_ridge_and_collinear_columns():
    X, Bl, w, t = crafted()
    plain = adjust_reference(X, Bl, w, target=t)
    ridged = adjust_reference(X, Bl, w, target=t, ridge=0.5)
    assert ridged.ridge == 0.5 and np.abs(ridged.beta).sum() < np.abs(plain.beta).sum()      # shrunk
    assert np.array_equal(bits(ridged.S_sx), bits(plain.S_sx))
    dup = Bl.copy()
    dup[:, 3] = dup[:, 1]                                    # a duplicated column: the pivot of column 3 vanishes
    with pytest.raises(ValueError, match="adjust: the simulated data are collinear or constant in column 3: pass `ridge` or fewer `columns`"):
        adjust_reference(X, dup, w, target=t)
    assert np.isfinite(adjust_reference(X, dup, w, target=t, ridge=1e-3).beta).all()
    assert np.isfinite(adjust_reference(X, dup, w, target=t[[0, 1, 2, 4]], columns=[0, 1, 2, 4]).beta).all()
    const = Bl.copy()
    const[:, 2] = 4.5
    with pytest.raises(ValueError, match="collinear or constant in column 2"):
        adjust_reference(X, const, w, target=t)
    with pytest.raises(ValueError, match="collinear or constant in column 2"):
        adjust_reference(X, const, w, target=t, ridge=10.0)       # a ridge scales a zero diagonal to zero
    for bad in (-0.1, math.inf, math.nan):
        with pytest.raises(ValueError, match="adjust: ridge must be finite and not negative"):
            adjust_reference(X, Bl, w, target=t, ridge=bad)
    # the threshold: a pivot at 2^-40 of its diagonal is refused, the next larger one is not
    with pytest.raises(ValueError, match="collinear or constant in column 1"):
        adjust_solve([[1.0, 1.0], [1.0, 1.0 + 2.0 ** -40]], [[1.0], [1.0]])
    assert np.isfinite(adjust_solve([[1.0, 1.0], [1.0, 1.0 + 2.0 ** -39]], [[1.0], [1.0]])).all()


def test_nan_rows_targets_and_blobs():
    X, Bl, w, t = crafted()
    clean = adjust_reference(X, Bl, w, target=t, rows=True)
    poisoned_X, poisoned_B = X.copy(), Bl.copy()
    poisoned_X[w == 0] = np.nan
    poisoned_B[w == 0] = np.nan                              # weightless rows are never read
    same = adjust_reference(poisoned_X, poisoned_B, w, target=t, rows=True)
    for f in ("mean", "S", "beta", "S_sx", "P"):
        assert np.array_equal(bits(getattr(same, f)), bits(getattr(clean, f))), f
    assert (same.P[w == 0] == 0).all() and not np.signbit(same.P[w == 0]).any()
    bad = Bl.copy()
    bad[int(np.flatnonzero(w > 0)[5]), 2] = np.nan           # a NaN in a row that counts
    with pytest.raises(ValueError, match="adjust: a moment of the simulated data is not finite"):
        adjust_reference(X, bad, w, target=t)
    assert np.isfinite(adjust_reference(X, bad, w, target=t[[0, 1]], columns=[0, 1]).beta).all()      # ... in a column not chosen
    for wrong in (t[:4], np.append(t, 1.0), 1.0):
        with pytest.raises(ValueError, match="adjust: target must hold 5 number"):
            adjust_reference(X, Bl, w, target=wrong)
    with pytest.raises(ValueError, match="adjust: target is required"):
        adjust_reference(X, Bl, w)
    with pytest.raises(ValueError, match="adjust: target is required"):
        adjust_reference(X, Bl, w, data=(1.0, 2.0))          # a blob such as the residuals has no default
    with pytest.raises(ValueError, match="adjust: the target is not finite"):
        adjust_reference(X, Bl, w, target=np.where(np.arange(5) == 1, np.nan, t))
    with pytest.raises(ValueError, match=r"adjust: needs a simulator that returns blobs \(blobs=True\)"):
        adjust_reference(X, None, w, target=t)
    # S_sx against the definition, column by column
    live = w > 0
    for j in range(5):
        for k in range(2):
            term = np.where(live, w * ((np.where(live, Bl[:, j], 0) - clean.s_mean[j]) * (np.where(live, X[:, k], 0) - clean.x_mean[k])), 0.0)
            assert bits(tile_tree_sum(term)) == bits(clean.S_sx[j, k])


WIEN = tuple(math.sqrt(0.25 * t * t + 4.0 * t) for t in range(8))


def test_refusals_through_the_driver(oracle):
    prior = A.Factored(A.Uniform(-2, 2), A.Uniform(0, 4))
    kw = dict(nparticles=200, verbose=False, rng=9, engine=oracle.oracle_engine, max_iters=2)
    with pytest.raises(ValueError, match=r"adjust: needs a simulator that returns blobs \(blobs=True\)"):
        A.abcdesmc(prior, A.WienerRMS(WIEN), 0.3, None, adjust=True, **kw)
    with pytest.raises(ValueError, match="adjust: unknown option"):
        A.abcdesmc(prior, A.WienerRMS(WIEN, blobs=True), 0.3, None, adjust=dict(bins=3), **kw)
    with pytest.raises(ValueError, match="adjust: target must hold 8 number"):
        A.abcdesmc(prior, A.WienerRMS(WIEN, blobs=True), 0.3, None, adjust=dict(target=(1.0, 2.0)), **kw)
    with pytest.raises(ValueError, match="adjust: p must be in"):
        A.abcdesmc(prior, A.WienerRMS(WIEN, blobs=True), 0.3, None, adjust=dict(wquantiles=(1.5,)), **kw)
    # the first observation of the series is constant (t = 0): the default columns are refused, columns 1 .. 7 work
    with pytest.raises(ValueError, match="collinear or constant in column 0"):
        A.abcdesmc(prior, A.WienerRMS(WIEN, blobs=True), 0.3, None, adjust=True, **kw)
    r = A.abcdesmc(prior, A.WienerRMS(WIEN, blobs=True), 0.3, None, adjust=dict(columns=range(1, 8), ridge=1e-6), **kw)
    assert r.adjusted.beta.shape == (7, 2) and np.array_equal(r.adjusted.target, np.array(WIEN[1:]))
    with pytest.raises(ValueError, match="adjust: target is required"):
        A.abcdesmc(A.Uniform(-2, 2), A.DiracSquare(1.5, blobs=True), 0.3, None, adjust=True, **kw)
