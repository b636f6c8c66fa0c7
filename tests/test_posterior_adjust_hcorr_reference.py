"""Bounded transforms and the heteroscedastic correction of the regression adjustment without a GPU (include/abcdez_spec.h,
"REGRESSION ADJUSTMENT": TRANSFORM, HETEROSCEDASTIC CORRECTION): the literal Python abz_log / abz_exp of abcdez_amd.summary against
the oracle's bit for bit, the options and their refusals, the unchanged record with both options off, the law of the correction and
of the transforms, and the drivers' keyword on the CPU test engine."""
import math

import numpy as np
import pytest

import abcdez_amd as A
from abcdez_amd import summary as S
from abcdez_amd.summary import (adjust_apply, adjust_options, adjust_reference, adjust_solve, adjust_transform, summary_reference,
                                tile_tree_sum)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def oracle_math(O):
    """the pair (log, exp) over float64 arrays by the oracle's orc_math_eval, functions 0 and 1"""
    def fn(which):
        def f(a):
            x = np.ascontiguousarray(a, dtype=np.float64)
            y, y2 = np.zeros_like(x), np.zeros_like(x)
            if x.size:
                O.lib().orc_math_eval(which, x.ctypes.data, y.ctypes.data, y2.ctypes.data, x.size)
            return y
        return f
    return fn(0), fn(1)


# ------------------------------------------------------------------------------------------ the literal log and exp
def test_literal_log_and_exp_are_the_oracles_bit_for_bit(oracle):
    rng = np.random.default_rng(680)
    special = [0.0, -0.0, -1.0, -5e-324, -1e300, math.inf, -math.inf, math.nan, 5e-324, 1e-310, 2.2250738585072009e-308,
               2.2250738585072014e-308, 1.0, 0.5, 2.0, math.sqrt(0.5), math.sqrt(2.0), 1.7976931348623157e308]
    ends = [709.782712893383973096, np.nextafter(709.782712893383973096, 800.0), np.nextafter(709.782712893383973096, 0.0),
            -745.13321910194110842, np.nextafter(-745.13321910194110842, -800.0), np.nextafter(-745.13321910194110842, 0.0),
            -708.4, -744.9, 708.0, 1e-320, -1e-320, 1e-17, -1e-17]
    x_log = np.concatenate([special, ends, rng.uniform(0, 1, 800), np.exp(rng.uniform(-700, 700, 800)), 1 + rng.uniform(-1e-3, 1e-3, 300),
                            rng.uniform(0, 1, 100) * 1e-310])
    x_exp = np.concatenate([special, ends, rng.uniform(-745.2, 709.8, 1200), rng.uniform(-1, 1, 600), rng.uniform(-40, 40, 400)])
    olog, oexp = oracle_math(oracle)
    for name, lit, orc, x in (("log", S.ADJUST_MATH[0], olog, x_log), ("exp", S.ADJUST_MATH[1], oexp, x_exp)):
        a, b = lit(x), orc(x)
        same = bits(a) == bits(b)
        assert same.all(), (name, x[~same][:5], a[~same][:5], b[~same][:5])
    assert S.abz_log(0.0) == -math.inf and math.isnan(S.abz_log(-1.0)) and S.abz_exp(-math.inf) == 0.0 and S.abz_exp(0.0) == 1.0
    assert len(x_log) > 2000 and len(x_exp) > 2000


# ------------------------------------------------------------------------------------------ options and refusals
def crafted(N=700, d=2, c=3, seed=4):
    rng = np.random.default_rng(seed)
    w = rng.random(N) + 0.05
    w[rng.random(N) < 0.3] = 0.0
    w /= w.sum()
    s = rng.uniform(-1, 1, (N, c))
    X = np.exp(0.2 + s @ rng.uniform(0.1, 0.4, (c, d)) + 0.3 * np.exp(0.5 * s[:, :1]) * rng.standard_normal((N, d)))
    return X, s, w, rng.uniform(-0.5, 0.5, c)


def test_options_are_checked_by_name():
    assert set(S.ADJUST_OPTIONS) >= {"hcorr", "transform"}
    assert adjust_options(dict(hcorr=True, transform="log")) == dict(hcorr=True, transform="log")
    assert adjust_transform(None, 3) is None and adjust_transform([None, None], 2) is None
    kind, lo_hi = adjust_transform("log", 3)
    assert kind.tolist() == [1, 1, 1]
    kind, lo_hi = adjust_transform(("logit", 0.0, 2.0), 2)
    assert kind.tolist() == [2, 2] and lo_hi.tolist() == [[0.0, 2.0], [0.0, 2.0]]
    kind, lo_hi = adjust_transform([None, "log", ("logit", -1, 1)], 3)
    assert kind.tolist() == [0, 1, 2] and lo_hi[2].tolist() == [-1.0, 1.0]
    X, s, w, t = crafted()
    for bad in ("sqrt", ["log", "probit"], 3.5, [("logit", 0.0), None], "logit"):
        with pytest.raises(ValueError, match="adjust: transform: "):
            adjust_reference(X, s, w, target=t, transform=bad)
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (0.0, math.inf), (math.nan, 1.0)):
        with pytest.raises(ValueError, match=r'adjust: transform: \("logit", lo, hi\) needs finite bounds with lo < hi'):
            adjust_reference(X, s, w, target=t, transform=("logit", lo, hi))
    for wrong in (["log"], ["log", None, "log"], []):
        with pytest.raises(ValueError, match="adjust: transform must be one entry or a list of 2 entries"):
            adjust_reference(X, s, w, target=t, transform=wrong)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="adjust: hcorr must be False or True"):
            adjust_reference(X, s, w, target=t, hcorr=bad)


def test_rows_outside_a_domain_and_zero_residuals_are_refused_by_name():
    X, s, w, t = crafted()
    fast = (np.log, np.exp)
    live = np.flatnonzero(w > 0)
    for value, tf, k in ((0.0, "log", 1), (-0.5, "log", 0), (0.0, [None, ("logit", 0.0, 50.0)], 1), (50.0, [("logit", 0.0, 50.0), None], 0),
                         (51.0, ("logit", 0.0, 50.0), 1)):
        bad = X.copy()
        bad[live[7], k] = value
        with pytest.raises(ValueError, match=f"adjust: transform: parameter {k} has a value outside the domain"):
            adjust_reference(bad, s, w, target=t, transform=tf, math=fast)
    # a zero count of a discrete parameter
    counts = np.rint(X * 3.0)
    counts[live[3], 0] = 0.0
    with pytest.raises(ValueError, match="adjust: transform: parameter 0 has a value outside the domain of its log transform"):
        adjust_reference(counts, s, w, target=t, transform=["log", None], math=fast)
    # ... but a weightless row may hold anything, NaN and values outside the domain included: never read
    poisoned_X, poisoned_s = X.copy(), s.copy()
    poisoned_X[w == 0] = np.nan
    poisoned_X[np.flatnonzero(w == 0)[:3]] = -4.0
    poisoned_s[w == 0] = np.nan
    opts = dict(target=t, hcorr=True, transform=["log", ("logit", 0.0, 50.0)], rows=True, math=fast)
    clean, same = adjust_reference(X, s, w, **opts), adjust_reference(poisoned_X, poisoned_s, w, **opts)
    for f in ("mean", "S", "beta", "S_sx", "gamma", "S_sz", "z_mean", "P"):
        assert np.array_equal(bits(getattr(same, f)), bits(getattr(clean, f))), f
    assert (same.P[w == 0] == 0).all() and not np.signbit(same.P[w == 0]).any() and np.isfinite(same.P).all()
    # an exactly zero residual: s = 2 x in dyadic numbers (the worked example of tests/test_posterior_adjust_reference.py)
    P = np.array([-1.0, np.nan, 3.0, 7.0])
    Bl = np.array([-2.0, np.nan, 6.0, 14.0])
    wd = np.array([0.125, 0.0, 0.75, 0.125])
    assert adjust_reference(P, Bl, wd, target=[4.0]).beta.tolist() == [[0.5]]
    with pytest.raises(ValueError, match="adjust: hcorr: a residual of parameter 0 is exactly zero"):
        adjust_reference(P, Bl, wd, target=[4.0], hcorr=True)


def plain_record(X, B, w, t, cols, ridge):
    """the adjustment as it was before the two options existed, from its pieces: (beta, S_sx, x_mean, s_mean, Y, summary of Y)"""
    live = w > 0
    wl = np.where(live, w, 0.0)
    mx, ms = summary_reference(X, w, cov=False), summary_reference(B, w, cov=True)
    Cs = np.where(live[:, None], B[:, cols], 0.0) - ms.mean[cols]
    Cx = np.where(live[:, None], X, 0.0) - mx.mean
    S_sx = np.stack([tile_tree_sum(np.where(live[:, None], wl[:, None] * (Cs[:, j:j + 1] * Cx), 0.0)) for j in range(len(cols))])
    beta = adjust_solve(ms.S[np.ix_(cols, cols)], S_sx, ridge, cols)
    Y = adjust_apply(X, B[:, cols], live, t, beta)
    return beta, S_sx, mx.mean, ms.mean[cols], Y, summary_reference(Y, w, cov=True, wquantiles=(0.1, 0.5, 0.9))


def test_with_both_options_off_nothing_changes():
    X, s, w, t = crafted(N=2500)
    X[w == 0] = np.nan
    for cols, ridge in (([0, 1, 2], 0.0), ([0, 2], 0.25)):
        beta, S_sx, xm, sm, Y, rec = plain_record(X, s, w, t[cols], cols, ridge)
        for extra in ({}, dict(hcorr=False, transform=None), dict(transform=[None, None])):
            r = adjust_reference(X, s, w, target=t[cols], columns=cols, ridge=ridge, rows=True, wquantiles=(0.1, 0.5, 0.9), **extra)
            for name, want in (("beta", beta), ("S_sx", S_sx), ("x_mean", xm), ("s_mean", sm), ("P", Y), ("mean", rec.mean), ("S", rec.S),
                               ("cov", rec.cov), ("wquantiles", rec.wquantiles)):
                assert np.array_equal(bits(getattr(r, name)), bits(want)), (name, extra)
            assert r.hcorr is False and r.transform is None and r.gamma is None and r.z_mean is None and r.S_sz is None
            assert (r.W, r.Q, r.n_pos, r.M, r.n_mass) == (rec.W, rec.Q, rec.n_pos, rec.M, rec.n_mass)


# ------------------------------------------------------------------------------------------ the laws
def test_law_of_the_heteroscedastic_correction():
    """s ~ U(-1, 1), theta = 1 + 2 s + exp(s) xi, so log sigma^2(s) = 2 s; t = 0.9, n = 20 000, unit weights.  The corrected sample
    has the spread AT the target, exp(0.9) = 2.4596; the plain one keeps the spread averaged over the whole range of s,
    sqrt(E exp(2 s)) = sqrt(sinh(2) / 2) = 1.3467.  Both within 10 %: se(gamma) ~ 2.22 / (sqrt(n) 0.577) ~ 0.03 (2.22 = the standard
    deviation of log chi^2_1, 0.577 that of s) moves the ratio exp(0.5 gamma 0.9) by under 3 %, and the sampling error of a standard
    deviation at this n is 0.5 %.  Measured with this seed: corrected 2.5014 (+1.70 % of 2.4596, gamma = 2.021), plain
    1.3595 (+0.95 % of 1.3467); the two targets are 45 % apart."""
    rng = np.random.default_rng(20100)
    n = 20000
    s = rng.uniform(-1.0, 1.0, n)
    theta = 1.0 + 2.0 * s + np.exp(s) * rng.standard_normal(n)
    kw = dict(target=[0.9], rows=True, math=(np.log, np.exp))
    corrected = adjust_reference(theta, s, None, hcorr=True, **kw)
    plain = adjust_reference(theta, s, None, hcorr=False, **kw)
    sd_c, sd_p = float(np.std(corrected.P[:, 0])), float(np.std(plain.P[:, 0]))
    want_c, want_p = math.exp(0.9), math.sqrt(math.sinh(2.0) / 2.0)
    print("hcorr", sd_c, sd_c / want_c - 1.0, "plain", sd_p, sd_p / want_p - 1.0, "gamma", corrected.gamma[0, 0])
    assert abs(sd_c / want_c - 1.0) < 0.10, (sd_c, want_c)
    assert abs(sd_p / want_p - 1.0) < 0.10, (sd_p, want_p)
    assert abs(corrected.gamma[0, 0] - 2.0) < 0.15 and abs(corrected.beta[0, 0] - 2.0) < 0.05      # five standard errors of the slope
    assert abs(corrected.mean[0] - 2.8) < 0.1 and abs(plain.mean[0] - 2.8) < 0.1                    # both centre on 1 + 2 t
    assert np.array_equal(bits(corrected.beta), bits(plain.beta)) and corrected.hcorr and plain.gamma is None


def test_law_of_the_transforms():
    """theta = exp(0.2 + 0.5 s + 0.3 xi) is positive; the plain adjustment towards the edge t = -0.95 of the support of s subtracts a
    straight line from a convex relation and sends some particles below zero (checked: this seed gives several).  On the log scale
    the relation IS linear, and the adjusted values are positive by construction; a logit keeps them in its closed interval.  The
    default ``math`` -- the literal abz_log / abz_exp -- is what runs here."""
    rng = np.random.default_rng(1998)
    n = 1500
    s = rng.uniform(-1.0, 1.0, n)
    theta = np.exp(0.2 + 0.5 * s + 0.3 * rng.standard_normal(n))
    plain = adjust_reference(theta, s, None, target=[-0.95], rows=True)
    assert (plain.P <= 0.0).sum() >= 3, (plain.P <= 0.0).sum()
    logged = adjust_reference(theta, s, None, target=[-0.95], rows=True, transform="log")
    assert (logged.P > 0.0).all() and logged.transform == ("log",)
    assert abs(logged.beta[0, 0] - 0.5) < 0.05 and abs(logged.x_mean[0] - 0.2) < 0.05          # beta and x_mean are on the log scale
    assert abs(np.log(logged.P[:, 0]).mean() - (0.2 - 0.475)) < 0.05
    lo, hi = 0.0, float(theta.max()) * 1.01
    for hc in (False, True):
        lg = adjust_reference(theta, s, None, target=[-0.95], rows=True, transform=("logit", lo, hi), hcorr=hc)
        assert ((lg.P >= lo) & (lg.P <= hi)).all() and lg.transform == (("logit", lo, hi),)
    # a far target saturates the back-transform at the closed ends instead of leaving the interval
    far = adjust_reference(theta, s, None, target=[-4000.0], rows=True, transform=("logit", lo, hi), math=(np.log, np.exp))
    assert ((far.P >= lo) & (far.P <= hi)).all() and (far.P == lo).any()


# ------------------------------------------------------------------------------------------ the drivers' keyword
WIEN = tuple(math.sqrt(0.25 * t * t + 4.0 * t) for t in range(8))
LV_OBS = (1.0, 0.5, 1.46, 0.43, 1.77, 0.62, 1.52, 1.13, 0.95, 1.31, 0.66, 1.09)


def same_record(a, b):
    for f in ("mean", "S", "cov", "beta", "S_sx", "x_mean", "s_mean", "gamma", "S_sz", "z_mean", "P", "wquantiles"):
        assert np.array_equal(bits(getattr(a, f)), bits(getattr(b, f))), f
    assert a.transform == b.transform and a.hcorr == b.hcorr and (a.M, a.n_mass, a.n_pos) == (b.M, b.n_mass, b.n_pos)


def test_the_keyword_through_the_oracle_engine(oracle):
    kw = dict(nparticles=200, verbose=False, rng=9, engine=oracle.oracle_engine, max_iters=2)
    opts = dict(columns=[1, 4, 7], ridge=1e-3, hcorr=True, transform=[("logit", -2.0, 2.0), ("logit", 0.0, 4.0)], rows=True,
                wquantiles=(0.1, 0.9))
    r = A.abcdesmc(A.Factored(A.Uniform(-2, 2), A.Uniform(0, 4)), A.WienerRMS(WIEN, blobs=True), 0.3, None, adjust=opts, **kw)
    ref = adjust_reference(r.P, r.blobs, r.Wns, data=WIEN, **opts)
    same_record(r.adjusted, ref)
    assert r.adjusted.hcorr and r.adjusted.gamma.shape == (3, 2) and ((r.adjusted.P >= [-2.0, 0.0]) & (r.adjusted.P <= [2.0, 4.0])).all()
    lv = A.LotkaVolterraRK4(LV_OBS, dt=0.05, steps_per_obs=10, blobs=True)
    opts = dict(ridge=1e-3, hcorr=True, transform="log", rows=True)
    m = A.abcdemc(A.Factored(*[A.Uniform(0.0, 2.0)] * 4), lv, 5.0, None, nparticles=150, generations=3, verbose=False, rng=8,
                  engine=oracle.oracle_engine, adjust=opts)
    same_record(m.adjusted, adjust_reference(m.P, m.blobs, None, data=LV_OBS, **opts))
    assert (m.adjusted.P >= 0.0).all() and m.adjusted.transform == ("log",) * 4
    with pytest.raises(ValueError, match="adjust: transform must be one entry or a list of 2 entries"):
        A.abcdesmc(A.Factored(A.Uniform(-2, 2), A.Uniform(0, 4)), A.WienerRMS(WIEN, blobs=True), 0.3, None,
                   adjust=dict(columns=[1, 4, 7], transform=["log"]), **kw)
