"""The regression-adjusted posterior on the device (csrc/abz_adjust.hip: abcdez_adjust_cross / abcdez_adjust_apply,
PopulationEngine.posterior_adjusted) against abcdez_amd.summary.adjust_reference of data that reached the host through the existing
routes -- BIT FOR BIT: float64 fields as uint64 (beta, S_sx and the adjusted rows P included), integer fields exactly.  Crafted
populations and blob matrices go to the C entry points as plain device pointers (the technique of
tests/test_gpu_posterior_summary_edges.py and tests/test_gpu_posterior_predictive.py): the rows of weightless positions of BOTH
inputs and the padding columns of the blob matrix hold NaN, so that one missing guard in a kernel poisons a sum or a row."""
import math

import numpy as np
import pytest
import torch

import abcdez_amd as A
from abcdez_amd import _lib
from abcdez_amd.engine import HipOps, PopulationEngine
from abcdez_amd.summary import (adjust_apply, adjust_reference, adjust_solve, make_adjusted, make_hist, make_summary, hist_options,
                                summary_reference, tile_tree_sum)
from test_gpu_posterior_summary_edges import synthetic

pytestmark = pytest.mark.gpu

PROBS = (0.0, 0.025, 0.5, 0.975, 1.0)
FIELDS = ("mean", "beta", "S_sx", "s_mean", "x_mean", "target", "wquantiles")
ABCKS = {"indicator_strict": A.IndicatorStrict0toeps, "indicator": A.Indicator0toeps, "epa_strict": A.EpaStrict0toeps,
         "epa": A.Epa0toeps}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_adjusted(dev, ref, what):
    assert dev.n_pos == ref.n_pos and (dev.M, dev.n_mass) == (ref.M, ref.n_mass) and dev.columns == ref.columns, what
    assert dev.ridge == ref.ridge and dev.wprobs == ref.wprobs and dev.quantiles.shape == ref.quantiles.shape, what
    for f in ("W", "Q", "ess"):
        assert bits(getattr(dev, f)) == bits(getattr(ref, f)), (what, f)
    for f in FIELDS:
        a, b = getattr(dev, f), getattr(ref, f)
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), (what, f, a, b)
    assert (dev.S is None) == (ref.S is None) and (dev.P is None) == (ref.P is None), what
    if ref.S is not None:
        assert np.array_equal(bits(dev.S), bits(ref.S)) and np.array_equal(bits(dev.cov), bits(ref.cov)), (what, "S")
    if ref.P is not None:
        assert dev.P.shape == ref.P.shape and np.array_equal(bits(dev.P), bits(ref.P)), (what, "P", np.nanmax(np.abs(dev.P - ref.P)))
    assert (dev.hist is None) == (ref.hist is None), what
    if ref.hist is not None:
        a, b = dev.hist, ref.hist
        assert a.columns == b.columns and a.pairs == b.pairs and (a.M, a.n_mass) == (b.M, b.n_mass), what
        for f in ("lo", "hi"):
            assert np.array_equal(bits(getattr(a, f)), bits(getattr(b, f))), (what, f)
        for f in ("mass1", "under", "over", "nan", "mass2", "outside2"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), (what, f)


# ------------------------------------------------------------------------------------------ crafted populations, C entry points
def crafted_spec(d):
    if d == 1:
        return A.ModelSpec(A.Normal(0.0, 3.0), A.Normal1D(0.4), A.Epa0toeps, seed=3)
    factors = [A.Normal(0.0, 1.0) for _ in range(d)]
    factors[1] = A.Poisson(4.0)                          # a discrete factor: push_p is rint there
    return A.ModelSpec(A.Factored(*factors), A.MVNormal(tuple([0.25] * d)), A.Epa0toeps, seed=3)


@pytest.fixture(scope="module")
def ops_of():
    made = {}

    def get(d):
        if d not in made:
            made[d] = HipOps(crafted_spec(d))
        return made[d]
    yield get
    for o in made.values():
        o.close()


def crafted_weights(N, pattern, rng):
    if pattern == "none":
        return None
    if pattern == "equal":
        return np.full(N, 1.0 / N)
    w = rng.random(N) + 0.05
    w[rng.random(N) < 0.3] = 0.0
    w[min(2040, N // 2):min(2060, N)] = 0.0            # a run of weightless positions across the first tile boundary (or to the end)
    w[N // 4] += 0.5                                    # never all dead
    return w / w.sum()


def device_adjusted(ops, syn, wns, dSb, nb, cols, t, ridge, beta=None, hist=None):
    """the record of posterior_adjusted through the C entry points, in the engine's order; ``beta``: skip the solve"""
    d, N = syn.d, syn.N
    pop = (syn.bits, syn.slot0, syn.slot1, wns)
    x_mean = ops.posterior_moments(*pop, N, want_second=False)[0]
    s_all, S_all = ops.columns_moments(dSb, wns, m=nb, want_second=True)[:2]
    s_mean = s_all[cols]
    S_sx = ops.adjust_cross(*pop, N, dSb, cols, s_mean, x_mean)
    if beta is None:
        beta = adjust_solve(S_all[np.ix_(cols, cols)], S_sx, ridge, cols)
    Y = ops.adjust_apply(*pop, N, dSb, cols, t, beta)
    mean, S, W, Q, n_pos = ops.columns_moments(Y, wns, m=d, want_second=True)
    q, M, n_mass = ops.columns_wquantiles(Y, wns, PROBS, m=d)
    h = None
    if hist:
        hc, bins, rng_, pairs, bins2 = hist_options(hist, d)
        lo_hi, mass1, tallies1, mass2, outside2, M, n_mass = ops.columns_histograms(Y, wns, m=d, columns=hc, bins=bins, range=rng_,
                                                                                    pairs=pairs, bins2=bins2)
        h = make_hist(hc, bins, lo_hi, mass1, tallies1, pairs, bins2, mass2, outside2, M, n_mass)
    rec = make_summary(mean, S, W, Q, n_pos, np.empty((0, d)), (), True, np.ascontiguousarray(q.T), PROBS, M, n_mass, h)
    return make_adjusted(rec, beta, cols, t, ridge, s_mean, x_mean, S_sx, Y.cpu().numpy())


@pytest.mark.parametrize("pattern", ["none", "equal", "unequal"])
@pytest.mark.parametrize("d,c,lds", [(1, 1, 1), (2, 3, 5), (5, 17, 24), (32, 32, 32), (3, 64, 64), (33, 9, 9)])
@pytest.mark.parametrize("N", [1, 2047, 2049, 3 * 2048 + 5])
def test_crafted_populations_through_the_c_entries(ops_of, N, d, c, lds, pattern):
    """N: one position, both sides of a tile boundary, four tiles with a ragged end; (d, c, lds): one column each, odd strides and a
    stride larger than c, j-blocks of 4 that end inside c (17, 9), k-chunks of 8 that end inside d (5, 33, 3), more parameters than
    regressors and the reverse"""
    ops = ops_of(d)
    rng = np.random.default_rng(1000003 * d + 1009 * c + 10 * N + len(pattern))
    w = crafted_weights(N, pattern, rng)
    live = np.ones(N, dtype=bool) if w is None else w > 0
    values = rng.standard_normal((N, d)) * 2.3 + 1.0
    syn = synthetic(ops.spec, N, rng, live, values=values, weights=None if w is None else w, ops=ops)
    wns = None if w is None else syn.wns
    P = np.where(live[:, None], syn.P, np.nan)                          # push_p of the current rows; dead rows poisoned
    G = rng.standard_normal((d, c))
    V = np.where(live[:, None], syn.P, 0.0) @ G + rng.standard_normal((N, c)) * 0.7 + 0.3
    Sb = np.full((N, lds), np.nan)                                      # the padding columns are never read
    Sb[:, :c] = np.where(live[:, None], V, np.nan)                      # rows of weightless positions are poisoned
    dSb = torch.from_numpy(Sb).to(ops.device)
    t = rng.standard_normal(c)
    what = (N, d, c, lds, pattern)
    variants = [(list(range(c)), 0.0)]
    if c >= 3:
        variants.append((list(range(1, c, 2)), 0.25))                  # a columns subset, and a ridge
    for cols, ridge in variants:
        tt = t[cols]
        if int(live.sum()) > len(cols) + 1:
            ref = adjust_reference(P, Sb[:, :c], w, target=tt, columns=cols, ridge=ridge, cov=True, wquantiles=PROBS, rows=True,
                                   hist=dict(bins=5, pairs="all", bins2=3) if d >= 2 else dict(bins=5))
            dev = device_adjusted(ops, syn, wns, dSb, c, cols, tt, ridge, hist=dict(bins=5, pairs="all", bins2=3) if d >= 2 else dict(bins=5))
        else:
            # too few positions for a regression (one position: every centred value is 0): the two passes with coefficients of
            # the test's own, against the pieces of the restatement
            beta = rng.standard_normal((len(cols), d))
            mx, ms = summary_reference(P, w, cov=False), summary_reference(Sb[:, :c], w, cov=False)
            wl = np.where(live, 1.0 if w is None else w, 0.0)
            Cs = np.where(live[:, None], Sb[:, cols], 0.0) - ms.mean[cols]
            Cx = np.where(live[:, None], P, 0.0) - mx.mean
            S_sx = np.stack([tile_tree_sum(np.where(live[:, None], wl[:, None] * (Cs[:, j:j + 1] * Cx), 0.0)) for j in range(len(cols))])
            Y = adjust_apply(P, Sb[:, cols], live, tt, beta)
            ref = make_adjusted(summary_reference(Y, w, cov=True, wquantiles=PROBS), beta, cols, tt, ridge, ms.mean[cols], mx.mean, S_sx, Y)
            dev = device_adjusted(ops, syn, wns, dSb, c, cols, tt, ridge, beta=beta)
        assert_same_adjusted(dev, ref, what + (len(cols), ridge))
        assert (dev.P[~live] == 0).all() and not np.signbit(dev.P[~live]).any()
        assert np.isfinite(dev.P).all() and np.isfinite(dev.S_sx).all()
    # Y with a stride of its own: the same rows, and the columns beyond d are not written
    Yw = torch.full((N, d + 3), -7.0, dtype=torch.float64, device=ops.device)
    ops.adjust_apply(syn.bits, syn.slot0, syn.slot1, wns, N, dSb, cols, t[cols], dev.beta, Yw)
    Yh = Yw.cpu().numpy()
    assert (Yh[:, d:] == -7.0).all() and np.array_equal(bits(Yh[:, :d]), bits(dev.P))


def test_refusals_come_back_through_the_error_string(ops_of):
    ops = ops_of(2)
    rng = np.random.default_rng(1)
    N = 100
    syn = synthetic(ops.spec, N, rng, np.ones(N, dtype=bool), ops=ops)
    pop = (syn.bits, syn.slot0, syn.slot1, syn.wns)
    Sb = torch.from_numpy(rng.standard_normal((N, 3))).to(ops.device)
    wide = torch.zeros((4, 300), dtype=torch.float64, device=ops.device)
    sm, xm = np.zeros(3), np.zeros(2)
    with pytest.raises(_lib.AbcdezError, match=r"adjust: the columns must be 1 <= n_cols <= min\(lds, 256\)"):
        ops.adjust_cross(*pop, N, Sb, [], np.zeros(0), xm)
    with pytest.raises(_lib.AbcdezError, match=r"adjust: the columns must be 1 <= n_cols <= min\(lds, 256\)"):
        ops.adjust_cross(syn.bits, syn.slot0, syn.slot1, None, 4, wide, list(range(257)), np.zeros(257), xm)
    for bad in ([1, 0, 2], [0, 1, 1], [0, 1, 3], [-1, 0, 1]):
        with pytest.raises(_lib.AbcdezError, match="adjust: the columns must be strictly increasing in 0 .. lds - 1"):
            ops.adjust_cross(*pop, N, Sb, bad, sm, xm)
        with pytest.raises(_lib.AbcdezError, match="adjust: the columns must be strictly increasing in 0 .. lds - 1"):
            ops.adjust_apply(*pop, N, Sb, bad, sm, np.zeros((3, 2)))
    with pytest.raises(_lib.AbcdezError, match="adjust: a mean of the simulated data or of the parameters is not finite"):
        ops.adjust_cross(*pop, N, Sb, [0, 1, 2], np.array([0.0, math.nan, 0.0]), xm)
    with pytest.raises(_lib.AbcdezError, match="adjust: a mean of the simulated data or of the parameters is not finite"):
        ops.adjust_cross(*pop, N, Sb, [0, 1, 2], sm, np.array([math.inf, 0.0]))
    with pytest.raises(_lib.AbcdezError, match="adjust: the target is not finite"):
        ops.adjust_apply(*pop, N, Sb, [0, 1, 2], np.array([0.0, math.nan, 0.0]), np.zeros((3, 2)))
    with pytest.raises(_lib.AbcdezError, match="adjust: a regression coefficient is not finite"):
        ops.adjust_apply(*pop, N, Sb, [0, 1, 2], sm, np.array([[0.0, 1.0], [math.inf, 0.0], [0.0, 0.0]]))
    with pytest.raises(_lib.AbcdezError, match=r"adjust: ldy must be at least length\(prior\)"):
        ops.adjust_apply(*pop, N, Sb, [0, 1, 2], sm, np.zeros((3, 2)), torch.zeros((N, 1), dtype=torch.float64, device=ops.device))
    with pytest.raises(_lib.AbcdezError, match="adjust: N out of range"):
        ops.adjust_cross(*pop, 0, Sb, [0, 1, 2], sm, xm)
    # the context still works
    assert np.isfinite(ops.adjust_cross(*pop, N, Sb, [0, 2], sm[:2], xm)).all()


# ------------------------------------------------------------------------------------------ real runs
USER_BLOB3 = """
__device__ double abz_user_dist(const double* theta, int d, const double* data, int n_data, const double* sim_p,
                                abz_user_rng& rng) {
  double z0, z1; rng.normal_pair(z0, z1);
  const double x = __builtin_fma(sim_p[0], z0, theta[0]), y = __builtin_fma(sim_p[0], z1, theta[1]);
  return __builtin_fabs(x - data[0]) + __builtin_fabs(y - data[1]);
}
__device__ void abz_user_blob(const double* theta, int d, const double* data, int n_data, const double* sim_p,
                              abz_user_rng& rng, double* blob, int n_blob) {
  double z0, z1; rng.normal_pair(z0, z1);
  const double x = __builtin_fma(sim_p[0], z0, theta[0]), y = __builtin_fma(sim_p[0], z1, theta[1]);
  blob[0] = x; blob[1] = y; blob[2] = x * y;
}
"""
WIEN = tuple(math.sqrt(0.25 * t * t + 4.0 * t) for t in range(8))
LV_OBS = (1.0, 0.5, 1.46, 0.43, 1.77, 0.62, 1.52, 1.13, 0.95, 1.31, 0.66, 1.09)      # six observations (x, y)
OPTS = dict(cov=True, wquantiles=PROBS, hist=dict(bins=7), rows=True)


@pytest.mark.parametrize("abck", list(ABCKS))
def test_normal1d_under_the_four_kernels(abck):
    """the conjugate model of the CPU law test, stopped at a loose epsilon: unequal weights for the Epanechnikov kernels"""
    N = 4096
    r = A.abcdesmc(A.Normal(0.0, 2.0), A.Normal1D(1.5, 1.0, blobs=True), 0.0, None, nparticles=N, α=0.6, δess=0.25, ABCk=ABCKS[abck],
                   verbose=False, rng=5, max_iters=4)
    assert r.iters == 4 and (r.Wns == 0).any() and r.blobs.shape == (N,)
    dev = r.engine.posterior_adjusted(**OPTS)
    ref = adjust_reference(r.P, r.blobs, r.Wns, target=[1.5], **OPTS)          # the default target: the simulator's data
    assert_same_adjusted(dev, ref, abck)
    assert dev.beta.shape == (1, 1) and dev.beta[0, 0] > 0.0 and dev.P.shape == (N, 1)
    print(abck, "dead", int((r.Wns == 0).sum()), "beta", dev.beta[0, 0], "raw mean", dev.x_mean[0], "adjusted", dev.mean[0])


def real_cases():
    return {
        # the first observation of the Wiener series is the constant 0, and the series of a particle shares one noise factor, so
        # its columns are nearly collinear (all seven are refused, as they should be): three of them, and a ridge
        "wiener": (A.Factored(A.Uniform(-2, 2), A.Uniform(0, 4)), A.WienerRMS(WIEN, blobs=True), dict(columns=[1, 4, 7], ridge=1e-3)),
        "lv": (A.Factored(*[A.Uniform(0.0, 2.0)] * 4), A.LotkaVolterraRK4(LV_OBS, dt=0.05, steps_per_obs=10, blobs=True), dict(ridge=1e-3)),
        "user3": (A.Factored(A.Normal(0.0, 2.0), A.Normal(0.0, 2.0)),
                  A.UserSimulator(USER_BLOB3, params=(0.5,), data=(1.0, -1.0), n_blob=3), dict(target=(1.0, -1.0, -1.0))),
    }


@pytest.mark.parametrize("name", ["wiener", "lv", "user3"])
def test_adjusted_posterior_of_a_real_run_is_the_reference(name):
    prior, sim, extra = real_cases()[name]
    N = 4096
    r = A.abcdesmc(prior, sim, 0.0, None, nparticles=N, α=0.6, δess=0.25, ABCk=A.Epa0toeps, verbose=False, rng=5, max_iters=4)
    assert r.iters == 4 and (r.Wns == 0).any()
    opts = dict(OPTS, hist=dict(bins=7, pairs="all", bins2=5), **extra)
    dev = r.engine.posterior_adjusted(**opts)
    ref = adjust_reference(r.P, r.blobs, r.Wns, data=tuple(sim.data()), **opts)
    assert_same_adjusted(dev, ref, name)
    assert np.isfinite(dev.P).all() and (dev.P[r.Wns == 0] == 0).all()
    if name == "user3":
        with pytest.raises(ValueError, match="adjust: target is required"):
            r.engine.posterior_adjusted()


def test_abcdemc_classic_storage_unit_weights():
    prior, sim, extra = real_cases()["wiener"]
    opts = dict(OPTS, **extra)
    r = A.abcdemc(prior, sim, 0.5, None, nparticles=2049, generations=6, verbose=False, rng=8, adjust=opts)
    ref = adjust_reference(r.P, r.blobs, None, data=WIEN, **opts)
    assert_same_adjusted(r.adjusted, ref, "abcdemc")
    assert r.adjusted.n_pos == 2049 and r.adjusted.W == 2049.0


def test_driver_keyword_and_download_false():
    prior, sim, extra = real_cases()["lv"]
    kw = dict(nparticles=2049, α=0.6, δess=0.33, ABCk=A.Epa0toeps, verbose=False, rng=5, max_iters=3)
    r = A.abcdesmc(prior, sim, 0.0, None, adjust=extra, **kw)
    assert_same_adjusted(r.adjusted, adjust_reference(r.P, r.blobs, r.Wns, data=LV_OBS, **extra), "adjust=dict")
    assert r.adjusted.P is None and r.adjusted.beta.shape == (12, 4)
    bare = A.abcdesmc(prior, sim, 0.0, None, download=False, adjust=dict(extra, wquantiles=(0.025, 0.5, 0.975), rows=True), **kw)
    assert bare.P is None and bare.blobs is None
    assert_same_adjusted(bare.adjusted, adjust_reference(r.P, r.blobs, r.Wns, data=LV_OBS, wquantiles=(0.025, 0.5, 0.975), rows=True, **extra),
                         "download=False")
    with pytest.raises(ValueError, match=r"adjust: needs a simulator that returns blobs \(blobs=True\)"):
        A.abcdesmc(prior, A.LotkaVolterraRK4(LV_OBS, dt=0.05, steps_per_obs=10), 0.0, None, adjust=True, **kw)


# ------------------------------------------------------------------------------------------ continuation
def test_a_run_continued_on_the_same_engine_is_bit_identical():
    """two engines on the same key, the next generation's select enqueued ahead behind every group of sweeps; one is asked for the
    adjusted posterior between the generations (the five generations include resamplings)"""
    prior, sim, extra = real_cases()["wiener"]
    spec = A.ModelSpec(prior, sim, A.Epa0toeps, seed=9)
    N = 5001
    engs = [PopulationEngine(spec, N, ops=HipOps(spec), storage="packed") for _ in range(2)]
    out = [[], []]
    for which, e in enumerate(engs):
        e.init_population()
        e.reset_weights()
        eps = eps_k = math.inf
        for gen in range(5):
            g = e.smc_generation(0.6, eps, 0.0, eps_k, 0.5 * N, 2.38 / math.sqrt(2 * spec.d), 1e-5, 3, 1.0, select_ahead=True)
            eps = eps_k = g["eps"]
            out[which].append((g["eps"], g["wnorm"], g["ess"], g["n_alive"], tuple(g["range"]), tuple(g["naccs"]), tuple(g["nsims"]),
                               g["Ki"], g.get("logZ")))
            if which == 0:
                assert e.posterior_adjusted(**dict(OPTS, **extra)).n_mass >= 1
        e.discard_select_ahead()
    assert out[0] == out[1]
    assert engs[0].draw == engs[1].draw >= 1, "the run was meant to resample"
    a, b = engs[0].result(), engs[1].result()
    for f in ("P", "theta", "logpi", "C", "Wns", "alive", "blobs"):
        assert np.array_equal(a[f], b[f]), f
    assert engs[0].ops.smc_select_stats() == engs[1].ops.smc_select_stats()      # the selects enqueued ahead were all still used
