"""Bounded transforms and the heteroscedastic correction of the regression adjustment on the device (csrc/abz_adjust_hcorr.hip:
abcdez_adjust_transform / _cross_dense / _logres / _apply_scaled, PopulationEngine.posterior_adjusted(hcorr=, transform=)) against
abcdez_amd.summary.adjust_reference with ``math=`` the oracle's abz_log / abz_exp -- BIT FOR BIT, by the techniques of
tests/test_gpu_posterior_adjust.py: float64 fields as uint64 (gamma, S_sz, z_mean and the rows P included), crafted populations and
blob matrices through the C entry points with NaN in the rows of weightless positions and in the padding columns."""
import math

import numpy as np
import pytest
import torch

import abcdez_amd as A
from abcdez_amd import _lib
from abcdez_amd import summary as S
from abcdez_amd.engine import HipOps, PopulationEngine
from abcdez_amd.summary import adjust_reference, adjust_solve, make_adjusted, make_summary, summary_reference, tile_tree_sum
from test_gpu_posterior_adjust import LV_OBS, WIEN, assert_same_adjusted, bits, crafted_spec, crafted_weights, real_cases
from test_gpu_posterior_summary_edges import synthetic

pytestmark = pytest.mark.gpu

PROBS = (0.0, 0.025, 0.5, 0.975, 1.0)


@pytest.fixture(scope="module")
def omath(oracle):
    """(log, exp) over float64 arrays: the oracle's orc_math_eval 0 / 1 (the literal Python pair is too slow here)"""
    def fn(which):
        def f(a):
            x = np.ascontiguousarray(a, dtype=np.float64)
            y, y2 = np.zeros_like(x), np.zeros_like(x)
            if x.size:
                oracle.lib().orc_math_eval(which, x.ctypes.data, y.ctypes.data, y2.ctypes.data, x.size)
            return y
        return f
    return fn(0), fn(1)


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


def assert_same(dev, ref, what):
    assert_same_adjusted(dev, ref, what)
    assert dev.hcorr == ref.hcorr and dev.transform == ref.transform, what
    for f in ("gamma", "S_sz", "z_mean"):
        a, b = getattr(dev, f), getattr(ref, f)
        assert (a is None) == (b is None), (what, f)
        if b is not None:
            assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), (what, f, a, b)


# ------------------------------------------------------------------------------------------ crafted populations, C entry points
def mixed_transform(d):
    """log, none, logit, log, ...: column 1 of crafted_spec is the discrete one and stays untransformed"""
    if d == 1:
        return ["log"]
    return [("log", None, ("logit", 0.0, 60.0))[k % 3] for k in range(d)]


def device_adjusted(ops, syn, wns, dSb, nb, cols, t, ridge, hcorr, tf, beta=None, gamma=None):
    """the record of posterior_adjusted through the C entry points, in the engine's order; ``beta`` / ``gamma``: skip the solves"""
    d, N = syn.d, syn.N
    pop = (syn.bits, syn.slot0, syn.slot1, wns)
    U = None
    if tf is not None:
        U = ops.adjust_transform(*pop, N, tf)
        x_mean = ops.columns_moments(U, wns, m=d, want_second=False)[0]
    else:
        x_mean = ops.posterior_moments(*pop, N, want_second=False)[0]
    s_all, S_all = ops.columns_moments(dSb, wns, m=nb, want_second=True)[:2]
    s_mean = s_all[cols]
    S_sx = ops.adjust_cross(*pop, N, dSb, cols, s_mean, x_mean) if U is None else ops.adjust_cross_dense(U, wns, N, dSb, cols, s_mean, x_mean, m=d)
    S_ss = S_all[np.ix_(cols, cols)]
    if beta is None:
        beta = adjust_solve(S_ss, S_sx, ridge, cols)
    z_mean = S_sz = None
    Zh = None
    if hcorr:
        Z = ops.adjust_logres(*pop, N, U, dSb, cols, s_mean, x_mean, beta)
        Zh = Z.cpu().numpy()
        z_mean = ops.columns_moments(Z, wns, m=d, want_second=False)[0]
        if gamma is None:
            S_sz = ops.adjust_cross_dense(Z, wns, N, dSb, cols, s_mean, z_mean, m=d)
            gamma = adjust_solve(S_ss, S_sz, ridge, cols)
        Y = ops.adjust_apply_scaled(*pop, N, U, dSb, cols, t, beta, s_mean=s_mean, x_mean=x_mean, gamma=gamma,
                                    m=S.adjust_centre(x_mean, beta, s_mean, t), tf=tf, Y=Z)
        assert Y.data_ptr() == Z.data_ptr()                                # the adjusted rows were written over the log residuals
    else:
        Y = ops.adjust_apply_scaled(*pop, N, U, dSb, cols, t, beta, tf=tf)
    mean, Sm, W, Q, n_pos = ops.columns_moments(Y, wns, m=d, want_second=True)
    q, M, n_mass = ops.columns_wquantiles(Y, wns, PROBS, m=d)
    rec = make_summary(mean, Sm, W, Q, n_pos, np.empty((0, d)), (), True, np.ascontiguousarray(q.T), PROBS, M, n_mass, None)
    out = make_adjusted(rec, beta, cols, t, ridge, s_mean, x_mean, S_sx, Y.cpu().numpy(), hcorr, tf, gamma if hcorr else None, z_mean, S_sz)
    out.Z, out.U = Zh, None if U is None else U.cpu().numpy()
    return out


def pieces(P, Sb, w, live, cols, t, ridge, hcorr, tf, beta, gamma, math):
    """the restatement from its pieces with coefficients of the test's own, for populations too small for a regression"""
    N, d = P.shape
    X = P
    if tf is not None:
        X = np.zeros((N, d))
        X[live] = S.adjust_forward(P[live], tf, math)
    mx, ms = summary_reference(X, w, cov=False), summary_reference(Sb, w, cov=False)
    s_mean, x_mean = ms.mean[cols], mx.mean
    wl = np.where(live, 1.0 if w is None else w, 0.0)
    Bc = Sb[:, cols]
    Cs = np.where(live[:, None], Bc, 0.0) - s_mean
    Cx = np.where(live[:, None], X, 0.0) - x_mean
    S_sx = np.stack([tile_tree_sum(np.where(live[:, None], wl[:, None] * (Cs[:, j:j + 1] * Cx), 0.0)) for j in range(len(cols))])
    Z = z_mean = None
    if hcorr:
        E = S.adjust_residual(X, Bc, live, s_mean, x_mean, beta)
        Z = np.zeros((N, d))
        with np.errstate(all="ignore"):
            Z[live] = math[0](E[live] * E[live])
            z_mean = summary_reference(Z, w, cov=False).mean
        V = S.adjust_scaled(E, Bc, live, t, gamma, S.adjust_centre(x_mean, beta, s_mean, t), math)
    else:
        V = S.adjust_apply(X, Bc, live, t, beta)
    Y = V
    if tf is not None:
        Y = np.zeros((N, d))
        Y[live] = S.adjust_back(V[live], tf, math)
    out = make_adjusted(summary_reference(Y, w, cov=True, wquantiles=PROBS), beta, cols, t, ridge, s_mean, x_mean, S_sx, Y, hcorr, tf,
                        gamma if hcorr else None, z_mean, None)
    out.Z = Z
    return out


@pytest.mark.parametrize("pattern", ["none", "equal", "unequal"])
@pytest.mark.parametrize("d,c,lds", [(1, 1, 1), (3, 5, 7), (8, 4, 4), (9, 17, 24)])
@pytest.mark.parametrize("N", [1, 2047, 2049, 2 * 2048 + 5])
def test_crafted_populations_through_the_c_entries(ops_of, omath, N, d, c, lds, pattern):
    """N: one position, both sides of a tile boundary, two tiles with a ragged end (block edges of 256 inside all of them); (d, c,
    lds): one column each, odd strides and a stride larger than c, k-chunks of 8 (logres) and of 4 (scaled apply) that end on and
    inside d (8, 9, 3, 1), j-blocks of 4 that end on and inside c (4, 17, 5).  Every combination of the two options, the transform a
    mixed per-column list; the spread of the parameters grows along the first blob column, so gamma is not noise."""
    ops = ops_of(d)
    rng = np.random.default_rng(680 + 1000003 * d + 1009 * c + 10 * N + len(pattern))
    w = crafted_weights(N, pattern, rng)
    live = np.ones(N, dtype=bool) if w is None else w > 0
    V = rng.uniform(-1.0, 1.0, (N, c))
    G = rng.uniform(0.05, 0.3, (c, d))
    values = np.exp(0.7 + V @ G / math.sqrt(c) + 0.25 * np.exp(0.6 * V[:, :1]) * rng.standard_normal((N, d))) + 0.6      # > 0.6: rint >= 1
    assert values.max() < 59.0
    syn = synthetic(ops.spec, N, rng, live, values=values, weights=None if w is None else w, ops=ops)
    wns = None if w is None else syn.wns
    P = np.where(live[:, None], syn.P, np.nan)                          # push_p of the current rows; dead rows poisoned
    Sb = np.full((N, lds), np.nan)                                      # the padding columns are never read
    Sb[:, :c] = np.where(live[:, None], V, np.nan)                      # rows of weightless positions are poisoned
    dSb = torch.from_numpy(Sb).to(ops.device)
    t = rng.uniform(-0.8, 0.8, c)
    variants = [(list(range(c)), 0.0)]
    if c >= 3:
        variants.append((list(range(1, c, 2)), 0.25))                  # a columns subset, and a ridge
    tf_list = mixed_transform(d)
    for cols, ridge in variants:
        tt = t[cols]
        for hcorr, transform in ((True, tf_list), (True, None), (False, tf_list), (False, None)):
            tf = S.adjust_transform(transform, d)
            what = (N, d, c, lds, pattern, len(cols), ridge, hcorr, transform is not None)
            if int(live.sum()) > len(cols) + 1:
                ref = adjust_reference(P, Sb[:, :c], w, target=tt, columns=cols, ridge=ridge, cov=True, wquantiles=PROBS, rows=True,
                                       hcorr=hcorr, transform=transform, math=omath)
                dev = device_adjusted(ops, syn, wns, dSb, c, cols, tt, ridge, hcorr, tf)
                assert np.isfinite(dev.P).all() and np.isfinite(dev.S_sx).all(), what
            else:
                # one position: every centred value is 0, both solves refuse and the log residual is -inf; the passes with
                # coefficients of the test's own, against the pieces of the restatement
                beta, gamma = rng.standard_normal((len(cols), d)), rng.standard_normal((len(cols), d))
                ref = pieces(P, Sb[:, :c], w, live, cols, tt, ridge, hcorr, tf, beta, gamma, omath)
                dev = device_adjusted(ops, syn, wns, dSb, c, cols, tt, ridge, hcorr, tf, beta=beta, gamma=gamma)
                if hcorr:
                    assert np.array_equal(bits(dev.Z), bits(ref.Z)) and (ref.Z[live] == -math.inf).all(), what
            assert_same(dev, ref, what)
            assert (dev.P[~live] == 0).all() and not np.signbit(dev.P[~live]).any(), what
            if dev.U is not None:
                assert (dev.U[~live] == 0).all() and not np.signbit(dev.U[~live]).any(), what
            if tf is not None:
                for k, e in enumerate(tf_list):
                    lo, hi = (0.0, math.inf) if e == "log" else (-math.inf, math.inf) if e is None else e[1:]
                    assert ((dev.P[live, k] >= lo) & (dev.P[live, k] <= hi)).all(), (what, k)
    # without gamma and without a transform the scaled pass IS the plain apply; and a Y with a stride of its own
    pop = (syn.bits, syn.slot0, syn.slot1, wns)
    plain = ops.adjust_apply(*pop, N, dSb, cols, tt, dev.beta).cpu().numpy()
    Yw = torch.full((N, d + 3), -7.0, dtype=torch.float64, device=ops.device)
    ops.adjust_apply_scaled(*pop, N, None, dSb, cols, tt, dev.beta, Y=Yw)
    Yh = Yw.cpu().numpy()
    assert (Yh[:, d:] == -7.0).all() and np.array_equal(bits(Yh[:, :d]), bits(plain))


def test_refusals_come_back_through_the_error_string(ops_of):
    ops = ops_of(2)
    rng = np.random.default_rng(1)
    N = 100
    syn = synthetic(ops.spec, N, rng, np.ones(N, dtype=bool), values=rng.uniform(1.0, 3.0, (N, 2)), ops=ops)
    pop = (syn.bits, syn.slot0, syn.slot1, syn.wns)
    Sb = torch.from_numpy(rng.standard_normal((N, 3))).to(ops.device)
    sm, xm, b = np.zeros(3), np.zeros(2), np.zeros((3, 2))
    kinds = lambda *k: (np.array(k, dtype=np.int32), np.array([[0.0, 4.0], [0.0, 4.0]]))
    narrow = torch.zeros((N, 1), dtype=torch.float64, device=ops.device)
    U = ops.adjust_transform(*pop, N, kinds(1, 2))
    with pytest.raises(_lib.AbcdezError, match="adjust: transform: unknown kind for parameter 1"):
        ops.adjust_transform(*pop, N, kinds(1, 3))
    with pytest.raises(_lib.AbcdezError, match="adjust: transform: logit of parameter 0 needs finite bounds with lo < hi"):
        ops.adjust_transform(*pop, N, (np.array([2, 0], dtype=np.int32), np.array([[4.0, 4.0], [0.0, 1.0]])))
    with pytest.raises(_lib.AbcdezError, match="adjust: transform: logit of parameter 1 needs finite bounds with lo < hi"):
        ops.adjust_apply_scaled(*pop, N, None, Sb, [0, 1, 2], sm, b, tf=(np.array([0, 2], dtype=np.int32), np.array([[0.0, 1.0], [0.0, math.inf]])))
    with pytest.raises(_lib.AbcdezError, match=r"adjust: ldu must be at least length\(prior\)"):
        ops.adjust_transform(*pop, N, kinds(1, 2), narrow)
    with pytest.raises(_lib.AbcdezError, match=r"adjust: ldz must be at least length\(prior\)"):
        ops.adjust_logres(*pop, N, U, Sb, [0, 1, 2], sm, xm, b, narrow)
    with pytest.raises(_lib.AbcdezError, match=r"adjust: ldy must be at least length\(prior\)"):
        ops.adjust_apply_scaled(*pop, N, U, Sb, [0, 1, 2], sm, b, Y=narrow)
    with pytest.raises(_lib.AbcdezError, match="adjust: Y must not be U"):
        ops.adjust_apply_scaled(*pop, N, U, Sb, [0, 1, 2], sm, b, Y=U)
    with pytest.raises(_lib.AbcdezError, match="adjust: Z must not be U"):
        ops.adjust_logres(*pop, N, U, Sb, [0, 1, 2], sm, xm, b, U)
    with pytest.raises(_lib.AbcdezError, match="adjust: a regression coefficient is not finite"):
        ops.adjust_apply_scaled(*pop, N, U, Sb, [0, 1, 2], sm, b, s_mean=sm, x_mean=xm, gamma=np.where(np.arange(6).reshape(3, 2) == 3, math.nan, 0.0),
                                m=xm)
    with pytest.raises(_lib.AbcdezError, match="adjust: a mean of the simulated data or of the parameters is not finite"):
        ops.adjust_apply_scaled(*pop, N, U, Sb, [0, 1, 2], sm, b, s_mean=sm, x_mean=xm, gamma=b, m=np.array([0.0, math.inf]))
    with pytest.raises(_lib.AbcdezError, match="adjust: a mean of the simulated data or of the parameters is not finite"):
        ops.adjust_logres(*pop, N, U, Sb, [0, 1, 2], sm, np.array([math.nan, 0.0]), b)
    with pytest.raises(_lib.AbcdezError, match="adjust: a mean of the simulated data or of the parameters is not finite"):
        ops.adjust_cross_dense(U, syn.wns, N, Sb, [0, 1, 2], np.array([0.0, math.nan, 0.0]), xm)
    for bad in ([1, 0, 2], [0, 1, 3]):
        with pytest.raises(_lib.AbcdezError, match="adjust: the columns must be strictly increasing in 0 .. lds - 1"):
            ops.adjust_cross_dense(U, syn.wns, N, Sb, bad, sm, xm)
        with pytest.raises(_lib.AbcdezError, match="adjust: the columns must be strictly increasing in 0 .. lds - 1"):
            ops.adjust_logres(*pop, N, U, Sb, bad, sm, xm, b)
    with pytest.raises(ValueError, match="adjust: gamma, m, s_mean and x_mean are given together or not at all"):
        ops.adjust_apply_scaled(*pop, N, U, Sb, [0, 1, 2], sm, b, gamma=b)
    # the context still works
    assert np.isfinite(ops.adjust_cross_dense(U, syn.wns, N, Sb, [0, 2], sm[:2], xm)).all()
    assert ops.lib.abcdez_version() >= 680


# ------------------------------------------------------------------------------------------ real runs
OPTS = dict(cov=True, wquantiles=PROBS, hist=dict(bins=7), rows=True, hcorr=True)
WIENER_TF = [("logit", -2.0, 2.0), ("logit", 0.0, 4.0)]          # the supports of the two uniform priors


@pytest.mark.parametrize("name", ["wiener", "lv"])
def test_adjusted_posterior_of_a_real_run_is_the_reference(name, omath):
    prior, sim, extra = real_cases()[name]
    N = 4096
    r = A.abcdesmc(prior, sim, 0.0, None, nparticles=N, α=0.6, δess=0.25, ABCk=A.Epa0toeps, verbose=False, rng=5, max_iters=4)
    assert r.iters == 4 and (r.Wns == 0).any()
    live = r.Wns > 0
    for transform, hcorr in ((WIENER_TF if name == "wiener" else "log", True), (WIENER_TF if name == "wiener" else "log", False), (None, True)):
        opts = dict(OPTS, hist=dict(bins=7, pairs="all", bins2=5), transform=transform, hcorr=hcorr, **extra)
        dev = r.engine.posterior_adjusted(**opts)
        ref = adjust_reference(r.P, r.blobs, r.Wns, data=tuple(sim.data()), math=omath, **opts)
        assert_same(dev, ref, (name, transform, hcorr))
        assert np.isfinite(dev.P).all() and (dev.P[~live] == 0).all()
        if transform == "log":
            assert (dev.P[live] > 0.0).all() and dev.transform == ("log",) * 4
        elif transform is not None:
            assert ((dev.P[live] >= [-2.0, 0.0]) & (dev.P[live] <= [2.0, 4.0])).all()
    if name == "wiener":        # the first parameter is uniform on (-2, 2): a log is refused on the device route too, by name
        with pytest.raises(ValueError, match="adjust: transform: parameter 0 has a value outside the domain of its log transform"):
            r.engine.posterior_adjusted(transform="log", **extra)


def test_abcdemc_classic_storage_unit_weights(omath):
    prior, sim, extra = real_cases()["wiener"]
    opts = dict(OPTS, transform=[None, ("logit", 0.0, 4.0)], **extra)
    r = A.abcdemc(prior, sim, 0.5, None, nparticles=2049, generations=6, verbose=False, rng=8, adjust=opts)
    ref = adjust_reference(r.P, r.blobs, None, data=WIEN, math=omath, **opts)
    assert_same(r.adjusted, ref, "abcdemc")
    assert r.adjusted.n_pos == 2049 and r.adjusted.W == 2049.0 and r.adjusted.gamma.shape == (3, 2)


def test_driver_keyword_and_download_false(omath):
    prior, sim, extra = real_cases()["lv"]
    extra = dict(extra, hcorr=True, transform="log")
    kw = dict(nparticles=2049, α=0.6, δess=0.33, ABCk=A.Epa0toeps, verbose=False, rng=5, max_iters=3)
    r = A.abcdesmc(prior, sim, 0.0, None, adjust=extra, **kw)
    assert_same(r.adjusted, adjust_reference(r.P, r.blobs, r.Wns, data=LV_OBS, math=omath, **extra), "adjust=dict")
    assert r.adjusted.P is None and r.adjusted.beta.shape == (12, 4) and r.adjusted.gamma.shape == (12, 4)
    bare = A.abcdesmc(prior, sim, 0.0, None, download=False, adjust=dict(extra, wquantiles=(0.025, 0.5, 0.975), rows=True), **kw)
    assert bare.P is None and bare.blobs is None
    assert_same(bare.adjusted, adjust_reference(r.P, r.blobs, r.Wns, data=LV_OBS, wquantiles=(0.025, 0.5, 0.975), rows=True, math=omath, **extra),
                "download=False")
    assert (bare.adjusted.P >= 0.0).all() and (bare.adjusted.wquantiles > 0.0).all()


# ------------------------------------------------------------------------------------------ continuation
def test_a_run_continued_on_the_same_engine_is_bit_identical():
    """two engines on the same key, the next generation's select enqueued ahead behind every group of sweeps; one is asked for the
    corrected, transformed adjustment between the generations"""
    prior, sim, extra = real_cases()["wiener"]
    spec = A.ModelSpec(prior, sim, A.Epa0toeps, seed=9)
    N = 5000
    engs = [PopulationEngine(spec, N, ops=HipOps(spec), storage="packed") for _ in range(2)]
    out = [[], []]
    for which, e in enumerate(engs):
        e.init_population()
        e.reset_weights()
        eps = eps_k = math.inf
        for gen in range(4):
            g = e.smc_generation(0.6, eps, 0.0, eps_k, 0.5 * N, 2.38 / math.sqrt(2 * spec.d), 1e-5, 3, 1.0, select_ahead=True)
            eps = eps_k = g["eps"]
            out[which].append((g["eps"], g["wnorm"], g["ess"], g["n_alive"], tuple(g["range"]), tuple(g["naccs"]), tuple(g["nsims"]),
                               g["Ki"], g.get("logZ")))
            if which == 0:
                assert e.posterior_adjusted(**dict(OPTS, transform=WIENER_TF, **extra)).n_mass >= 1
        e.discard_select_ahead()
    assert out[0] == out[1]
    a, b = engs[0].result(), engs[1].result()
    for f in ("P", "theta", "logpi", "C", "Wns", "alive", "blobs"):
        assert np.array_equal(a[f], b[f]), f
    assert engs[0].ops.smc_select_stats() == engs[1].ops.smc_select_stats()      # the selects enqueued ahead were all still used
