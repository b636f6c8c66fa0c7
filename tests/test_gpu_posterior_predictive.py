"""Column summaries / posterior predictive on the device (the dense-matrix source of csrc/abz_summary.h: abcdez_columns_moments /
_wquantiles / _histograms, PopulationEngine.posterior_predictive) against abcdez_amd.summary.summary_reference /
predictive_reference of data that reached the host through the existing routes (the uploaded matrix itself, or ``r.blobs`` and ``r.Wns`` of the downloaded
result) -- BIT FOR BIT: float64 fields as uint64, integer fields exactly.  Crafted matrices go to the C entry points as plain device
pointers (the technique of tests/test_gpu_posterior_summary_edges.py): rows of weightless positions and the padding columns beyond m
hold NaN, so that one missing guard in a kernel poisons a sum."""
import math

import numpy as np
import pytest
import torch

import abcdez_amd as A
from abcdez_amd import _lib
from abcdez_amd.engine import HipOps, PopulationEngine
from abcdez_amd.summary import (adjust_reference, make_hist, make_sample, make_summary, predictive_reference, sample_reference,
                                summary_reference)

pytestmark = pytest.mark.gpu

PROBS = (0.0, 0.025, 0.5, 0.975, 1.0)
HIST = dict(bins=7, pairs="all", bins2=5)
ABCKS = {"indicator_strict": A.IndicatorStrict0toeps, "indicator": A.Indicator0toeps, "epa_strict": A.EpaStrict0toeps,
         "epa": A.Epa0toeps}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_record(dev, ref, what):
    assert dev.n_pos == ref.n_pos and (dev.M, dev.n_mass) == (ref.M, ref.n_mass), what
    for f in ("W", "Q", "ess"):
        assert bits(getattr(dev, f)) == bits(getattr(ref, f)), (what, f, getattr(dev, f), getattr(ref, f))
    assert dev.mean.shape == ref.mean.shape and np.array_equal(bits(dev.mean), bits(ref.mean)), (what, "mean", dev.mean, ref.mean)
    assert (dev.S is None) == (ref.S is None) and (dev.cov is None) == (ref.cov is None), what
    if ref.S is not None:
        assert np.array_equal(bits(dev.S), bits(ref.S)), (what, "S", np.abs(dev.S - ref.S).max())
        assert np.array_equal(bits(dev.cov), bits(ref.cov)), (what, "cov")
    assert dev.quantiles.shape == ref.quantiles.shape == (0, ref.mean.shape[0]) and dev.wprobs == ref.wprobs, what
    assert dev.wquantiles.shape == ref.wquantiles.shape, what
    assert np.array_equal(bits(dev.wquantiles), bits(ref.wquantiles)), (what, "wquantiles", dev.wquantiles, ref.wquantiles)
    assert (dev.hist is None) == (ref.hist is None), what
    if ref.hist is not None:
        a, b = dev.hist, ref.hist
        assert a.columns == b.columns and a.pairs == b.pairs and (a.bins, a.bins2) == (b.bins, b.bins2) and (a.M, a.n_mass) == (b.M, b.n_mass)
        for f in ("lo", "hi", "edges"):
            assert np.array_equal(bits(getattr(a, f)), bits(getattr(b, f))), (what, f)
        for f in ("mass1", "under", "over", "nan", "mass2", "outside2"):
            x, y = getattr(a, f), getattr(b, f)
            assert x.dtype == np.uint64 and x.shape == y.shape and np.array_equal(x, y), (what, f)


# ------------------------------------------------------------------------------------------ crafted matrices, C entry points
@pytest.fixture(scope="module")
def ops():
    spec = A.ModelSpec(A.Factored(A.Normal(0.0, 1.0), A.Normal(0.0, 1.0)), A.MVNormal((0.25, 0.25)), A.Epa0toeps, seed=3)
    o = HipOps(spec)
    yield o
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


def device_record(ops, X, w, m, hist, cov=True, range_=None):
    """the record of posterior_predictive through the three C entry points"""
    dX = torch.from_numpy(np.ascontiguousarray(X)).to(ops.device)
    dw = None if w is None else torch.from_numpy(w).to(ops.device)
    mean, S, W, Q, n_pos = ops.columns_moments(dX, dw, m=m, want_second=cov)
    q, M, n_mass = ops.columns_wquantiles(dX, dw, PROBS, m=m)
    h = None
    if hist:
        from abcdez_amd.summary import hist_options
        cols, bins, rng_, pairs, bins2 = hist_options(hist, m)
        lo_hi, mass1, tallies1, mass2, outside2, M2, n_mass2 = ops.columns_histograms(dX, dw, m=m, columns=cols, bins=bins, range=rng_,
                                                                                    pairs=pairs, bins2=bins2)
        assert (M2, n_mass2) == (M, n_mass)
        h = make_hist(cols, bins, lo_hi, mass1, tallies1, pairs, bins2, mass2, outside2, M2, n_mass2)
    return make_summary(mean, S, W, Q, n_pos, np.empty((0, m)), (), True, np.ascontiguousarray(q.T), PROBS, M, n_mass, h)


@pytest.mark.parametrize("pattern", ["none", "equal", "unequal"])
@pytest.mark.parametrize("m,ldx", [(1, 1), (2, 2), (11, 11), (17, 24), (64, 64)])
@pytest.mark.parametrize("N", [1, 2047, 2049, 3 * 2048 + 5])
def test_crafted_matrices_through_the_c_entries(ops, N, m, ldx, pattern):
    """N: one position, both sides of a tile boundary, four tiles with a ragged end; (m, ldx): odd strides, a stride larger than m,
    more than one 16-column chunk of the quantile gather (and 4-column blocks of the moment passes that end inside m)"""
    rng = np.random.default_rng(100000 * m + 10 * N + len(pattern))
    w = crafted_weights(N, pattern, rng)
    live = np.ones(N, dtype=bool) if w is None else w > 0
    V = rng.standard_normal((N, m)) * 3.1
    if N > 8:
        for k in range(m):                              # a few exact ties per column
            V[rng.integers(0, N, 3), k] = V[rng.integers(0, N, 3), k]
    if m >= 2:
        V[:, 1] = -1.75                                 # a constant column: automatic range +- 0.5
    X = np.full((N, ldx), np.nan)                       # the padding columns are never read
    X[:, :m] = np.where(live[:, None], V, np.nan)      # rows of weightless positions are poisoned
    what = (N, m, ldx, pattern)
    ref = summary_reference(X[:, :m], w, cov=True, wquantiles=PROBS, hist=HIST if m >= 2 else dict(bins=7))
    dev = device_record(ops, X, w, m, HIST if m >= 2 else dict(bins=7))
    assert_same_record(dev, ref, what)
    if m >= 2:
        assert dev.hist.lo[1] == -2.25 and dev.hist.hi[1] == -1.25
    # without the second moments: the same first ones, S untouched
    mean, S, W, Q, n_pos = ops.columns_moments(torch.from_numpy(X).to(ops.device), None if w is None else torch.from_numpy(w).to(ops.device),
                                               m=m, want_second=False)
    assert S is None and np.array_equal(bits(mean), bits(ref.mean)) and (bits(W), bits(Q), n_pos) == (bits(ref.W), bits(ref.Q), ref.n_pos)
    # a NaN in a counting row, under an explicit range: the NaN tally
    at = int(np.flatnonzero(live)[len(np.flatnonzero(live)) // 2])
    Xn = X.copy()
    Xn[at, 0] = np.nan
    opts = dict(HIST if m >= 2 else dict(bins=7), range=(-3.0, 3.0))
    href = summary_reference(Xn[:, :m], w, cov=False, hist=opts).hist
    hdev = device_record(ops, Xn, w, m, opts, cov=False).hist
    assert hdev.nan[0] == href.nan[0] > 0
    for f in ("mass1", "under", "over", "nan", "mass2", "outside2"):
        assert np.array_equal(getattr(hdev, f), getattr(href, f)), (what, f)


def test_refusals_come_back_through_the_error_string(ops):
    rng = np.random.default_rng(1)
    N = 100
    X = torch.from_numpy(rng.standard_normal((N, 3))).to(ops.device)
    wide = torch.zeros((4, 300), dtype=torch.float64, device=ops.device)
    zero = torch.zeros(N, dtype=torch.float64, device=ops.device)
    raw = torch.full((N,), 1e6, dtype=torch.float64, device=ops.device)        # weights that were never normalised
    for call in (lambda **k: ops.columns_moments(k["X"], k["w"], m=k["m"]),
                 lambda **k: ops.columns_wquantiles(k["X"], k["w"], (0.5,), m=k["m"], nk=1),
                 lambda **k: ops.columns_histograms(k["X"], k["w"], m=k["m"], columns=[0], bins=4)):
        with pytest.raises(_lib.AbcdezError, match="m must be in 1 .. 256"):
            call(X=X, w=None, m=0)
        with pytest.raises(_lib.AbcdezError, match="m must be in 1 .. 256"):
            call(X=wide, w=None, m=257)
        with pytest.raises(_lib.AbcdezError, match="ldx must be at least m"):
            call(X=X, w=None, m=5)
    with pytest.raises(_lib.AbcdezError, match="columns_moments: no particle has a positive weight"):
        ops.columns_moments(X, zero)
    with pytest.raises(_lib.AbcdezError, match="columns_wquantiles: no particle has a positive weight that carries mass"):
        ops.columns_wquantiles(X, zero, (0.5,))
    with pytest.raises(_lib.AbcdezError, match="columns_histograms: no particle has a positive weight that carries mass"):
        ops.columns_histograms(X, zero, bins=4)
    with pytest.raises(_lib.AbcdezError, match=r"columns_wquantiles: the total mass reaches 2\^63"):
        ops.columns_wquantiles(X, raw, (0.5,))
    with pytest.raises(_lib.AbcdezError, match=r"columns_histograms: the total mass reaches 2\^63"):
        ops.columns_histograms(X, raw, bins=4)
    with pytest.raises(_lib.AbcdezError, match=r"columns_wquantiles: p must be in \[0, 1\]"):
        ops.columns_wquantiles(X, None, (0.5, 1.5))
    with pytest.raises(_lib.AbcdezError, match="bins must be in 1 .. 4096"):
        ops.columns_histograms(X, None, bins=4097)
    with pytest.raises(_lib.AbcdezError, match="bins2 must be in 1 .. 128"):
        ops.columns_histograms(X, None, bins=4, pairs=[(0, 1)], bins2=129)
    bad = X.clone()
    bad[7, 2] = math.inf
    with pytest.raises(_lib.AbcdezError, match="columns_histograms: the automatic range of column 2 is not usable"):
        ops.columns_histograms(bad, None, bins=4)
    # the context still works
    assert ops.columns_moments(X, None)[4] == N


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


def sim_cases():
    return {
        "wiener": (A.Factored(A.Uniform(-2, 2), A.Uniform(0, 4)), A.WienerRMS(WIEN, blobs=True)),
        "socks": (A.Factored(A.NegativeBinomial(900 / 195, (900 / 195) / (30 + 900 / 195)), A.Beta(15, 2)), A.Socks(0, 11, blobs=True)),
        "mvn5": (A.Factored(*[A.Normal(0, 1)] * 5), A.MVNormal((1.0,) * 5, blobs=True)),       # blob width 8, n_blob 5
        "lv": (A.Factored(*[A.Uniform(0.0, 2.0)] * 4), A.LotkaVolterraRK4(LV_OBS, dt=0.05, steps_per_obs=10, blobs=True)),
        "user3": (A.Factored(A.Normal(0.0, 2.0), A.Normal(0.0, 2.0)), A.UserSimulator(USER_BLOB3, params=(0.5,), data=(1.0, -1.0), n_blob=3)),
    }


WIDTH = {"wiener": 8, "socks": 2, "mvn5": 5, "lv": 12, "user3": 3}


@pytest.mark.parametrize("abck", list(ABCKS))
@pytest.mark.parametrize("name", list(WIDTH))
def test_predictive_of_a_real_run_is_the_reference(name, abck):
    prior, sim = sim_cases()[name]
    N = 4096
    # four generations that resample once and end on a prologue: dead positions, and unequal weights for the Epanechnikov kernels.
    # The socks' distances are small integers: under a strict kernel a target of 0 leaves nobody alive, so that run aims at
    # distances below 2.5 and may reach them before the fourth generation.
    target = 2.5 if name == "socks" else 0.0
    r = A.abcdesmc(prior, sim, target, None, nparticles=N, α=0.6, δess=0.25, ABCk=ABCKS[abck], verbose=False, rng=5, max_iters=4)
    assert r.blobs.shape == (N, WIDTH[name])
    if name == "socks":                                 # (a run that resampled last has no weightless position)
        assert 2 <= r.iters <= 4
    else:
        assert r.iters == 4 and (r.Wns == 0).any()
    dev = r.engine.posterior_predictive(cov=True, wquantiles=PROBS, hist=HIST)
    ref = predictive_reference(r.blobs, r.Wns, cov=True, wquantiles=PROBS, hist=HIST)
    assert_same_record(dev, ref, (name, abck))
    assert dev.mean.shape == (WIDTH[name],) and np.isfinite(dev.mean).all()
    print(name, abck, "dead", int((r.Wns == 0).sum()), "distinct positive weights", np.unique(r.Wns[r.Wns > 0]).size)


def test_abcdemc_classic_storage_unit_weights():
    prior, sim = sim_cases()["wiener"]
    r = A.abcdemc(prior, sim, 0.5, None, nparticles=2049, generations=6, verbose=False, rng=8,
                  predictive=dict(cov=True, wquantiles=PROBS, hist=HIST))
    ref = predictive_reference(r.blobs, None, cov=True, wquantiles=PROBS, hist=HIST)
    assert_same_record(r.predictive, ref, "abcdemc")
    assert r.predictive.n_pos == 2049 and r.predictive.W == 2049.0


def test_driver_keyword_and_download_false():
    prior, sim = sim_cases()["lv"]
    kw = dict(nparticles=2049, α=0.6, δess=0.33, ABCk=A.Epa0toeps, verbose=False, rng=5, max_iters=3)
    r = A.abcdesmc(prior, sim, 0.0, None, predictive=True, **kw)
    assert_same_record(r.predictive, r.engine.posterior_predictive(), "predictive=True")
    assert_same_record(r.predictive, predictive_reference(r.blobs, r.Wns), "predictive=True, reference")
    bare = A.abcdesmc(prior, sim, 0.0, None, download=False, predictive=dict(wquantiles=(0.025, 0.5, 0.975)), **kw)
    assert bare.P is None and bare.blobs is None
    assert_same_record(bare.predictive, predictive_reference(r.blobs, r.Wns, wquantiles=(0.025, 0.5, 0.975)), "download=False")
    with pytest.raises(ValueError, match=r"predictive: needs a simulator that returns blobs \(blobs=True\)"):
        A.abcdesmc(prior, A.LotkaVolterraRK4(LV_OBS, dt=0.05, steps_per_obs=10), 0.0, None, predictive=True, **kw)


# ------------------------------------------------------------------------------------------ all four keywords in one driver call
ALL = dict(cov=True, wquantiles=PROBS, hist=dict(bins=7))
DRAWS = dict(n=257, draw=3)


def all_keywords_run(driver, N, engine=None, **kw):
    """One driver call with the download and ``summary``, ``sample``, ``predictive`` and ``adjust`` together (the path on which the
    four posterior calls share their tail and their blob rebuild): every record is the restatement of the downloaded result, bit
    for bit.  Normal1D with blobs: P and blobs are vectors.  Returns the driver's result."""
    from test_gpu_posterior_adjust import assert_same_adjusted

    sim = A.Normal1D(1.5, 1.0, blobs=True)
    r = driver(A.Normal(0.0, 2.0), sim, kw.pop("target"), None, nparticles=N, verbose=False, rng=5, engine=engine, summary=ALL,
               sample=DRAWS, predictive=ALL, adjust=dict(ALL, rows=True), **kw)
    Wns = vars(r).get("Wns")                             # abcdemc: no weights
    assert r.P.shape == r.C.shape == r.blobs.shape == (N,)
    assert_same_record(r.summary, summary_reference(r.P, Wns, **ALL), "summary")
    index, M, n_mass = sample_reference(r.P, Wns, DRAWS["n"], 5, DRAWS["draw"], rounds=r.engine.ops.stream_version()[1])
    ref = make_sample(r.P[index], index, r.C[index], r.blobs[index], M, n_mass, **DRAWS)
    assert r.sample.index.dtype == np.int64 and np.array_equal(r.sample.index, ref.index)
    assert (r.sample.M, r.sample.n_mass, r.sample.n, r.sample.draw) == (ref.M, ref.n_mass, ref.n, ref.draw)
    for f in ("P", "C", "blobs"):
        assert getattr(r.sample, f).shape == (DRAWS["n"],) and np.array_equal(bits(getattr(r.sample, f)), bits(getattr(ref, f))), f
    assert_same_record(r.predictive, predictive_reference(r.blobs, Wns, **ALL), "predictive")
    assert_same_adjusted(r.adjusted, adjust_reference(r.P, r.blobs, Wns, data=tuple(sim.data()), rows=True, **ALL), "adjust")
    return r


def test_all_four_keywords_in_one_call_packed_storage():
    """2049 particles: one tile of 2048 and one row"""
    r = all_keywords_run(A.abcdesmc, 2049, target=0.0, ABCk=A.Epa0toeps, max_iters=3)
    assert type(r.engine.ops) is HipOps and r.iters == 3 and (r.Wns == 0).any()


def test_all_four_keywords_in_one_call_classic_storage():
    r = all_keywords_run(A.abcdemc, 2049, target=0.5, generations=6)
    assert type(r.engine.ops) is HipOps and r.summary.n_pos == 2049


# ------------------------------------------------------------------------------------------ continuation
def test_a_resumed_run_is_bit_identical_after_a_predictive_summary():
    prior, sim = sim_cases()["mvn5"]
    kw = dict(nparticles=3001, α=0.6, δess=0.5, ABCk=A.Epa0toeps, verbose=False, rng=9)
    part = A.abcdesmc(prior, sim, 0.0, None, max_iters=3, **kw)
    p = part.engine.posterior_predictive(cov=True, wquantiles=PROBS, hist=HIST)
    assert_same_record(p, predictive_reference(part.blobs, part.Wns, cov=True, wquantiles=PROBS, hist=HIST), "stopped")
    rest = A.abcdesmc(prior, sim, 0.0, None, max_iters=6, resume=part.checkpoint(), **kw)
    full = A.abcdesmc(prior, sim, 0.0, None, max_iters=6, **kw)
    assert rest.iters == full.iters == 6 and rest.logZ == full.logZ and rest.nsims == full.nsims
    for f in ("P", "Wns", "C", "blobs"):
        assert np.array_equal(bits(getattr(rest, f)), bits(getattr(full, f))), f


def test_a_run_continued_on_the_same_engine_is_bit_identical():
    """two engines on the same key, the next generation's select enqueued ahead behind every group of sweeps; one is asked for the
    predictive summary between the generations (the five generations include resamplings)"""
    prior, sim = sim_cases()["wiener"]
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
                assert e.posterior_predictive(cov=True, wquantiles=PROBS, hist=HIST).n_mass >= 1
        e.discard_select_ahead()
    assert out[0] == out[1]
    assert engs[0].draw == engs[1].draw >= 1, "the run was meant to resample"
    a, b = engs[0].result(), engs[1].result()
    for f in ("P", "theta", "logpi", "C", "Wns", "alive", "blobs"):
        assert np.array_equal(a[f], b[f]), f
    assert engs[0].ops.smc_select_stats() == engs[1].ops.smc_select_stats()      # the selects enqueued ahead were all still used
