"""Posterior summaries on the device (abcdez_posterior_moments / abcdez_posterior_quantiles, csrc/abz_summary.hip) against the
numpy restatement of the same arithmetic (abcdez_amd.summary.summary_reference) on the downloaded P, Wns -- BIT FOR BIT: mean,
the unnormalised second central moments S, W, Q, n_pos, and the marginal quantiles.

The populations are runs stopped after three generations with alpha = 0.6 and delta_ess = 0.5: the second generation leaves
0.36 N alive and resamples, the third kills again -- so both row slots are in use, dead positions exist and hold stale rows."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import abcdez_amd as A
from abcdez_amd import _lib
from abcdez_amd.engine import HipOps, PopulationEngine
from abcdez_amd.summary import summary_reference

pytestmark = pytest.mark.gpu

PROBS = (0.0, 0.025, 0.5, 0.975, 1.0)


def model(d):
    if d == 1:
        return A.Normal(0.0, math.sqrt(10.0)), A.Normal1D(0.4)
    return A.Factored(*[A.Normal(0.0, 1.0) for _ in range(d)]), A.MVNormal(tuple([0.25] * d))


def run3(prior, sim, N, abck=A.IndicatorStrict0toϵ, iters=3, δess=0.5, engine=None):
    r = A.abcdesmc(prior, sim, 0.0, None, nparticles=N, α=0.6, δess=δess, ABCk=abck, verbose=False, rng=5, max_iters=iters,
                   engine=engine)
    assert r.iters == iters
    if iters >= 3:
        assert any(abs(e - N) <= 1e-9 * N for e in r.esss[1:]), "the run was meant to resample"
        assert (r.Wns == 0).any(), "the run was meant to leave dead positions"
    return r


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same(dev, ref, what):
    assert dev.n_pos == ref.n_pos, what
    for f in ("W", "Q"):
        assert bits(getattr(dev, f)) == bits(getattr(ref, f)), (what, f, getattr(dev, f), getattr(ref, f))
    assert np.array_equal(bits(dev.mean), bits(ref.mean)), (what, "mean", dev.mean, ref.mean)
    assert np.array_equal(bits(dev.S), bits(ref.S)), (what, "S", np.abs(dev.S - ref.S).max())
    assert np.array_equal(bits(dev.cov), bits(ref.cov)) and dev.ess == ref.ess, what
    assert dev.quantiles.shape == ref.quantiles.shape
    assert np.array_equal(bits(dev.quantiles), bits(ref.quantiles)), (what, "quantiles", dev.quantiles, ref.quantiles)


@pytest.mark.parametrize("N", [300, 2048, 5001])
@pytest.mark.parametrize("d", [1, 2, 3, 17, 32])
def test_packed_population_summary_is_the_reference_bit_for_bit(d, N):
    """d = 3, 17: rows padded to 4 / 32 doubles; d = 17, 32: rows spread over lanes in the sweeps; N = 300 / 2048 / 5001: part of a
    tile, exactly one, three with a ragged end"""
    prior, sim = model(d)
    r = run3(prior, sim, N)
    assert (np.asarray(r.P) < 0).any()                    # negative posterior mass: the select sees negative keys
    dev = r.engine.posterior_summary(cov=True, corrected=True, quantiles=PROBS)
    ref = summary_reference(r.P, r.Wns, cov=True, corrected=True, quantiles=PROBS)
    assert_same(dev, ref, (d, N))
    assert dev.mean.shape == (d,) and dev.cov.shape == (d, d) and dev.quantiles.shape == (len(PROBS), d)
    unc = r.engine.posterior_summary(cov=True, corrected=False)
    assert np.array_equal(bits(unc.cov), bits(ref.S / ref.W)) and unc.quantiles.shape == (0, d)
    first = r.engine.posterior_summary(cov=False)
    assert first.cov is None and np.array_equal(bits(first.mean), bits(ref.mean))


@pytest.mark.parametrize("abck", A.ALL_KERNELS, ids=lambda k: k.__name__)
def test_every_abc_kernel(abck):
    """the Epanechnikov kernels leave non-uniform weights: moments as for any weights, the unweighted quantile is refused.
    (Four generations with delta_ess = 0.25: with every kernel the third resamples and the fourth does not.)"""
    prior, sim = model(2)
    r = run3(prior, sim, 5001, abck=abck, iters=4, δess=0.25)
    live = r.Wns[r.Wns > 0]
    epa = "Epa" in abck.__name__
    assert (np.unique(live).size > 1) == epa
    if epa:
        assert_same(r.engine.posterior_summary(), summary_reference(r.P, r.Wns), abck.__name__)
        with pytest.raises(_lib.AbcdezError, match="weighted quantiles are not provided"):
            r.engine.posterior_summary(quantiles=(0.5,))
        with pytest.raises(ValueError, match="weighted quantiles are not provided"):
            summary_reference(r.P, r.Wns, quantiles=(0.5,))
    else:
        assert_same(r.engine.posterior_summary(quantiles=PROBS), summary_reference(r.P, r.Wns, quantiles=PROBS), abck.__name__)


def test_discrete_factor_is_rounded_by_push_p():
    prior, sim = A.Factored(A.Normal(1, 0.5), A.DiscreteUniform(1, 10)), A.NormalTimesDU(5.5)
    r = run3(prior, sim, 5001)
    res = r.engine.result()
    assert not np.array_equal(res["theta"][:, 1], r.P[:, 1]) and np.array_equal(r.P[:, 1], np.rint(r.P[:, 1]))
    assert_same(r.engine.posterior_summary(quantiles=PROBS), summary_reference(r.P, r.Wns, quantiles=PROBS), "normdu")


def test_crafted_column_with_signed_zeros_and_extremes():
    """a column uploaded through the checkpoint path: negative values, -0.0 next to +0.0, ties, denormals, large magnitudes"""
    prior, sim = model(2)
    r = run3(prior, sim, 5001)
    eng = r.engine
    st = eng.download_state()
    rng = np.random.default_rng(3)
    col = rng.choice(np.array([-0.0, 0.0, -1.0, 1.0, -5e-324, 5e-324, -1e150, 1e150, -2.5, 2.5, 1.0 + 2.0 ** -52]), 5001)
    col[:64] = np.repeat([-0.0, 0.0], 32)
    st["theta"] = st["theta"].copy()
    st["theta"][:, 0] = col
    eng.upload_state(st)
    res = eng.result()
    assert np.array_equal(bits(res["P"][:, 0]), bits(col))
    for probs in (PROBS, (0.3, 0.31, 0.5, 0.52)):
        assert_same(eng.posterior_summary(quantiles=probs), summary_reference(res["P"], res["Wns"], quantiles=probs), "crafted")


def test_abcdemc_classic_storage_unit_weights():
    prior, sim = model(3)
    m = A.abcdemc(prior, sim, 0.5, None, nparticles=4099, generations=6, verbose=False, rng=5, summary=dict(quantiles=PROBS))
    ref = summary_reference(m.P, None, quantiles=PROBS)
    assert_same(m.summary, ref, "abcdemc")
    assert ref.n_pos == 4099 and ref.W == 4099.0 and ref.Q == 4099.0
    m2 = A.abcdemc(prior, sim, 0.5, None, nparticles=4099, generations=6, verbose=False, rng=5, summary=True, download=False)
    assert m2.P is None and m2.C is None and np.array_equal(bits(m2.summary.mean), bits(ref.mean))


def test_driver_keywords_on_the_device():
    prior, sim = model(2)
    kw = dict(nparticles=2048, α=0.6, δess=0.5, verbose=False, rng=5, max_iters=3)
    r = A.abcdesmc(prior, sim, 0.0, None, summary=dict(quantiles=(0.025, 0.975)), **kw)
    assert_same(r.summary, summary_reference(r.P, r.Wns, quantiles=(0.025, 0.975)), "summary=")
    r2 = A.abcdesmc(prior, sim, 0.0, None, summary=True, download=False, **kw)
    assert r2.P is None and r2.Wns is None and r2.C is None and r2.logZ == r.logZ
    assert np.array_equal(bits(r2.summary.mean), bits(r.summary.mean)) and np.array_equal(bits(r2.summary.cov), bits(r.summary.cov))


def test_tree_level_two():
    """2^22 + 5 positions: 2049 tile partials per tree, so the finishing kernel runs level 1 and level 2"""
    prior, sim = model(2)
    r = run3(prior, sim, 2 ** 22 + 5, iters=2)
    assert_same(r.engine.posterior_summary(quantiles=PROBS), summary_reference(r.P, r.Wns, quantiles=PROBS), "2^22 + 5")


def test_a_run_continued_after_a_summary_is_bit_identical():
    """the stepwise engine calls of the driver loop (smc.py), the next generation's select enqueued ahead behind every group of
    sweeps; one engine is asked for a full summary between the generations"""
    prior, sim = model(3)
    spec = A.ModelSpec(prior, sim, A.IndicatorStrict0toϵ, seed=9)
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
            out[which].append((g["eps"], g["wnorm"], g["ess"], g["n_alive"], tuple(g["range"]), tuple(g["naccs"]), tuple(g["nsims"]), g["Ki"]))
            if which == 0:
                s = e.posterior_summary(quantiles=PROBS)
                assert s.n_pos >= 1
        e.discard_select_ahead()
    assert out[0] == out[1]
    a, b = engs[0].result(), engs[1].result()
    for f in ("P", "theta", "logpi", "C", "Wns", "alive"):
        assert np.array_equal(a[f], b[f]), f
    assert engs[0].ops.smc_select_stats() == engs[1].ops.smc_select_stats()      # the selects enqueued ahead were all still used
    assert_same(engs[0].posterior_summary(quantiles=PROBS), summary_reference(b["P"], b["Wns"], quantiles=PROBS), "continued")


def test_c_abi_refusals():
    prior, sim = model(2)
    r = run3(prior, sim, 300)
    e = r.engine
    lib, ctx, N = e.ops.lib, e.ops.ctx, e.N
    pop = (e.bits[e.bc].data_ptr(), N, e.buf[0][0].data_ptr(), e.buf[1][0].data_ptr())
    mean, S = np.zeros(2), np.zeros((2, 2))
    W, Q, n = C.c_double(), C.c_double(), C.c_int64()
    q, p_ok, p_bad = np.zeros(1), np.array([0.5]), np.array([1.5])

    def err(rc):
        assert rc != 0
        return lib.abcdez_last_error().decode()

    moments = lambda w, m: lib.abcdez_posterior_moments(ctx, pop[0], N, pop[2], pop[3], w, 1, m, S.ctypes.data, C.byref(W), C.byref(Q), C.byref(n))
    quant = lambda w, k, p: lib.abcdez_posterior_quantiles(ctx, pop[0], N, pop[2], pop[3], w, k, p.ctypes.data, 1, q.ctypes.data)
    wns = e.wns.data_ptr()
    assert moments(wns, mean.ctypes.data) == 0 and n.value == (r.Wns > 0).sum()
    assert "null argument" in err(moments(wns, None))
    assert "k must be in" in err(quant(wns, 2, p_ok)) and "k must be in" in err(quant(wns, -1, p_ok))
    assert "p must be in [0, 1]" in err(quant(wns, 0, p_bad))
    assert "N out of range" in err(lib.abcdez_posterior_moments(ctx, pop[0], 0, pop[2], pop[3], wns, 1, mean.ctypes.data, S.ctypes.data,
                                                               C.byref(W), C.byref(Q), C.byref(n)))
    zero = torch.zeros(N, dtype=torch.float64, device=e.device)
    assert "no particle has a positive weight" in err(moments(zero.data_ptr(), mean.ctypes.data))
    assert "no particle has a positive weight" in err(quant(zero.data_ptr(), 0, p_ok))
    assert quant(wns, 1, p_ok) == 0                        # and the context still works
    assert bits(q[0]) == bits(summary_reference(r.P, r.Wns, cov=False, quantiles=(0.5,)).quantiles[0, 1])
