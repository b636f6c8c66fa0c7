"""Weighted marginal quantiles on the device (abcdez_posterior_wquantiles, csrc/abz_wquantile.hip) against the literal restatement
of include/abcdez_spec.h ("posterior summaries", weighted quantiles) in abcdez_amd.summary.summary_reference -- BIT FOR BIT, with the
total integer mass M and n_mass.

Whole runs are stopped after a few generations with alpha = 0.6 (run3, as in test_gpu_posterior_summary.py): both row slots in use,
dead positions with stale rows; the Epanechnikov kernels leave unequal positive weights.  Crafted populations are handed to
HipOps.posterior_wquantiles as plain device tensors (bits, slot0, slot1, wns)."""
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
PROBS37 = tuple(float(p) for p in np.random.default_rng(37).permutation(np.r_[np.linspace(0.0, 1.0, 31), [0.5, 0.5, 0.025, 1.0, 0.0, 0.3]]))
NAN_BIG = np.array([np.nan, 1e300])


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


def assert_same_wq(dev, ref, what):
    assert dev.wquantiles.shape == ref.wquantiles.shape, what
    assert (dev.M, dev.n_mass) == (ref.M, ref.n_mass), (what, dev.M, ref.M, dev.n_mass, ref.n_mass)
    same = bits(dev.wquantiles) == bits(ref.wquantiles)
    assert same.all(), (what, np.argwhere(~same)[:5], dev.wquantiles[~same][:5], ref.wquantiles[~same][:5])
    assert dev.wprobs == ref.wprobs


def unequal_positive(w):
    return np.unique(w[w > 0]).size > 1


# ------------------------------------------------------------------------------------------ whole runs

@pytest.mark.parametrize("N", [300, 2048, 5001])
@pytest.mark.parametrize("d", [1, 3, 17, 32])
def test_epanechnikov_runs_are_the_reference_bit_for_bit(d, N):
    prior, sim = model(d)
    r = run3(prior, sim, N, abck=A.Epa0toϵ, δess=0.33)       # ess / N = 1, 0.4 .. 0.5, 1 (resampled), 0.47 .. 0.52 at every shape
    assert unequal_positive(r.Wns)
    dev = r.engine.posterior_summary(cov=False, wquantiles=PROBS)
    ref = summary_reference(r.P, r.Wns, cov=False, wquantiles=PROBS)
    assert_same_wq(dev, ref, (d, N))
    assert dev.wquantiles.shape == (len(PROBS), d) and dev.quantiles.shape == (0, d)
    assert np.array_equal(bits(dev.mean), bits(ref.mean)) and dev.n_pos == ref.n_pos >= dev.n_mass


@pytest.mark.parametrize("abck", A.ALL_KERNELS, ids=lambda k: k.__name__)
def test_every_abc_kernel(abck):
    prior, sim = model(2)
    r = run3(prior, sim, 5001, abck=abck, iters=4, δess=0.25)
    assert unequal_positive(r.Wns) == ("Epa" in abck.__name__)
    dev = r.engine.posterior_summary(wquantiles=PROBS)
    assert_same_wq(dev, summary_reference(r.P, r.Wns, wquantiles=PROBS), abck.__name__)


def test_the_refusal_of_quantiles_stays_and_wquantiles_works_on_the_same_engine():
    prior, sim = model(2)
    r = run3(prior, sim, 2048, abck=A.EpaStrict0toϵ, iters=4, δess=0.25)
    assert unequal_positive(r.Wns)
    with pytest.raises(_lib.AbcdezError, match="weighted quantiles are not provided"):
        r.engine.posterior_summary(quantiles=(0.5,))
    with pytest.raises(ValueError, match="weighted quantiles are not provided"):
        summary_reference(r.P, r.Wns, quantiles=(0.5,))
    dev = r.engine.posterior_summary(wquantiles=(0.5,))
    assert_same_wq(dev, summary_reference(r.P, r.Wns, wquantiles=(0.5,)), "same engine")
    assert np.isfinite(dev.wquantiles).all()


def test_driver_keyword_reaches_the_device():
    prior, sim = model(3)
    kw = dict(nparticles=2048, α=0.6, δess=0.33, ABCk=A.Epa0toϵ, verbose=False, rng=5, max_iters=3)
    r = A.abcdesmc(prior, sim, 0.0, None, summary=dict(cov=False, wquantiles=(0.025, 0.975)), **kw)
    assert unequal_positive(r.Wns)
    assert_same_wq(r.summary, summary_reference(r.P, r.Wns, cov=False, wquantiles=(0.025, 0.975)), "summary=")
    r2 = A.abcdesmc(prior, sim, 0.0, None, summary=dict(wquantiles=(0.025, 0.975)), download=False, **kw)
    assert r2.P is None and np.array_equal(bits(r2.summary.wquantiles), bits(r.summary.wquantiles))


def test_abcdemc_classic_storage_no_weights():
    prior, sim = model(3)
    N = 4099
    m = A.abcdemc(prior, sim, 0.5, None, nparticles=N, generations=6, verbose=False, rng=5,
                  summary=dict(quantiles=PROBS37, wquantiles=PROBS37))
    ref = summary_reference(m.P, None, quantiles=PROBS37, wquantiles=PROBS37)
    assert_same_wq(m.summary, ref, "abcdemc")
    assert ref.n_mass == N and ref.M == N << 40
    rng_ = m.P.max(axis=0) - m.P.min(axis=0)
    assert (np.abs(m.summary.wquantiles - m.summary.quantiles) <= 2.0 ** -38 * rng_).all()


def test_a_run_continued_after_wquantiles_is_bit_identical():
    """two engines on the same key, the next generation's select enqueued ahead; one is asked between the generations"""
    prior, sim = model(3)
    spec = A.ModelSpec(prior, sim, A.Epa0toϵ, seed=9)
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
                assert e.posterior_summary(cov=False, wquantiles=PROBS).n_mass >= 1
        e.discard_select_ahead()
    assert out[0] == out[1]
    a, b = engs[0].result(), engs[1].result()
    for f in ("P", "theta", "logpi", "C", "Wns", "alive"):
        assert np.array_equal(a[f], b[f]), f
    assert engs[0].ops.smc_select_stats() == engs[1].ops.smc_select_stats()
    assert_same_wq(engs[0].posterior_summary(wquantiles=PROBS), summary_reference(b["P"], b["Wns"], wquantiles=PROBS), "continued")


# ------------------------------------------------------------------------------------------ crafted populations

@pytest.fixture(scope="module")
def ops_of():
    made = {}

    def get(d):
        if d not in made:
            prior, sim = model(d)
            spec = A.ModelSpec(prior, sim, A.Epa0toϵ, seed=1)
            made[d] = (spec, HipOps(spec))
        return made[d]
    yield get
    for _, ops in made.values():
        ops.close()


def crafted(spec, ops, values, weights, rng):
    """upload (values N x d, weights N) as a packed population: a random half of the bits set, the slot that is not current and
    both slots of a position with w <= 0 hold NaN / 1e300.  -> (device tuple, P with the dead rows poisoned)"""
    N, d = values.shape
    ld = ops.layout()[0]
    live = weights > 0.0
    bit = rng.random(N) < 0.5
    if N > 1:
        bit[:2] = (False, True)
    slots = [np.zeros((N, ld)), np.zeros((N, ld))]
    poison = np.resize(NAN_BIG, (N, d))
    for s in (0, 1):
        cur = live & (bit == bool(s))
        slots[s][:, :d] = np.where(cur[:, None], values, poison)
    words = np.zeros((N + 31) // 32, dtype=np.uint32)
    idx = np.flatnonzero(bit)
    np.bitwise_or.at(words, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    dev = ops.device
    pop = (torch.from_numpy(words.view(np.int32)).to(dev), torch.from_numpy(slots[0]).to(dev), torch.from_numpy(slots[1]).to(dev),
           torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float64)).to(dev))
    return pop, np.where(live[:, None], values, poison)


def check_crafted(ops_of, d, values, weights, probs=PROBS, k0=0, nk=None, seed=0):
    spec, ops = ops_of(d)
    values = np.ascontiguousarray(values, dtype=np.float64).reshape(len(weights), d)
    pop, P = crafted(spec, ops, values, np.asarray(weights, dtype=np.float64), np.random.default_rng(seed))
    N = len(weights)
    q, M, n_mass = ops.posterior_wquantiles(*pop, N, probs, k0=k0, nk=nk)
    nk = d - k0 if nk is None else nk
    assert q.shape == (nk, len(probs))
    ref = summary_reference(P[:, k0:k0 + nk], weights, cov=False, wquantiles=probs)
    same = bits(q.T) == bits(ref.wquantiles)
    assert (M, n_mass) == (ref.M, ref.n_mass) and same.all(), (M, ref.M, n_mass, ref.n_mass, q.T[~same][:5], ref.wquantiles[~same][:5])
    return ref


def dyadic_weights(rng, N, dead=0.3):
    """k / 2^20 normalised by a power of two; a share of exact zeros"""
    k = rng.integers(1, 1 << 20, N).astype(np.float64)
    k[rng.random(N) < dead] = 0.0
    k[0] = max(k[0], 1.0)
    return k / 2.0 ** math.ceil(math.log2(k.sum()))


@pytest.mark.parametrize("N", [300, 2048, 5001])
def test_both_slots_and_poisoned_dead_rows(ops_of, N):
    rng = np.random.default_rng(N)
    ref = check_crafted(ops_of, 3, rng.standard_normal((N, 3)), dyadic_weights(rng, N), seed=N)
    assert np.isfinite(ref.wquantiles).all() and ref.n_mass < N


def test_ties_signed_zeros_and_a_massless_positive_weight(ops_of):
    """the edge cases of test_posterior_wquantiles_reference.py on the device"""
    # ties with different masses: the crossing in the first element of a tie group (p = 0.5 of the worked case) and not in it
    check_crafted(ops_of, 1, [2.0, 1.0, 2.0, 4.0], [0.125, 0.25, 0.125, 0.5], probs=(0.0, 0.3, 0.5, 0.55, 0.6, 0.7, 1.0))
    check_crafted(ops_of, 1, [2.0, 1.0, 2.0, 4.0, 2.0], [0.25, 0.125, 0.125, 0.25, 0.25], probs=tuple(np.linspace(0, 1, 33)))
    # -0.0 next to +0.0
    check_crafted(ops_of, 1, [0.0, -0.0, 1.0, -0.0, 0.0, -1.0], [0.125, 0.25, 0.125, 0.125, 0.125, 0.25], probs=tuple(np.linspace(0, 1, 17)))
    # a weight of 2^-70 is positive and carries no mass
    w = np.array([0.5, 2.0 ** -70, 0.25, 0.0, 0.25])
    ref = check_crafted(ops_of, 1, [3.0, -7.0, 1.0, 9.0, 2.0], w)
    assert ref.n_mass == 3 < (w > 0).sum() and ref.wquantiles.min() == 1.0
    # all mass on one position; n_mass = 1
    ref = check_crafted(ops_of, 1, [3.0, -0.0, 1.0], [0.0, 1.0, 0.0])
    assert ref.n_mass == 1 and np.signbit(ref.wquantiles).all()
    ref = check_crafted(ops_of, 1, [3.0, 5.0, 1.0], [2.0 ** -70, 1.0, 2.0 ** -70])
    assert ref.n_mass == 1 and (ref.wquantiles == 5.0).all()


def test_denormals_extremes_and_a_constant_column(ops_of):
    N = 5001
    rng = np.random.default_rng(3)
    vals = rng.standard_normal((N, 3))
    vals[:, 0] = rng.choice(np.array([-0.0, 0.0, -1.0, 1.0, -5e-324, 5e-324, -1e150, 1e150, -2.5, 2.5, 1.0 + 2.0 ** -52]), N)
    vals[:, 1] = -1.75
    check_crafted(ops_of, 3, vals, dyadic_weights(rng, N), probs=PROBS37, seed=1)


@pytest.mark.parametrize("d,k0,nk", [(17, 5, 12), (17, 16, 1), (3, 1, 2), (3, 2, 1)])
def test_a_sub_range_of_the_columns(ops_of, d, k0, nk):
    N = 2048 + 77
    rng = np.random.default_rng(d * 100 + k0)
    assert ops_of(d)[1].layout()[0] == {17: 32, 3: 4}[d]
    check_crafted(ops_of, d, rng.standard_normal((N, d)), dyadic_weights(rng, N), k0=k0, nk=nk, seed=2)


def test_more_probabilities_than_one_batch(ops_of):
    N = 5001
    rng = np.random.default_rng(37)
    assert len(PROBS37) == 37 and list(PROBS37) != sorted(PROBS37) and len(set(PROBS37)) < 37
    check_crafted(ops_of, 17, rng.standard_normal((N, 17)), dyadic_weights(rng, N), probs=PROBS37, seed=3)


def test_refusals(ops_of):
    spec, ops = ops_of(3)
    N = 300
    rng = np.random.default_rng(0)
    vals = rng.standard_normal((N, 3))
    pop, _ = crafted(spec, ops, vals, np.full(N, 1.0 / N), rng)
    call = lambda w, probs=(0.5,), **kw: ops.posterior_wquantiles(pop[0], pop[1], pop[2], w, N, probs, **kw)
    dev = ops.device
    with pytest.raises(_lib.AbcdezError, match="not normalised"):
        call(torch.full((N,), 1e6, dtype=torch.float64, device=dev))
    with pytest.raises(_lib.AbcdezError, match="no particle has a positive weight"):
        call(torch.full((N,), 2.0 ** -70, dtype=torch.float64, device=dev))
    with pytest.raises(_lib.AbcdezError, match="no particle has a positive weight"):
        call(torch.zeros(N, dtype=torch.float64, device=dev))
    with pytest.raises(_lib.AbcdezError, match=r"p must be in \[0, 1\]"):
        call(pop[3], probs=(1.5,))
    with pytest.raises(_lib.AbcdezError, match="k0 \\+ nk <= length"):
        call(pop[3], k0=2, nk=2)
    with pytest.raises(_lib.AbcdezError, match="nk >= 1"):
        call(pop[3], k0=0, nk=0)
    q, M, n_mass = call(pop[3])                             # and the context still works; wns == NULL is w_i = 1 / N
    q0, M0, n0 = call(None)
    assert (M, n_mass) == (M0, n0) == (N << 40, N)
    assert np.array_equal(bits(q), bits(q0)) and np.array_equal(bits(q0), bits(summary_reference(vals, None, cov=False, wquantiles=(0.5,)).wquantiles.T))
