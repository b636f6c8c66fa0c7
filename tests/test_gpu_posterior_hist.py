"""Marginal and pairwise histograms on the device (abcdez_posterior_histograms, csrc/abz_hist.hip) against the literal restatement of
include/abcdez_spec.h ("posterior summaries", histograms) in abcdez_amd.summary.summary_reference(..., hist=): every mass and tally
EXACTLY, lo / hi bitwise.

Whole runs are stopped after a few generations with alpha = 0.6 (run3, as in test_gpu_posterior_wquantiles.py): both row slots in
use, dead positions with stale rows; the Epanechnikov kernels leave unequal positive weights.  Crafted populations are handed to
HipOps.posterior_histograms as plain device tensors (bits, slot0, slot1, wns)."""
import math

import numpy as np
import pytest
import torch

import abcdez_amd as A
from abcdez_amd import _lib
from abcdez_amd.engine import HipOps, PopulationEngine
from abcdez_amd.summary import hist_options, hist_reference, make_hist, summary_reference

pytestmark = pytest.mark.gpu

NAN_BIG = np.array([np.nan, 1e300])
HIST = dict(bins=37, pairs="all", bins2=16)


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


def assert_same_hist(dev, ref, what=""):
    assert (dev.M, dev.n_mass) == (ref.M, ref.n_mass), (what, dev.M, ref.M, dev.n_mass, ref.n_mass)
    assert dev.columns == ref.columns and dev.pairs == ref.pairs and dev.bins == ref.bins and dev.bins2 == ref.bins2, what
    assert np.array_equal(bits(dev.lo), bits(ref.lo)) and np.array_equal(bits(dev.hi), bits(ref.hi)), (what, dev.lo, ref.lo, dev.hi, ref.hi)
    for f in ("mass1", "under", "over", "nan", "mass2", "outside2"):
        a, b = getattr(dev, f), getattr(ref, f)
        assert a.dtype == np.uint64 and a.shape == b.shape, (what, f, a.shape, b.shape)
        assert np.array_equal(a, b), (what, f, np.argwhere(a != b)[:5], a[a != b][:5], b[a != b][:5])
    assert np.array_equal(bits(dev.edges), bits(ref.edges))


def assert_identities(h):
    assert ((h.mass1.sum(axis=1) + h.under + h.over + h.nan) == np.uint64(h.M)).all()
    if h.pairs:
        assert ((h.mass2.sum(axis=(1, 2)) + h.outside2) == np.uint64(h.M)).all()


def unequal_positive(w):
    return np.unique(w[w > 0]).size > 1


# ------------------------------------------------------------------------------------------ whole runs

@pytest.mark.parametrize("N", [300, 2048, 5001])
@pytest.mark.parametrize("d", [1, 3, 17, 32])
def test_epanechnikov_runs_are_the_reference_exactly(d, N):
    prior, sim = model(d)
    r = run3(prior, sim, N, abck=A.Epa0toϵ, δess=0.33)
    assert unequal_positive(r.Wns)
    opts = dict(HIST) if d > 1 else dict(bins=37)
    dev = r.engine.posterior_summary(cov=False, hist=opts)
    ref = summary_reference(r.P, r.Wns, cov=False, hist=opts)
    assert_same_hist(dev.hist, ref.hist, (d, N))
    assert_identities(dev.hist)
    assert len(dev.hist.pairs) == d * (d - 1) // 2 and dev.hist.mass1.shape == (d, 37)
    assert (dev.M, dev.n_mass) == (ref.M, ref.n_mass) and np.array_equal(bits(dev.mean), bits(ref.mean))


@pytest.mark.parametrize("abck", A.ALL_KERNELS, ids=lambda k: k.__name__)
def test_every_abc_kernel(abck):
    prior, sim = model(2)
    r = run3(prior, sim, 5001, abck=abck, iters=4, δess=0.25)
    assert unequal_positive(r.Wns) == ("Epa" in abck.__name__)
    dev = r.engine.posterior_summary(hist=HIST)
    assert_same_hist(dev.hist, summary_reference(r.P, r.Wns, hist=HIST).hist, abck.__name__)


def test_lo_hi_are_the_extreme_wquantiles_and_the_marginals_are_consistent():
    prior, sim = model(3)
    r = run3(prior, sim, 5001, abck=A.Epa0toϵ, δess=0.33)
    s = r.engine.posterior_summary(cov=False, wquantiles=(0.0, 1.0), hist=dict(bins=16, pairs="all", bins2=16))
    h = s.hist
    assert np.array_equal(bits(h.lo), bits(s.wquantiles[0])) and np.array_equal(bits(h.hi), bits(s.wquantiles[1])) and (h.lo < h.hi).all()
    assert (h.under == 0).all() and (h.over == 0).all() and (h.nan == 0).all() and (h.outside2 == 0).all()
    for q, (j, k) in enumerate(h.pairs):
        assert np.array_equal(h.mass2[q].sum(axis=1), h.mass1[j]) and np.array_equal(h.mass2[q].sum(axis=0), h.mass1[k])
    assert np.allclose((h.density() * ((h.hi - h.lo) / 16)[:, None]).sum(axis=1), 1.0)


def test_driver_keyword_reaches_the_device_and_download_false():
    prior, sim = model(3)
    kw = dict(nparticles=2048, α=0.6, δess=0.33, ABCk=A.Epa0toϵ, verbose=False, rng=5, max_iters=3)
    opts = dict(bins=20, range=(-1.0, 1.5), pairs=[(0, 2)], bins2=7)
    r = A.abcdesmc(prior, sim, 0.0, None, summary=dict(cov=False, hist=opts), **kw)
    assert unequal_positive(r.Wns)
    assert_same_hist(r.summary.hist, summary_reference(r.P, r.Wns, cov=False, hist=opts).hist, "summary=")
    assert r.summary.hist.under.min() > 0 and r.summary.hist.outside2.min() > 0
    r2 = A.abcdesmc(prior, sim, 0.0, None, summary=dict(hist=opts), download=False, **kw)
    assert r2.P is None
    assert_same_hist(r2.summary.hist, r.summary.hist, "download=False")


def test_abcdemc_classic_storage_no_weights():
    prior, sim = model(3)
    N = 4099
    m = A.abcdemc(prior, sim, 0.5, None, nparticles=N, generations=6, verbose=False, rng=5, summary=dict(hist=HIST))
    ref = summary_reference(m.P, None, hist=HIST)
    assert_same_hist(m.summary.hist, ref.hist, "abcdemc")
    h = m.summary.hist
    assert h.n_mass == N and h.M == N << 40 and (h.mass1 % np.uint64(1 << 40) == 0).all() and (h.mass2 % np.uint64(1 << 40) == 0).all()
    assert ((h.mass1 >> np.uint64(40)).sum(axis=1) == N).all() and ((h.mass2 >> np.uint64(40)).sum(axis=(1, 2)) == N).all()
    m2 = A.abcdemc(prior, sim, 0.5, None, nparticles=N, generations=6, verbose=False, rng=5, summary=dict(hist=HIST), download=False)
    assert m2.P is None
    assert_same_hist(m2.summary.hist, h, "abcdemc download=False")


def test_a_run_continued_after_histograms_is_bit_identical():
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
                assert e.posterior_summary(cov=False, hist=HIST).hist.n_mass >= 1
        e.discard_select_ahead()
    assert out[0] == out[1]
    a, b = engs[0].result(), engs[1].result()
    for f in ("P", "theta", "logpi", "C", "Wns", "alive"):
        assert np.array_equal(a[f], b[f]), f
    assert engs[0].ops.smc_select_stats() == engs[1].ops.smc_select_stats()
    assert_same_hist(engs[0].posterior_summary(hist=HIST).hist, summary_reference(b["P"], b["Wns"], hist=HIST).hist, "continued")


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


def crafted(spec, ops, values, weights, rng, live=None):
    """upload (values N x d, weights N) as a packed population: a random half of the bits set, the slot that is not current and
    both slots of a position that is not ``live`` (default: w <= 0) hold NaN / 1e300.  -> (device tuple, P with those rows poisoned)"""
    N, d = values.shape
    ld = ops.layout()[0]
    live = weights > 0.0 if live is None else live
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


def device_hist(ops, pop, N, d, opts):
    cols, nbins, rng_, pairs, bins2 = hist_options(opts, d)
    out = ops.posterior_histograms(*pop, N, columns=cols, bins=nbins, range=rng_, pairs=pairs, bins2=bins2)
    return make_hist(cols, nbins, out[0], out[1], out[2], pairs, bins2, out[3], out[4], out[5], out[6])


def check_crafted(ops_of, d, values, weights, opts, seed=0, live=None):
    spec, ops = ops_of(d)
    weights = np.asarray(weights, dtype=np.float64)
    values = np.ascontiguousarray(values, dtype=np.float64).reshape(len(weights), d)
    pop, P = crafted(spec, ops, values, weights, np.random.default_rng(seed), live)
    dev = device_hist(ops, pop, len(weights), d, opts)
    ref = hist_reference(P, weights, **opts)
    assert_same_hist(dev, ref, opts)
    assert_identities(dev)
    return dev


def dyadic_weights(rng, N, dead=0.3):
    """k / 2^20 normalised by a power of two; a share of exact zeros"""
    k = rng.integers(1, 1 << 20, N).astype(np.float64)
    k[rng.random(N) < dead] = 0.0
    k[0] = max(k[0], 1.0)
    return k / 2.0 ** math.ceil(math.log2(k.sum()))


@pytest.mark.parametrize("N", [300, 2048, 5001])
def test_both_slots_and_poisoned_dead_rows(ops_of, N):
    """were a dead row ever read, the automatic range would be NaN / 1e300 (a refusal, or a wrecked lo / hi)"""
    rng = np.random.default_rng(N)
    h = check_crafted(ops_of, 3, rng.standard_normal((N, 3)), dyadic_weights(rng, N), HIST, seed=N)
    assert h.n_mass < N and (h.nan == 0).all() and np.isfinite(h.lo).all() and (h.hi < 10).all()
    # a positive weight without mass is not read either: its row is poisoned although w > 0
    w = dyadic_weights(rng, N)
    massless = rng.random(N) < 0.1
    massless[0] = False
    w[massless] = 2.0 ** -70
    h = check_crafted(ops_of, 3, rng.standard_normal((N, 3)), w, HIST, seed=N + 1, live=(w > 0) & ~massless)
    assert h.n_mass == ((w > 0) & ~massless).sum() < (w > 0).sum() and (h.nan == 0).all() and (h.hi < 10).all()


def test_values_on_edges_signed_zeros_denormals_and_extremes(ops_of):
    N = 5001
    rng = np.random.default_rng(3)
    w = dyadic_weights(rng, N)
    vals = rng.standard_normal((N, 3))
    vals[:, 0] = rng.integers(0, 33, N) / 4.0                                   # on every edge of 8 bins over (0, 8), and on hi
    vals[:, 1] = rng.choice(np.array([-0.0, 0.0, -1.0, 1.0, -5e-324, 5e-324, -1e150, 1e150, -2.5, 2.5, 1.0 + 2.0 ** -52]), N)
    vals[:, 2] = -1.75
    h = check_crafted(ops_of, 3, vals, w, dict(bins=8, range=[(0.0, 8.0), (0.0, 1.0), (-2.0, -1.5)], pairs="all", bins2=8), seed=1)
    assert h.over[0] == 0 and h.under[0] == 0 and (h.mass1[0] > 0).all()                  # hi itself is in the last bin
    assert h.under[1] > 0 and h.over[1] > 0 and h.mass1[1][0] > 0 and (h.outside2 > 0).any()
    h = check_crafted(ops_of, 3, vals, w, dict(bins=33, pairs="all", bins2=33), seed=2)    # automatic: (0, 8), (-1e150, 1e150), -1.75 +- 0.5
    assert (h.lo[2], h.hi[2]) == (-2.25, -1.25) and (h.lo[1], h.hi[1]) == (-1e150, 1e150) and (h.lo[0], h.hi[0]) == (0.0, 8.0)
    # only signed zeros: the automatic range is (-0.0, +0.0), equal as doubles
    z = np.where(rng.random((300, 1)) < 0.5, 0.0, -0.0)
    h = check_crafted(ops_of, 1, z, np.full(300, 1.0 / 300), dict(bins=4))
    assert (h.lo[0], h.hi[0]) == (-0.5, 0.5) and h.mass1[0][2] == h.M
    h = check_crafted(ops_of, 1, z, np.full(300, 1.0 / 300), dict(bins=4, range=(0.0, 1.0)))
    assert h.under[0] == 0 and h.mass1[0][0] == h.M                              # -0.0 with lo = +0.0 is in bin 0


def test_a_nan_in_a_counting_row(ops_of):
    N = 2048
    rng = np.random.default_rng(5)
    w = dyadic_weights(rng, N, dead=0.0)
    vals = rng.standard_normal((N, 3))
    vals[[7, 1500], 1] = np.nan
    h = check_crafted(ops_of, 3, vals, w, dict(bins=10, range=(-3.0, 3.0), pairs="all", bins2=6), seed=4)
    assert h.nan.tolist() == [0, int(h.nan[1]), 0] and h.nan[1] > 0 and h.outside2[0] >= h.nan[1]
    spec, ops = ops_of(3)
    pop, P = crafted(spec, ops, vals, w, np.random.default_rng(4))
    with pytest.raises(_lib.AbcdezError, match="automatic range of column 1 .*pass a range"):
        ops.posterior_histograms(*pop, N, bins=10)
    with pytest.raises(ValueError, match="automatic range of column 1 .*pass a range"):
        hist_reference(P, w, bins=10)
    vals[7, 1] = np.inf
    vals[1500, 1] = 0.0
    pop, P = crafted(spec, ops, vals, w, np.random.default_rng(4))
    with pytest.raises(_lib.AbcdezError, match="automatic range of column 1 .*pass a range"):
        ops.posterior_histograms(*pop, N, bins=10)
    assert_same_hist(device_hist(ops, pop, N, 3, dict(bins=10, columns=[0, 2])), hist_reference(P, w, bins=10, columns=[0, 2]), "other columns")


@pytest.mark.parametrize("opts", [dict(bins=1, pairs="all", bins2=1), dict(bins=4096, pairs="all", bins2=128),
                                  dict(bins=4095, pairs="all", bins2=91), dict(bins=64, pairs="all", bins2=90),
                                  dict(bins=2, pairs="all", bins2=23)], ids=lambda o: "%d-%d" % (o["bins"], o["bins2"]))
def test_smallest_and_largest_bin_counts(ops_of, opts):
    """bins2 = 128 and 91 cut a pair's cell space into two row ranges, 90 is the largest that fits one, 23 the smallest with
    fewer than 16 pairs a batch"""
    N = 5001
    rng = np.random.default_rng(opts["bins"])
    h = check_crafted(ops_of, 3, rng.standard_normal((N, 3)), dyadic_weights(rng, N), opts, seed=6)
    assert h.mass2.shape == (3, opts["bins2"], opts["bins2"])
    for q, (j, k) in enumerate(h.pairs):
        assert h.mass2[q].sum() == np.uint64(h.M)


def test_a_column_subset_and_an_explicit_pair_list(ops_of):
    N = 2048 + 77
    rng = np.random.default_rng(17)
    assert ops_of(17)[1].layout()[0] == 32
    vals, w = rng.standard_normal((N, 17)), dyadic_weights(rng, N)
    pairs = [(11, 16), (2, 5), (5, 16), (2, 16), (5, 11)]
    h = check_crafted(ops_of, 17, vals, w, dict(bins=19, columns=[16, 2, 5, 11], pairs=pairs, bins2=9), seed=2)
    assert h.columns == (2, 5, 11, 16) and h.pairs == tuple(pairs)
    check_crafted(ops_of, 17, vals, w, dict(bins=19, columns=[16], range=(-1.0, 0.0)), seed=2)
    # a per-column range follows the columns as given: each column is shifted, so a range applied to another column leaves nothing in it
    shifted = vals + 10.0 * np.arange(17)
    ranges = {k: (10.0 * k - 1.0 - 0.01 * k, 10.0 * k + 1.5) for k in range(17)}
    order = [16, 2, 5, 11]
    h = check_crafted(ops_of, 17, shifted, w, dict(bins=19, columns=order, range=[ranges[k] for k in order], pairs=pairs, bins2=9), seed=2)
    assert h.columns == (2, 5, 11, 16) and [(a, b) for a, b in zip(h.lo, h.hi)] == [ranges[k] for k in h.columns]
    assert (h.mass1.sum(axis=1) > np.uint64(h.M // 2)).all() and (h.under > 0).all() and (h.over > 0).all() and (h.outside2 < np.uint64(h.M // 2)).all()
    spec, ops = ops_of(17)
    pop, P = crafted(spec, ops, shifted, w, np.random.default_rng(2))
    r_ = np.array([ranges[k] for k in h.columns])                        # the raw call takes sorted columns with their ranges
    raw = ops.posterior_histograms(*pop, N, columns=list(h.columns), bins=19, range=r_)
    assert np.array_equal(raw[1], h.mass1) and np.array_equal(bits(raw[0]), bits(r_))
    check_crafted(ops_of, 17, vals, w, dict(bins=5, columns=[0, 16], range=[(-1.0, 0.0), (0.0, 2.0)], pairs="all", bins2=128), seed=2)


def test_refusals_leave_the_context_working(ops_of):
    spec, ops = ops_of(3)
    N = 300
    rng = np.random.default_rng(0)
    vals = rng.standard_normal((N, 3))
    pop, _ = crafted(spec, ops, vals, np.full(N, 1.0 / N), rng)
    call = lambda w, **kw: ops.posterior_histograms(pop[0], pop[1], pop[2], w, N, **kw)
    dev = ops.device
    with pytest.raises(_lib.AbcdezError, match="not normalised"):
        call(torch.full((N,), 1e6, dtype=torch.float64, device=dev))
    with pytest.raises(_lib.AbcdezError, match="no particle has a positive weight"):
        call(torch.full((N,), 2.0 ** -70, dtype=torch.float64, device=dev))
    with pytest.raises(_lib.AbcdezError, match="no particle has a positive weight"):
        call(torch.zeros(N, dtype=torch.float64, device=dev))
    for bad, msg in ((dict(bins=0), "bins must be in 1 .. 4096"), (dict(bins=4097), "bins must be in 1 .. 4096"),
                     (dict(pairs=[(0, 1)], bins2=0), "bins2 must be in 1 .. 128"), (dict(pairs=[(0, 1)], bins2=129), "bins2 must be in 1 .. 128"),
                     (dict(pairs=[(1, 0)]), "j < k"), (dict(pairs=[(0, 1), (1, 2), (0, 1)]), "listed twice"), (dict(pairs=[(1, 1)]), "j < k"), (dict(pairs=[(0, 3)]), "j < k"),
                     (dict(columns=[0, 2], pairs=[(0, 1)]), "among the requested columns"), (dict(columns=[2, 0]), "strictly increasing"),
                     (dict(columns=[0, 3]), "strictly increasing"), (dict(range=[(0, 1), (1, 1), (0, 1)]), "lo < hi"),
                     (dict(range=[(0, 1), (0, np.inf), (0, 1)]), "lo < hi"), (dict(range=[(0, 1), (-1e308, 1e308), (0, 1)]), "hi - lo finite")):
        with pytest.raises(_lib.AbcdezError, match=msg):
            call(pop[3], **bad)
    spec1, ops1 = ops_of(1)
    pop1, _ = crafted(spec1, ops1, vals[:, :1], np.full(N, 1.0 / N), rng)
    with pytest.raises(_lib.AbcdezError, match="j < k|at least two parameters"):
        ops1.posterior_histograms(*pop1, N, pairs=[(0, 1)])
    out, out0 = call(pop[3], bins=9, pairs=[(0, 2)], bins2=4), call(None, bins=9, pairs=[(0, 2)], bins2=4)   # wns == NULL is w_i = 1 / N
    assert out[5:] == out0[5:] == (N << 40, N)
    ref = hist_reference(vals, None, bins=9, pairs=[(0, 2)], bins2=4)
    for a, b in zip(out[:5], out0[:5]):
        assert np.array_equal(a, b)
    assert np.array_equal(out[1], ref.mass1) and np.array_equal(out[3], ref.mass2) and np.array_equal(bits(out[0][:, 0]), bits(ref.lo))
