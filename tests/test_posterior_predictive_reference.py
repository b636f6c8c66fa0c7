"""The posterior predictive summary without a GPU: the options of the ``predictive=`` keyword, the numpy restatement
(abcdez_amd.summary.predictive_reference: summary_reference of the simulated data under the population's weights) against values
computed by hand, and the drivers' keyword on the CPU test engine, which computes the restatement on its downloaded blobs."""
import math

import numpy as np
import pytest

import abcdez_amd as A
from abcdez_amd.summary import predictive_options, predictive_reference, summary_reference, weight_fix


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_predictive_options_accepts_and_refuses():
    assert predictive_options(True) == {}
    opts = dict(cov=True, corrected=False, wquantiles=(0.1, 0.9), hist=dict(bins=8))
    got = predictive_options(opts)
    assert got == opts and got is not opts
    assert predictive_options({}) == {}
    with pytest.raises(ValueError, match=r"unknown option\(s\) \['quantiles'\]"):
        predictive_options(dict(quantiles=(0.5,)))                 # the unweighted quantiles are not offered for columns
    with pytest.raises(ValueError, match="unknown option"):
        predictive_options(dict(cov=True, bins=4))
    for bad in (None, False, 3, "all", (0.5,)):
        with pytest.raises(ValueError, match="predictive must be None, True or a dict"):
            predictive_options(bad)


def test_reference_of_a_crafted_matrix_by_hand():
    """three columns, six particles; weights 0 (twice: one dead row holds NaN), equal and unequal ones, all dyadic so that every
    product and sum below is exact and the tree's order does not matter"""
    X = np.array([[1.0, 10.0, -2.0],
                  [np.nan, np.nan, np.nan],          # dead: never read for its value
                  [2.0, 10.0, 4.0],
                  [4.0, 10.0, 0.0],
                  [100.0, -100.0, 7.0],              # dead
                  [3.0, 10.0, 2.0]])
    w = np.array([0.25, 0.0, 0.25, 0.125, 0.0, 0.375])
    r = predictive_reference(X, w, cov=True, corrected=False, wquantiles=(0.0, 0.5, 1.0), hist=dict(bins=2, range=(0.0, 4.0)))
    assert r.n_pos == 4 and r.W == 1.0 and r.Q == 0.0625 + 0.0625 + 0.015625 + 0.140625 and r.ess == 1.0 / r.Q
    mean = np.array([0.25 * 1 + 0.25 * 2 + 0.125 * 4 + 0.375 * 3, 10.0, 0.25 * -2 + 0.25 * 4 + 0.375 * 2])
    assert np.array_equal(r.mean, mean) and list(mean) == [2.375, 10.0, 1.25]
    live = w > 0
    C = X[live] - mean
    S = (w[live][:, None, None] * C[:, :, None] * C[:, None, :]).sum(0)
    assert np.array_equal(r.S, S) and np.array_equal(r.cov, S)      # corrected=False: cov = S / W, W = 1
    assert (r.S[1] == 0).all() and r.S[0, 0] == 0.984375
    assert r.quantiles.shape == (0, 3) and r.probs == () and r.wprobs == (0.0, 0.5, 1.0)
    # weighted quantiles over the integer masses m_i = w_i N 2^40: p = 0 and 1 are the smallest and largest counting value
    m = weight_fix(w, 6)
    assert m == [int(x * 6 * 2 ** 40) for x in w] and r.M == sum(m) == 6 << 40 and r.n_mass == 4
    assert list(r.wquantiles[0]) == [1.0, 10.0, -2.0] and list(r.wquantiles[2]) == [4.0, 10.0, 4.0]
    # column 0 sorted: 1 (m 1.5 u), 2 (1.5 u), 3 (2.25 u), 4 (0.75 u), u = 2^40; H = m_1 + floor(0.5 (M - m_1)) = 1.5 + 2.25 = 3.75 u
    # -> S_2 = 3 u <= H < S_3 = 5.25 u: g = 0.75 / 2.25, between 2 and 3
    assert r.wquantiles[1, 0] == 2.0 + (0.75 / 2.25) * (3.0 - 2.0) and r.wquantiles[1, 1] == 10.0
    # histograms, two bins on [0, 4]: column 0 -> bins (1 | 2, 3, 4 with the edge value 2 in the upper bin), column 1 all over,
    # column 2: -2 under, 0 in the lower bin, 2 and 4 in the upper
    h = r.hist
    u = 1 << 40
    assert h.columns == (0, 1, 2) and h.M == r.M and h.n_mass == 4
    assert h.mass1.tolist() == [[m[0], m[2] + m[3] + m[5]], [0, 0], [m[3], m[2] + m[5]]]
    assert h.under.tolist() == [0, 0, m[0]] and h.over.tolist() == [0, 6 * u, 0] and h.nan.tolist() == [0, 0, 0]
    # a vector of blobs is one column; unit weights (abcdemc) count every row, so the dead rows must then be clean
    v = predictive_reference(X[live, 0], None, wquantiles=(0.5,))
    assert v.mean.shape == (1,) and v.mean[0] == 2.5 and v.cov is None and v.S is None and v.n_pos == 4 and v.W == 4.0
    assert v.wquantiles.shape == (1, 1) and v.M == 4 << 40
    with pytest.raises(ValueError, match="needs a simulator that returns blobs"):
        predictive_reference(None, w)
    with pytest.raises(ValueError, match="no particle has a positive weight"):
        predictive_reference(X, np.zeros(6))
    same = summary_reference(X, w, cov=True, corrected=False, wquantiles=(0.0, 0.5, 1.0))
    assert np.array_equal(bits(same.mean), bits(r.mean)) and np.array_equal(bits(same.wquantiles), bits(r.wquantiles))


WIEN = tuple(math.sqrt(0.25 * t * t + 4.0 * t) for t in range(8))


def test_driver_keyword_on_the_cpu_engine(oracle):
    prior = A.Factored(A.Uniform(-2, 2), A.Uniform(0, 4))
    kw = dict(nparticles=600, verbose=False, rng=9, engine=oracle.oracle_engine)
    r = A.abcdesmc(prior, A.WienerRMS(WIEN, blobs=True), 0.3, None, predictive=dict(wquantiles=(0.1, 0.9)), **kw)
    p = r.predictive
    assert r.blobs.shape == (600, 8) and (r.Wns == 0).any()
    ref = predictive_reference(r.blobs, r.Wns, wquantiles=(0.1, 0.9))
    assert p.cov is None and p.S is None and p.hist is None and p.quantiles.shape == (0, 8) and p.wprobs == (0.1, 0.9)
    assert np.array_equal(bits(p.mean), bits(ref.mean)) and p.mean.shape == (8,)
    assert np.array_equal(bits(p.wquantiles), bits(ref.wquantiles)) and p.wquantiles.shape == (2, 8)
    assert (p.W, p.Q, p.n_pos, p.M, p.n_mass) == (ref.W, ref.Q, ref.n_pos, ref.M, ref.n_mass)
    assert (p.wquantiles[0] <= p.wquantiles[1]).all()
    # the engine call, with the other options; and the keyword goes with download=False
    q = r.engine.posterior_predictive(cov=True, corrected=False, hist=dict(bins=5, pairs=[(0, 7)], columns=(0, 3, 7)))
    ref = predictive_reference(r.blobs, r.Wns, cov=True, corrected=False, hist=dict(bins=5, pairs=[(0, 7)], columns=(0, 3, 7)))
    assert np.array_equal(bits(q.S), bits(ref.S)) and np.array_equal(bits(q.cov), bits(ref.cov))
    assert np.array_equal(q.hist.mass1, ref.hist.mass1) and np.array_equal(q.hist.mass2, ref.hist.mass2)
    assert q.hist.columns == (0, 3, 7) and np.array_equal(bits(q.hist.lo), bits(ref.hist.lo))
    bare = A.abcdesmc(prior, A.WienerRMS(WIEN, blobs=True), 0.3, None, predictive=True, download=False, **kw)
    assert bare.P is None and bare.blobs is None and np.array_equal(bits(bare.predictive.mean), bits(p.mean))
    assert bare.predictive.wquantiles.shape == (0, 8) and bare.predictive.M is None
    # default behaviour: no keyword, no field
    assert not hasattr(A.abcdesmc(prior, A.WienerRMS(WIEN, blobs=True), 0.3, None, **kw), "predictive")
    # abcdemc: unit weights
    m = A.abcdemc(prior, A.WienerRMS(WIEN, blobs=True), 0.5, None, nparticles=200, generations=8, verbose=False, rng=9,
                  engine=oracle.oracle_engine, predictive=dict(cov=True, wquantiles=(0.5,)))
    ref = predictive_reference(m.blobs, None, cov=True, wquantiles=(0.5,))
    assert m.predictive.n_pos == 200 and m.predictive.W == 200.0
    assert np.array_equal(bits(m.predictive.mean), bits(ref.mean)) and np.array_equal(bits(m.predictive.S), bits(ref.S))
    assert np.array_equal(bits(m.predictive.wquantiles), bits(ref.wquantiles))


def test_all_four_keywords_in_one_call_on_the_cpu_engine(oracle):
    """the download with ``summary``, ``sample``, ``predictive`` and ``adjust`` in one driver call: on the CPU test engine every
    one of the four engine methods takes its fallback, the restatement of ``result()``"""
    from test_gpu_posterior_predictive import all_keywords_run

    r = all_keywords_run(A.abcdesmc, 600, engine=oracle.oracle_engine, target=0.0, ABCk=A.Epa0toeps, max_iters=3)
    assert r.iters == 3 and (r.Wns == 0).any() and np.unique(r.Wns[r.Wns > 0]).size > 1
    m = all_keywords_run(A.abcdemc, 600, engine=oracle.oracle_engine, target=0.5, generations=6)
    assert m.summary.n_pos == 600 and m.adjusted.W == 600.0


def test_refused_without_blobs(oracle):
    prior = A.Factored(A.Uniform(-2, 2), A.Uniform(0, 4))
    kw = dict(nparticles=200, verbose=False, rng=9, engine=oracle.oracle_engine, max_iters=2)
    with pytest.raises(ValueError, match=r"predictive: needs a simulator that returns blobs \(blobs=True\)"):
        A.abcdesmc(prior, A.WienerRMS(WIEN), 0.3, None, predictive=True, **kw)
    r = A.abcdesmc(prior, A.WienerRMS(WIEN), 0.3, None, **kw)
    with pytest.raises(ValueError, match=r"predictive: needs a simulator that returns blobs \(blobs=True\)"):
        r.engine.posterior_predictive()
    with pytest.raises(ValueError, match="unknown option"):          # refused before anything runs
        A.abcdesmc(prior, A.WienerRMS(WIEN, blobs=True), 0.3, None, predictive=dict(quantiles=(0.5,)), **kw)
    with pytest.raises(ValueError, match="p must be in"):
        A.abcdesmc(prior, A.WienerRMS(WIEN, blobs=True), 0.3, None, predictive=dict(wquantiles=(1.5,)), **kw)
