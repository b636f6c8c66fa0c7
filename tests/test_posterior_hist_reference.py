"""The marginal and pairwise histograms of include/abcdez_spec.h ("posterior summaries", histograms) as
abcdez_amd.summary.hist_reference restates them: integer masses, abz_hist_bin, integer sums.  No GPU: this file pins the DEFINITION
(a plain Python loop, np.histogram on dyadic data, the conservation identities, the edge cases, the refusals);
tests/test_gpu_posterior_hist.py then holds the device to this reference exactly."""
import math
import time

import numpy as np
import pytest

from abcdez_amd.summary import hist_reference, stratum_bits, summary_options, summary_reference, weight_fix


def loop_restatement(X, w, cols, bins, ranges, pairs, bins2):
    """every rule of the spec paragraph with Python floats and integers, one position at a time; ranges: {column: (lo, hi)}"""
    N = X.shape[0]
    masses = [1 << stratum_bits(N)] * N if w is None else weight_fix(w, N)

    def bin_of(x, lo, hi, nb):
        if x != x:
            return "nan"
        if x < lo:
            return "under"
        if x > hi:
            return "over"
        return min(int(math.floor((x - lo) * (float(nb) / (hi - lo)))), nb - 1)

    mass1 = {k: [0] * bins for k in cols}
    tally = {k: dict(under=0, over=0, nan=0) for k in cols}
    mass2 = {p: [[0] * bins2 for _ in range(bins2)] for p in pairs}
    outside2 = {p: 0 for p in pairs}
    for i in range(N):
        m = masses[i]
        if m < 1:
            continue
        for k in cols:
            b = bin_of(float(X[i, k]), *ranges[k], bins)
            if isinstance(b, str):
                tally[k][b] += m
            else:
                mass1[k][b] += m
        for (j, k) in pairs:
            bj, bk = bin_of(float(X[i, j]), *ranges[j], bins2), bin_of(float(X[i, k]), *ranges[k], bins2)
            if isinstance(bj, str) or isinstance(bk, str):
                outside2[(j, k)] += m
            else:
                mass2[(j, k)][bj][bk] += m
    return mass1, tally, mass2, outside2, sum(masses), sum(1 for m in masses if m >= 1)


def auto_ranges(X, w, cols):
    N = X.shape[0]
    masses = [1 << stratum_bits(N)] * N if w is None else weight_fix(w, N)
    live = np.array([m >= 1 for m in masses])
    out = {}
    for k in cols:
        v = sorted(X[live, k].tolist(), key=lambda x: (x, not math.copysign(1.0, x) < 0))    # -0.0 below +0.0
        lo, hi = v[0], v[-1]
        out[k] = (lo - 0.5, hi + 0.5) if lo == hi else (lo, hi)
    return out


def assert_is_the_loop(h, X, w, ranges):
    mass1, tally, mass2, outside2, M, n_mass = loop_restatement(X, w, h.columns, h.bins, ranges, h.pairs, h.bins2 or 1)
    assert (h.M, h.n_mass) == (M, n_mass)
    for c, k in enumerate(h.columns):
        assert (float(h.lo[c]), float(h.hi[c])) == ranges[k]
        assert h.mass1[c].tolist() == mass1[k], k
        assert (int(h.under[c]), int(h.over[c]), int(h.nan[c])) == (tally[k]["under"], tally[k]["over"], tally[k]["nan"]), k
    for q, p in enumerate(h.pairs):
        assert h.mass2[q].tolist() == mass2[p], p
        assert int(h.outside2[q]) == outside2[p], p


@pytest.mark.parametrize("N,d", [(7, 1), (60, 3), (301, 4)])
def test_against_a_plain_python_loop(N, d):
    rng = np.random.default_rng(N)
    X = rng.standard_normal((N, d))
    X[rng.integers(0, N, 5), 0] = 0.25
    w = rng.random(N) * (rng.random(N) < 0.7)
    w[0] = max(w[0], 0.1)
    w /= w.sum()
    pairs = "all" if d > 1 else None
    cols = list(range(d))
    h = hist_reference(X, w, bins=11, pairs=pairs, bins2=5)
    assert_is_the_loop(h, X, w, auto_ranges(X, w, cols))
    # an explicit range that cuts both tails, no weight array
    h = hist_reference(X, None, bins=6, range=(-0.75, 0.5), pairs=pairs, bins2=3)
    assert_is_the_loop(h, X, None, {k: (-0.75, 0.5) for k in cols})
    assert N < 60 or (h.under.min() > 0 and h.over.min() > 0 and h.outside2.min() > 0)      # seven values need not reach a tail
    assert h.M == N << 40 and h.n_mass == N and (h.mass1 % np.uint64(1 << 40) == 0).all()


def test_against_np_histogram_on_dyadic_data():
    """lo = 0, hi = 8, 8 bins: scale = 1, the edges 0 .. 8 are exact and np.histogram's own rule (last bin closed) is this one;
    values are multiples of 1/4, unit weights (no weight array): counts = mass >> b"""
    rng = np.random.default_rng(8)
    N = 4000
    X = rng.integers(-4, 40, (N, 2)) / 4.0                       # -1 .. 9.75: some under, some over, some exactly 8
    assert (X == 8.0).any() and (X < 0).any() and (X > 8).any()
    h = hist_reference(X, None, bins=8, range=(0.0, 8.0), pairs=[(0, 1)], bins2=8)
    b = stratum_bits(N)
    for k in range(2):
        counts, edges = np.histogram(X[:, k], bins=8, range=(0.0, 8.0), weights=np.ones(N))
        assert np.array_equal(edges, h.edges[k]) and np.array_equal(h.mass1[k] >> np.uint64(b), counts.astype(np.uint64))
        assert int(h.under[k]) >> b == (X[:, k] < 0).sum() and int(h.over[k]) >> b == (X[:, k] > 8).sum() and h.nan[k] == 0
    c2, _, _ = np.histogram2d(X[:, 0], X[:, 1], bins=8, range=((0.0, 8.0), (0.0, 8.0)))
    assert np.array_equal(h.mass2[0] >> np.uint64(b), c2.astype(np.uint64))
    assert np.allclose(h.density().sum(axis=1) * 1.0, (h.mass1.sum(axis=1) / h.M))


@pytest.mark.parametrize("N", [300, 2048, 5001])
def test_conservation_and_marginal_consistency(N):
    rng = np.random.default_rng(N)
    X = rng.standard_normal((N, 5))
    w = rng.random(N) * (rng.random(N) < 0.6)
    w /= w.sum()
    h = hist_reference(X, w, bins=16, pairs="all", bins2=16)
    assert ((h.mass1.sum(axis=1) + h.under + h.over + h.nan) == np.uint64(h.M)).all()
    assert (h.under == 0).all() and (h.over == 0).all() and (h.nan == 0).all() and (h.outside2 == 0).all()
    assert len(h.pairs) == 10 and h.mass2.shape == (10, 16, 16)
    for q, (j, k) in enumerate(h.pairs):
        assert np.array_equal(h.mass2[q].sum(axis=1), h.mass1[j]) and np.array_equal(h.mass2[q].sum(axis=0), h.mass1[k])
    # with an explicit range the identity holds with the tallies
    h = hist_reference(X, w, bins=9, range=(-1.0, 0.5), pairs="all", bins2=4)
    assert ((h.mass1.sum(axis=1) + h.under + h.over + h.nan) == np.uint64(h.M)).all() and h.under.min() > 0 and h.over.min() > 0
    assert ((h.mass2.sum(axis=(1, 2)) + h.outside2) == np.uint64(h.M)).all() and h.outside2.min() > 0


def test_edge_membership():
    w = None
    # x == hi lands in the last bin, x == lo in the first; values on inner edges go up
    h = hist_reference(np.array([0.0, 1.0, 2.0, 3.0, 4.0, 4.0]), w, bins=4, range=(0.0, 4.0))
    assert (h.mass1[0] >> np.uint64(40)).tolist() == [1, 1, 1, 3] and h.over[0] == 0
    h = hist_reference(np.array([1.0, 3.0, 7.0]), w, bins=3)                      # automatic: lo = 1, hi = 7
    assert (h.lo[0], h.hi[0]) == (1.0, 7.0) and (h.mass1[0] >> np.uint64(40)).tolist() == [1, 1, 1]
    # -0.0 with lo = +0.0 is in bin 0, not under
    h = hist_reference(np.array([-0.0, 0.5, 1.0]), w, bins=2, range=(0.0, 1.0))
    assert (h.mass1[0] >> np.uint64(40)).tolist() == [1, 2] and h.under[0] == 0
    # automatic range over signed zeros only: lo = -0.0, hi = +0.0 are equal as doubles -> +- 0.5
    h = hist_reference(np.array([0.0, -0.0, 0.0]), w, bins=4)
    assert (h.lo[0], h.hi[0]) == (-0.5, 0.5) and (h.mass1[0] >> np.uint64(40)).tolist() == [0, 0, 3, 0]
    # a constant column gets the +- 0.5 range
    h = hist_reference(np.full((9, 2), -1.75), w, bins=5, pairs="all", bins2=2)
    assert h.lo.tolist() == [-2.25, -2.25] and h.hi.tolist() == [-1.25, -1.25]
    assert (h.mass1 >> np.uint64(40)).tolist() == [[0, 0, 9, 0, 0]] * 2 and (h.mass2[0] >> np.uint64(40)).tolist() == [[0, 0], [0, 9]]
    assert h.edges.shape == (2, 6) and h.edges[0][0] == -2.25 and h.edges[0][-1] == -1.25 and (np.diff(h.edges[0]) > 0).all()
    # NaN under an explicit range is tallied, +-1e150 fall outside, denormals are in range
    h = hist_reference(np.array([np.nan, 1e150, -1e150, 5e-324, -5e-324, 0.0]), w, bins=2, range=(-1.0, 1.0))
    assert (int(h.nan[0]) >> 40, int(h.over[0]) >> 40, int(h.under[0]) >> 40) == (1, 1, 1)
    assert (h.mass1[0] >> np.uint64(40)).tolist() == [0, 3]      # -5e-324 - -1.0 rounds to 1.0: bin 1, membership is the rule's


def test_a_per_column_range_follows_columns_given_in_any_order():
    """columns come back sorted; row i of a per-column range belongs to columns[i] AS GIVEN and is sorted along with it"""
    X = np.empty((40, 3))
    X[:, 0], X[:, 1], X[:, 2] = 0.5, -3.0, 10.5
    h = hist_reference(X, None, bins=2, columns=[2, 0], range=[(10, 11), (0, 1)], pairs=[(0, 2)], bins2=2)
    assert h.columns == (0, 2) and h.lo.tolist() == [0.0, 10.0] and h.hi.tolist() == [1.0, 11.0]
    assert (h.under == 0).all() and (h.over == 0).all() and (h.mass1 >> np.uint64(40)).tolist() == [[0, 40], [0, 40]]
    assert (h.mass2[0] >> np.uint64(40)).tolist() == [[0, 0], [0, 40]] and h.outside2[0] == 0
    same = hist_reference(X, None, bins=2, columns=[0, 2], range=[(0, 1), (10, 11)], pairs=[(0, 2)], bins2=2)
    assert np.array_equal(h.mass1, same.mass1) and np.array_equal(h.lo, same.lo) and np.array_equal(h.mass2, same.mass2)
    rng = np.random.default_rng(4)
    Y = rng.standard_normal((301, 4)) + np.array([0.0, 5.0, -5.0, 20.0])
    ranges = {0: (-1.0, 1.5), 1: (4.0, 7.0), 2: (-6.0, -5.5), 3: (18.0, 23.0)}
    order = [3, 0, 2]
    h = hist_reference(Y, None, bins=7, columns=order, range=[ranges[k] for k in order], pairs="all", bins2=3)
    assert h.columns == (0, 2, 3) and h.pairs == ((0, 2), (0, 3), (2, 3))
    assert_is_the_loop(h, Y, None, ranges)
    s = summary_reference(Y, None, cov=False, hist=dict(bins=7, columns=order, range=[ranges[k] for k in order], pairs="all", bins2=3))
    assert np.array_equal(s.hist.mass1, h.mass1) and np.array_equal(s.hist.lo, h.lo) and np.array_equal(s.hist.mass2, h.mass2)
    h1 = hist_reference(Y, None, bins=7, columns=order, range=(-1.0, 1.5))              # one range for all: nothing to sort
    assert h1.lo.tolist() == [-1.0] * 3


def test_a_positive_weight_without_mass_does_not_count_and_is_never_read():
    wts = np.array([0.5, 2.0 ** -70, 0.25, 0.0, 0.25])
    X = np.array([3.0, np.nan, 1.0, 1e300, 2.0])
    h = hist_reference(X, wts, bins=2)
    assert h.n_mass == 3 and (h.lo[0], h.hi[0]) == (1.0, 3.0) and h.nan[0] == 0
    assert h.M == sum(weight_fix(wts, 5)) and h.mass1[0].tolist() == [weight_fix([0.25], 5)[0], weight_fix([0.75], 5)[0]]


def test_refusals():
    X = np.arange(12.0).reshape(6, 2)
    for bad in (dict(bins=0), dict(bins=4097), dict(pairs="all", bins2=0), dict(pairs="all", bins2=129), dict(pairs=[(1, 0)]),
                dict(pairs=[(0, 0)]), dict(pairs=[(0, 2)]), dict(pairs=[(0, 1), (0, 1)]), dict(columns=[0], pairs=[(0, 1)]), dict(columns=[2]), dict(columns=[]),
                dict(range=(1.0, 1.0)), dict(range=(2.0, 1.0)), dict(range=(0.0, np.inf)), dict(range=(-1e308, 1e308)),
                dict(range=(np.nan, 1.0)), dict(pairs="some"), dict(range=[(0, 1), (0, 1), (0, 1)])):
        with pytest.raises(ValueError, match="summary: "):
            hist_reference(X, None, **bad)
    with pytest.raises(ValueError, match="at least two parameters"):
        hist_reference(X[:, 0], None, pairs="all")
    with pytest.raises(ValueError, match="at least two parameters"):
        hist_reference(X[:, :1], None, pairs=[(0, 1)])
    for poison in (np.nan, np.inf, -np.inf):
        Y = X.copy()
        Y[3, 1] = poison
        with pytest.raises(ValueError, match="automatic range of column 1 .*pass a range"):
            hist_reference(Y, None)
        assert hist_reference(Y, None, range=(0.0, 12.0)).M == 6 << 40            # an explicit range takes it
        assert hist_reference(Y, np.array([.2, .2, .2, 0, .2, .2])).n_mass == 5     # and a dead row is never read
    Y = X.copy()
    Y[0, 0], Y[1, 0] = -1e308, 1e308
    with pytest.raises(ValueError, match="automatic range of column 0"):
        hist_reference(Y, None)
    with pytest.raises(ValueError, match="not normalised"):
        hist_reference(X, np.full(6, 1e6))
    with pytest.raises(ValueError, match="no particle has a positive weight"):
        hist_reference(X, np.full(6, 2.0 ** -70))
    with pytest.raises(ValueError, match="no particle has a positive weight"):
        hist_reference(X, np.zeros(6))
    with pytest.raises(ValueError, match="unknown hist option"):
        summary_reference(X, None, hist=dict(bin=3))


def test_summary_options_and_the_record():
    assert summary_options(dict(hist=dict(bins=8), cov=False)) == dict(hist=dict(bins=8), cov=False)
    with pytest.raises(ValueError, match="unknown option.*hist"):
        summary_options(dict(histogram=True))
    with pytest.raises(ValueError, match="wquantiles, hist"):
        summary_options(3)
    X = np.random.default_rng(0).standard_normal((50, 3))
    r = summary_reference(X, None)
    assert r.hist is None and r.M is None
    r = summary_reference(X, None, cov=False, hist=True)
    assert r.hist.bins == 64 and r.hist.columns == (0, 1, 2) and r.hist.pairs == () and r.hist.bins2 is None and r.hist.edges2 is None
    assert r.hist.mass2.shape == (0, 0, 0) and r.M == r.hist.M == 50 << 40 and r.n_mass == 50
    r = summary_reference(X, None, cov=False, wquantiles=(0.5,), hist=dict(bins=300, columns=(2, 0), pairs="all"))
    assert r.hist.columns == (0, 2) and r.hist.pairs == ((0, 2),) and r.hist.bins2 == 128 and r.hist.edges2.shape == (2, 129)
    assert r.hist.edges.shape == (2, 301) and (r.hist.edges[:, 0] == r.hist.lo).all() and (r.hist.edges[:, -1] == r.hist.hi).all()
    assert np.array_equal(r.hist.lo, X[:, [0, 2]].min(axis=0)) and r.wquantiles.shape == (1, 3)
    dens = r.hist.density()
    assert dens.dtype == np.float64 and np.allclose((dens * (r.hist.hi - r.hist.lo)[:, None] / 300).sum(axis=1), 1.0)


def test_the_restatement_is_quick_enough_for_the_gpu_tests():
    rng = np.random.default_rng(1)
    X = rng.standard_normal((5001, 32))
    w = rng.random(5001)
    w /= w.sum()
    t = time.perf_counter()
    h = hist_reference(X, w, bins=37, pairs="all", bins2=16)
    took = time.perf_counter() - t
    print("N = 5001, d = 32, 496 pairs:", took, "s")
    assert len(h.pairs) == 496 and took < 1.0


def test_driver_keyword_reaches_the_reference_engine(oracle):
    import abcdez_amd as A

    opts = dict(bins=12, range=(-2.0, 8.0))
    r = A.abcdesmc(A.Normal(0, math.sqrt(10)), A.Normal1D(3.0), 0.5, None, nparticles=300, verbose=False, rng=3, ABCk=A.Epa0toϵ,
                   engine=oracle.oracle_engine, summary=dict(cov=False, hist=opts))
    ref = hist_reference(r.P, r.Wns, **opts)
    h = r.summary.hist
    assert np.array_equal(h.mass1, ref.mass1) and h.M == ref.M == r.summary.M and h.n_mass == ref.n_mass
    assert np.unique(r.Wns[r.Wns > 0]).size > 1 and h.mass1.sum() + h.under[0] + h.over[0] == h.M
