"""Weighted marginal quantiles (csrc/abz_wquantile.hip) and marginal / pairwise histograms (csrc/abz_hist.hip) where
test_gpu_posterior_wquantiles.py and test_gpu_posterior_hist.py do not reach:

  1. discrete prior components away from index 0, so that every `M->prior[...]` index of the two files is observable;
  2. rows wider than 32 doubles (3 .. 16 chunks of 16 quantile columns, up to 32 640 pairs), a correlated prior, classic storage,
     N = 1, 2 and the N just past a tile, tiles without mass;
  3. the second trip of every grid-stride loop;
  4. the three entry points interleaved on one context's growing workspace.

Every comparison with abcdez_amd.summary (summary_reference, hist_reference, wquantiles_reference) is EXACT: masses, tallies, M and
n_mass as integers; lo, hi, edges and quantiles bit for bit.  There is no tolerance in this file.  The synthetic populations are
those of test_gpu_posterior_summary_edges.py (`synthetic`: both row slots in use, NaN / +-inf behind everything that must not be
read) with the unequal dyadic weights of the two suites above, whose zeros are the dead positions; the contexts are built with an
Epanechnikov kernel, as in test_gpu_posterior_wquantiles.py."""
import numpy as np
import pytest

import abcdez_amd as A
from abcdez_amd.engine import HipOps
from abcdez_amd.summary import hist_reference, make_summary, summary_reference, wquantiles_reference
from test_gpu_posterior_hist import assert_identities, assert_same_hist, crafted, device_hist, dyadic_weights, unequal_positive
from test_gpu_posterior_summary import assert_same
from test_gpu_posterior_summary_edges import POISON, TILE, spec_of, synthetic
from test_gpu_posterior_wquantiles import PROBS, PROBS37, assert_same_wq, bits, model, run3

pytestmark = pytest.mark.gpu

TIE_PROBS = (0.3, 0.31, 0.5, 0.52)          # inside tie groups of a column with a handful of distinct values

# launch bounds of the two files, each with the #define it mirrors: section 3 asserts its arithmetic from these
ABZ_BLOCK = 256               # abz_device.h   #define ABZ_BLOCK 256
WQ_CB = 16                    # abz_wquantile  #define WQ_CB 16
WQ_ITEMS = 8                  # abz_wquantile  #define WQ_ITEMS 8
WQ_TILE = ABZ_BLOCK * WQ_ITEMS  # abz_wquantile  #define WQ_TILE (ABZ_BLOCK * WQ_ITEMS)
WQ_MAX_BLOCKS = 2048          # abz_wquantile  #define WQ_MAX_BLOCKS 2048
WQ_PASS_BLOCKS = 128          # abz_wquantile  #define WQ_PASS_BLOCKS 128
HB_K = 16                     # abz_hist       #define HB_K 16
H1_CELLS = 5120               # abz_hist       #define H1_CELLS 5120
H2_CELLS = 8192               # abz_hist       #define H2_CELLS 8192
H_VEC = 4                     # abz_hist       #define H_VEC 4
H_TILE = ABZ_BLOCK * H_VEC    # abz_hist       #define H_TILE (ABZ_BLOCK * H_VEC)
H_PAD = 16                    # abz_hist       #define H_PAD 16
H_RANGE_BLOCKS = 1024         # abz_hist       #define H_RANGE_BLOCKS 1024
H_BIN_BLOCKS = 4096           # abz_hist       #define H_BIN_BLOCKS 4096
H_PASS_BLOCKS = 128           # abz_hist       #define H_PASS_BLOCKS 128
H_PASS_WORKGROUPS = 2048      # abz_hist       #define H_PASS_WORKGROUPS 2048


def ceil_div(a, b):
    return -(-a // b)


def epa(spec):
    """the model of ``spec`` under an Epanechnikov kernel"""
    return A.ModelSpec(spec.prior, spec.sim, A.Epa0toϵ, seed=1)


@pytest.fixture(scope="module")
def ops_of():
    """one Epanechnikov context per row width for the synthetic cases (a context is independent of N)"""
    made = {}

    def get(d):
        if d not in made:
            spec = epa(spec_of(d))
            made[d] = (spec, HipOps(spec))
        return made[d]
    yield get
    for _, ops in made.values():
        ops.close()


def weighted(spec, ops, N, rng, values=None, mask=None, dead=0.3):
    """`synthetic` with dyadic_weights: unequal positive weights, the zeros (a share ``dead``, and everything outside ``mask``)
    are the dead positions"""
    w = dyadic_weights(rng, N, dead=dead)
    if mask is not None:
        w = np.where(mask, w, 0.0)
    assert N < 3 or unequal_positive(w)
    return synthetic(spec, N, rng, w > 0.0, values=values, weights=w, ops=ops)


def device_wq(pop, probs, k0=0, nk=None):
    return pop.ops.posterior_wquantiles(pop.bits, pop.slot0, pop.slot1, pop.wns, pop.N, probs, k0=k0, nk=nk)


def assert_wq(got, ref, what, cols=slice(None)):
    """got: (q[nk, n_probs], M, n_mass) of the device; ref: (wquantiles[n_probs, d], M, n_mass) of wquantiles_reference"""
    q, M, n_mass = got
    want = ref[0][:, cols]
    assert (M, n_mass) == (ref[1], ref[2]), (what, M, ref[1], n_mass, ref[2])
    assert q.T.shape == want.shape, (what, q.shape, want.shape)
    same = bits(q.T) == bits(want)
    assert same.all(), (what, np.argwhere(~same)[:5], q.T[~same][:5], want[~same][:5])


def check_wq(pop, probs=PROBS, what=""):
    ref = wquantiles_reference(pop.P, pop.Wns, probs)
    assert_wq(device_wq(pop, probs), ref, what)
    return ref


def check_hist(pop, opts, what=""):
    dev = device_hist(pop.ops, (pop.bits, pop.slot0, pop.slot1, pop.wns), pop.N, pop.d, opts)
    ref = hist_reference(pop.P, pop.Wns, **opts)
    assert_same_hist(dev, ref, (what, opts))
    assert_identities(dev)
    return dev


# ------------------------------------------------------------------------------------------ 1. prior indices

HALF = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 0.49999999999999994, 0.2, -0.2, 3.7])
DISCRETE = (1, 17, 32)        # column 17 is in the second chunk of 16 quantile columns, column 32 alone in the third
CONTINUOUS = (0, 16, 5)       # the same values in continuous columns stay as they are


class Discrete33:
    """d = 33, DiscreteUniform(1, 10) at the columns 1 and 17, Poisson(2.0) at 32, Normal(0, 1) elsewhere; the half-way set in
    the discrete columns and in three continuous ones; N = TILE + 300, about 30 % dead and poisoned.  ``ref`` / ``raw``: the
    weighted quantiles of all columns of P (push_p applied) and of the rows as stored (unrounded), per set of probabilities."""
    d = 33
    N = TILE + 300

    def __init__(self):
        d, N = self.d, self.N
        comps = [A.Normal(0.0, 1.0) for _ in range(d)]
        comps[1], comps[17], comps[32] = A.DiscreteUniform(1, 10), A.DiscreteUniform(1, 10), A.Poisson(2.0)
        self.spec = A.ModelSpec(A.Factored(*comps), A.MVNormal(tuple([0.25] * d)), A.Epa0toϵ, seed=1)
        assert self.spec.discrete == tuple(k in DISCRETE for k in range(d))
        rng = np.random.default_rng(331)
        values = rng.standard_normal((N, d))
        for k in DISCRETE + CONTINUOUS:
            values[:, k] = rng.choice(HALF, N)
        self.ops = HipOps(self.spec)
        self.pop = pop = weighted(self.spec, self.ops, N, rng, values=values)
        live = pop.Wns > 0.0
        assert 0.6 * N < live.sum() < 0.8 * N and np.array_equal(bits(pop.rows[~live]), bits(np.resize(POISON, (N, d))[~live]))
        P = pop.P[live]
        for k in DISCRETE:
            zeros = P[P[:, k] == 0, k]
            assert np.array_equal(P[:, k], np.rint(P[:, k])) and set(P[:, k]) == {-2.0, 0.0, 2.0, 4.0}
            assert np.signbit(zeros).any() and not np.signbit(zeros).all()          # -0.0 and +0.0: their order keys differ
        for k in CONTINUOUS:
            assert np.array_equal(bits(P[:, k]), bits(values[live, k])) and not np.array_equal(P[:, k], np.rint(P[:, k]))
        self.ref = {probs: wquantiles_reference(pop.P, pop.Wns, probs) for probs in (PROBS, TIE_PROBS)}
        self.raw = {probs: wquantiles_reference(pop.rows, pop.Wns, probs) for probs in (PROBS, TIE_PROBS)}


@pytest.fixture(scope="module")
def discrete33():
    pop = Discrete33()
    yield pop
    pop.ops.close()


@pytest.mark.parametrize("k0,nk", [(0, 33), (1, 1), (17, 1), (16, 2), (17, 16), (32, 1), (5, 28)])
def test_wquantiles_push_the_discrete_columns_of_any_sub_range(discrete33, k0, nk):
    """`M->prior[k_first + c]` of wq_gather_kernel: in these sub-ranges k_first + c, the position c in the call and the
    chunk-local index all differ.  (A column's quantiles do not depend on the other columns of the call: the reference of a
    sub-range is that slice of the reference of all columns, computed once.)"""
    t = discrete33
    cols = slice(k0, k0 + nk)
    for probs in (PROBS, TIE_PROBS):
        assert_wq(device_wq(t.pop, probs, k0=k0, nk=nk), t.ref[probs], (k0, nk, probs), cols)
        # the test observes push_p: unrounded values would give other quantiles in every discrete column, and only there
        for k in range(k0, k0 + nk):
            same = np.array_equal(bits(t.ref[probs][0][:, k]), bits(t.raw[probs][0][:, k]))
            assert same == (k not in DISCRETE), (k, probs)
    assert any(k0 <= k < k0 + nk for k in DISCRETE)


def assert_hist_observes_push_p(t, opts, ref):
    """the reference of the rows as stored (unrounded) differs from ``ref`` in every discrete column, and in no other"""
    raw = hist_reference(t.pop.rows, t.pop.Wns, **opts)
    assert raw.columns == ref.columns
    for c, k in enumerate(ref.columns):
        same = all(np.array_equal(getattr(raw, f)[c], getattr(ref, f)[c]) for f in ("mass1", "under", "over", "lo", "hi"))
        assert same == (k not in DISCRETE), (opts, k)
    for q, (j, k) in enumerate(ref.pairs):
        assert not np.array_equal(raw.mass2[q], ref.mass2[q]) or (j not in DISCRETE and k not in DISCRETE), (opts, j, k)


HIST_DISCRETE = {
    "all columns, automatic": dict(bins=37, pairs=[(1, 17), (17, 32), (0, 17), (16, 32)], bins2=9),
    # list position != column index for every entry; the rounded 2.0 and 4.0 sit exactly on an edge of column 32 and 17
    "32, 17, 0 with ranges": dict(bins=8, columns=[32, 17, 0], range=[(0.0, 4.0), (-2.0, 2.0), (-1.0, 3.0)],
                                  pairs=[(0, 17), (17, 32)], bins2=4),
    "32, 17, 0 automatic": dict(bins=8, columns=[32, 17, 0], pairs=[(0, 17), (17, 32)], bins2=4),
    "17 alone with a range": dict(bins=8, columns=[17], range=(0.0, 4.0)),
    "17 alone automatic": dict(bins=8, columns=[17]),
}


@pytest.mark.parametrize("case", list(HIST_DISCRETE))
def test_histograms_push_the_discrete_columns_of_any_column_list(discrete33, case):
    """`M->prior[h.col]` of hist_range_kernel (automatic range) and hist_bin_kernel: the parameter index, not the position in the
    requested-column list (and not the index within the range kernel's launch of 8 columns)"""
    t, opts = discrete33, HIST_DISCRETE[case]
    dev = check_hist(t.pop, opts, case)
    assert_hist_observes_push_p(t, opts, dev)
    if "range" in opts and case.startswith("32"):
        assert dev.columns == (0, 17, 32) and [(a, b) for a, b in zip(dev.lo, dev.hi)] == [(-1.0, 3.0), (-2.0, 2.0), (0.0, 4.0)]
        c = dev.columns.index(32)                    # -2 under; -0.0 and +0.0 in bin 0; 2.0 on the edge of bin 4; 4.0 = hi in bin 7
        assert dev.under[c] > 0 and dev.over[c] == 0 and (dev.mass1[c][[0, 4, 7]] > 0).all() and dev.mass1[c].sum() + dev.under[c] == dev.M


# ------------------------------------------------------------------------------------------ 2. wide rows, bit for bit

def wide_hist(d):
    return dict(bins=37, pairs="all", bins2=16) if d <= 65 else dict(bins=37, pairs="all", bins2=4)


def assert_real_run(s, ref, d, opts):
    assert_same_wq(s, ref, d)
    assert_same_hist(s.hist, ref.hist, d)
    assert_identities(s.hist)
    assert (s.M, s.n_mass) == (ref.M, ref.n_mass) and np.array_equal(bits(s.mean), bits(ref.mean))
    n_pairs = len(opts["pairs"]) if isinstance(opts["pairs"], list) else d * (d - 1) // 2
    assert s.wquantiles.shape == (len(PROBS), d) and s.hist.mass1.shape == (d, opts["bins"])
    assert s.hist.mass2.shape == (n_pairs, opts["bins2"], opts["bins2"]) and len(s.hist.pairs) == n_pairs


@pytest.mark.parametrize("d", [33, 64, 65, 100, 129, 200, 255, 256])
def test_wide_rows_of_a_real_run(d):
    """ld = 64, 128, 256: 3 .. 16 chunks of WQ_CB quantile columns reusing the states, histograms and partials, the last chunk
    of d = 33, 65, 129 one column wide; 5 .. 32 launches of the range kernel; d = 256: 32 640 pairs (4 MB of cells at
    bins2 = 4), 16 columns k per batch with ragged last batches.  N = 2049, one position past a tile; the driver refuses
    nparticles < 3 d / min(α, δess) = 2319, 2328 at d = 255, 256, which run one position past two tiles."""
    N = 2049 if d <= 200 else 2 * TILE + 1
    assert N >= 3 * d / 0.33
    r = run3(*model(d), N, abck=A.Epa0toϵ, δess=0.33)
    assert unequal_positive(r.Wns) and r.engine.ops.layout()[0] == r.engine.spec.ld >= d > 2 * WQ_CB
    opts = wide_hist(d)
    s = r.engine.posterior_summary(cov=False, wquantiles=PROBS, hist=opts)
    assert_real_run(s, summary_reference(r.P, r.Wns, cov=False, wquantiles=PROBS, hist=opts), d, opts)


def test_wide_rows_with_a_correlated_prior():
    """the MvNormal prior of test_gpu_posterior_summary_edges.py::test_wide_rows_with_a_correlated_prior, d = 128"""
    d = 128
    rng = np.random.default_rng(5)
    Lm = np.tril(rng.normal(0, 0.05, (d, d)), -1) + np.diag(rng.uniform(0.8, 1.2, d))
    prior = A.MvNormal(rng.normal(0, 0.2, d), Lm @ Lm.T)
    r = run3(prior, A.MVNormal(tuple(1.0 for _ in range(d))), 2049, abck=A.Epa0toϵ, δess=0.33)
    assert unequal_positive(r.Wns)
    opts = dict(bins=37, pairs=[(0, 127), (63, 64)], bins2=16)
    s = r.engine.posterior_summary(cov=False, wquantiles=PROBS, hist=opts)
    assert_real_run(s, summary_reference(r.P, r.Wns, cov=False, wquantiles=PROBS, hist=opts), d, opts)


def test_wide_rows_in_classic_storage():
    d, N = 64, 2049
    opts = dict(bins=37, pairs="all", bins2=4)
    m = A.abcdemc(*model(d), 0.5, None, nparticles=N, generations=6, verbose=False, rng=5,
                  summary=dict(wquantiles=PROBS, hist=opts))
    ref = summary_reference(m.P, None, wquantiles=PROBS, hist=opts)
    assert_real_run(m.summary, ref, d, opts)
    assert m.summary.M == N << 40 and m.summary.n_mass == N and m.summary.hist.M == N << 40


def middle(bins):
    """the bin or bins around the centre of a range"""
    return list(range((bins - 1) // 2, bins // 2 + 1))


@pytest.mark.parametrize("N", [1, 2, 300, 2048, 2049, 3 * 2048 + 1])
@pytest.mark.parametrize("d", [5, 33, 255, 256])
def test_wide_synthetic_rows(ops_of, d, N):
    """the ragged chunks, launches and batches at every width with both slots in use, independent of what a sampler leaves;
    d = 256 with bins = 4096: G = 1, one workgroup group per column.  N = 1: M - m_(1) = 0 and every probability takes the `top`
    branch, Nld rounds 1 up to 16, the automatic range is the widened constant column.  N = 1, 2: no dead position."""
    spec, ops = ops_of(d)
    rng = np.random.default_rng(1000 * d + N)
    pop = weighted(spec, ops, N, rng, dead=0.3 if N > 2 else 0.0)
    bins = 4096 if d == 256 else 37
    assert bins != 4096 or min(H1_CELLS // (bins + 3), d) == 1
    ref = check_wq(pop, what=(d, N))
    hists = [check_hist(pop, dict(bins=bins, pairs="all", bins2=b2), (d, N)) for b2 in ((4, 91) if d == 5 else (4,))]
    assert ref[2] == (pop.Wns > 0).sum() == hists[0].n_mass and ref[1] == hists[0].M
    if N == 1:
        row = pop.P[0]
        assert all(np.array_equal(q, row) for q in ref[0])
        for h in hists:
            assert np.array_equal(h.lo, row - 0.5) and np.array_equal(h.hi, row + 0.5)
            assert (h.mass1[:, middle(bins)].sum(axis=1) == h.M).all()
            m2 = middle(h.bins2)
            assert (h.mass2[:, m2][:, :, m2].sum(axis=(1, 2)) == h.M).all() and (h.outside2 == 0).all()
    if N == 2:
        assert ref[2] == 2
        assert np.array_equal(ref[0][0], pop.P.min(axis=0)) and np.array_equal(ref[0][-1], pop.P.max(axis=0))
        assert PROBS[0] == 0.0 and PROBS[-1] == 1.0
        for h in hists:
            assert np.array_equal(h.lo, pop.P.min(axis=0)) and np.array_equal(h.hi, pop.P.max(axis=0))


CRAFTED_COLUMN = np.array([-0.0, 0.0, -1.0, 1.0, -5e-324, 5e-324, -1e150, 1e150, -2.5, 2.5, 1.0 + 2.0 ** -52])


def test_signed_zeros_denormals_and_extremes_in_a_row_spread_over_lanes(ops_of):
    """the crafted column of the two suites at d = 33, in the first column, the last one and one in between (one per chunk of
    16 quantile columns)"""
    d = 33
    spec, ops = ops_of(d)
    N = 5001
    rng = np.random.default_rng(3)
    values = rng.standard_normal((N, d))
    for k in (0, 16, 32):
        col = rng.choice(CRAFTED_COLUMN, N)
        col[:64] = np.repeat([-0.0, 0.0], 32)
        values[:, k] = col
    pop = weighted(spec, ops, N, rng, values=values, dead=0.2)
    assert (pop.Wns[:64] > 0).sum() > 32
    for probs in (PROBS, TIE_PROBS, PROBS37):
        check_wq(pop, probs, "crafted 33")
    pairs = [(0, 16), (16, 32), (0, 32), (1, 32)]
    h = check_hist(pop, dict(bins=33, pairs=pairs, bins2=33), "automatic")       # (-1e150, 1e150) in the crafted columns
    for k in (0, 16, 32):
        assert (h.lo[k], h.hi[k]) == (-1e150, 1e150)
    # explicit: -1, 0, 1 and +-2.5 on edges, -0.0 at lo = +0.0 of column 16, +-1e150 under and over
    rng_ = [(-2.5, 2.5) if k != 16 else (0.0, 2.5) for k in range(d)]
    h = check_hist(pop, dict(bins=10, range=rng_, pairs=pairs, bins2=5), "explicit")
    for k in (0, 16, 32):
        assert h.under[k] > 0 and h.over[k] > 0 and h.mass1[k][0] > 0 and h.mass1[k][-1] > 0
    assert (h.outside2 > 0).all()


@pytest.mark.parametrize("which", ["tile 1 dead", "only tile 1 live"])
@pytest.mark.parametrize("d", [3, 33])
def test_a_whole_tile_without_mass(ops_of, d, which):
    """the two cases of test_gpu_posterior_summary_edges.py::test_a_whole_tile_without_a_live_position for both kernels"""
    spec, ops = ops_of(d)
    N = 3 * TILE + 1
    rng = np.random.default_rng(d + 2)
    tile1 = (np.arange(N) // TILE) == 1
    mask = ~tile1 if which == "tile 1 dead" else tile1.copy()
    mask[N - 1] = which == "tile 1 dead"                         # the one position of the last tile
    mask[0] = which == "tile 1 dead"                             # (dyadic_weights keeps position 0 alive)
    pop = weighted(spec, ops, N, rng, mask=mask, dead=0.2)
    live = pop.Wns > 0
    assert live.sum() > 1000 and live[tile1].any() == (which == "only tile 1 live") and live[~tile1].any() == (which == "tile 1 dead")
    ref = check_wq(pop, what=(which, d))
    h = check_hist(pop, dict(bins=37, pairs="all", bins2=16), (which, d))
    assert ref[2] == h.n_mass == live.sum()


def test_weights_that_must_not_count():
    """-0.0, -1.0, NaN, +0.0 and 2^-70 (positive, but rint(w N 2^40) = 0: no mass) next to live weights at d = 33; the rows behind
    them hold NaN / 1e300, which would wreck a quantile or the automatic range"""
    d = 33
    spec = epa(spec_of(d))
    ops = HipOps(spec)
    try:
        N = 2 * TILE + 77
        rng = np.random.default_rng(d + 3)
        base = dyadic_weights(rng, N, dead=0.0)
        w = base.copy()
        not_counting = np.array([-0.0, -1.0, np.nan, 0.0, 2.0 ** -70])
        dead = rng.permutation(N)[:N // 2]
        w[dead] = np.resize(not_counting, dead.size)
        w[0:11:2], w[1:11:2] = base[0:11:2], not_counting        # one thread's neighbours, whatever the draw
        with np.errstate(invalid="ignore"):
            counts = (w > 0.0) & (w != 2.0 ** -70)
        assert counts[0] and (w[~counts & (w > 0)] == 2.0 ** -70).all() and (~counts).sum() >= N // 2
        values = rng.standard_normal((N, d))
        pop, P = crafted(spec, ops, values, w, rng, live=counts)
        assert (np.isnan(P[~counts]) | (P[~counts] == 1e300)).all()
        q, M, n_mass = ops.posterior_wquantiles(*pop, N, PROBS)
        assert_wq((q, M, n_mass), wquantiles_reference(P, w, PROBS), "weights")
        assert n_mass == counts.sum() and np.isfinite(q).all() and np.abs(q).max() < 10
        opts = dict(bins=37, pairs="all", bins2=16)
        h = device_hist(ops, pop, N, d, opts)
        assert_same_hist(h, hist_reference(P, w, **opts), "weights")
        assert_identities(h)
        assert (h.M, h.n_mass) == (M, n_mass) and (h.nan == 0).all() and (h.hi < 10).all()
    finally:
        ops.close()


# ------------------------------------------------------------------------------------------ 3. the second trip of every grid-stride loop

class Big:
    """N = 2^20 + 2049, d = 2, crafted: dyadic unequal weights, about 30 % dead and poisoned, both slots in use.  The smallest and
    the largest value of both columns, and the smallest mass at the smallest value, are at positions >= 2^20: only a second trip
    (of every loop below) finds v_1, m_(1), v_n, lo and hi."""
    N = (1 << 20) + 2049
    d = 2
    lo, hi = -7.5, 8.25

    def __init__(self):
        N, d = self.N, self.d
        self.spec = epa(spec_of(d))
        self.ops = HipOps(self.spec)
        rng = np.random.default_rng(20)
        w = dyadic_weights(rng, N)
        values = rng.standard_normal((N, d))
        at = (1 << 20) + np.array([5, 1300, 2048])                # smallest value twice, largest value once
        values[at[:2]] = self.lo
        values[at[2]] = self.hi
        unit = w[w > 0].min()
        w[at] = (3 * unit, unit / 2, 5 * unit)                   # m_(1): the smaller of the two masses at the smallest value
        assert np.abs(values).max() == self.hi and (w[w > 0] >= unit / 2).all() and (w == unit / 2).sum() == 1
        assert 0.25 * N < (w == 0).sum() < 0.35 * N and unequal_positive(w)
        self.w = w
        self.pop, self.P = crafted(self.spec, self.ops, values, w, rng)
        assert self.ops.layout()[0] == 2


@pytest.fixture(scope="module")
def big():
    b = Big()
    yield b
    b.ops.close()


def test_second_trip_of_the_histogram_range_and_bin_loops(big):
    """hist_range_kernel: min(ceil(N / ABZ_BLOCK), H_RANGE_BLOCKS) blocks stride gridDim.x * ABZ_BLOCK = 262 144 positions;
    hist_bin_kernel: min(ceil(Nld / ABZ_BLOCK), H_BIN_BLOCKS) blocks stride 1 048 576 = 2^20 positions.  N = 2^20 + 2049 is
    beyond both, and lo, hi are only found at positions >= 2^20.  (hist_pair_kernel wraps here as well: one batch, 128 blocks,
    1027 tiles.)"""
    N = big.N
    Nld = ceil_div(N, H_PAD) * H_PAD
    assert min(ceil_div(N, ABZ_BLOCK), H_RANGE_BLOCKS) * ABZ_BLOCK == 262144 < 1 << 20
    assert min(ceil_div(Nld, ABZ_BLOCK), H_BIN_BLOCKS) * ABZ_BLOCK == 1 << 20 < N
    assert ceil_div(Nld, H_TILE) > min(ceil_div(H_PASS_WORKGROUPS, 1), H_PASS_BLOCKS)
    opts = dict(bins=37, pairs="all", bins2=16)
    h = device_hist(big.ops, big.pop, N, big.d, opts)
    assert_same_hist(h, hist_reference(big.P, big.w, **opts), "big, automatic")
    assert_identities(h)
    assert (h.lo == big.lo).all() and (h.hi == big.hi).all() and (h.outside2 == 0).all() and (h.under + h.over + h.nan == 0).all()
    assert h.n_mass == (big.w > 0).sum()
    opts = dict(bins=37, range=[(-1.0, 2.0), (-3.0, 0.5)], pairs="all", bins2=16)      # mass under, over and outside
    h = device_hist(big.ops, big.pop, N, big.d, opts)
    assert_same_hist(h, hist_reference(big.P, big.w, **opts), "big, explicit")
    assert_identities(h)
    assert (h.under > 0).all() and (h.over > 0).all() and h.outside2[0] > 0


def test_second_trip_of_the_wquantile_gather_pass_and_close_loops(big):
    """wq_gather_kernel: min(ceil(N / ABZ_BLOCK), WQ_MAX_BLOCKS) blocks stride gridDim.x * ABZ_BLOCK = 524 288 positions;
    wq_pass_kernel: min(ceil(N / WQ_TILE), WQ_PASS_BLOCKS) blocks stride gridDim.x * WQ_TILE = 262 144; wq_close_kernel: the
    same grid strides gridDim.x * ABZ_BLOCK = 32 768.  One column (k0 = 1, nk = 1): the reference takes about 2 s a column."""
    N = big.N
    assert min(ceil_div(N, ABZ_BLOCK), WQ_MAX_BLOCKS) * ABZ_BLOCK == 524288 < 1 << 20
    npb = min(ceil_div(N, WQ_TILE), WQ_PASS_BLOCKS)
    assert npb * WQ_TILE == 262144 < 1 << 20 and npb * ABZ_BLOCK == 32768
    probs = PROBS + (0.31, 0.0, 1.0)
    q, M, n_mass = big.ops.posterior_wquantiles(*big.pop, N, probs, k0=1, nk=1)
    ref = wquantiles_reference(big.P[:, 1:2], big.w, probs)
    assert_wq((q, M, n_mass), ref, "big")
    assert q[0, 0] == big.lo and q[0, 4] == big.hi and q[0, 6] == big.lo and q[0, 7] == big.hi
    assert big.lo < q[0, 1] < q[0, 2] < q[0, 3] < big.hi and n_mass == (big.w > 0).sum()


def test_second_trip_of_the_pair_loop():
    """hist_pair_kernel at d = 33, N = 5001, all 528 pairs.  bins2 = 65: one pair a batch (B = 1), 528 batches, want =
    ceil(2048 / 528) = 4 blocks for 5 tiles, 18 MB of cells.  bins2 = 91: two row ranges a pair, 1056 batches, want = 2.  The
    whole last tile (the second trip of block 0 in both) is live with heavy weights."""
    d, N = 33, 5001
    n_pairs = d * (d - 1) // 2
    tiles = ceil_div(ceil_div(N, H_PAD) * H_PAD, H_TILE)
    for bins2, ranges in ((65, 1), (91, 2)):
        per = bins2 * bins2
        B = min(H2_CELLS // per, HB_K) if per <= H2_CELLS else 1
        R = bins2 if per <= H2_CELLS else H2_CELLS // bins2
        assert B == 1 and ceil_div(bins2, R) == ranges
        want = min(ceil_div(H_PASS_WORKGROUPS, n_pairs * ranges), H_PASS_BLOCKS)
        assert want == {65: 4, 91: 2}[bins2] < tiles == 5
    spec = epa(spec_of(d))
    ops = HipOps(spec)
    try:
        rng = np.random.default_rng(65)
        k = rng.integers(1, 1 << 10, N).astype(np.float64)
        k[rng.random(N) < 0.3] = 0.0
        last = np.arange(N) >= 4 * H_TILE
        k[last] = rng.integers(1 << 19, 1 << 20, last.sum())      # a block of mass in the last tile
        w = k / 2.0 ** np.ceil(np.log2(k.sum()))
        pop = synthetic(spec, N, rng, w > 0.0, weights=w, ops=ops)
        for bins2 in (65, 91):
            h = check_hist(pop, dict(bins=37, pairs="all", bins2=bins2), bins2)
            assert h.mass2.shape == (n_pairs, bins2, bins2) and (h.outside2 == 0).all()
            assert (h.mass2.sum(axis=(1, 2)) + h.outside2 == np.uint64(h.M)).all()
            assert 2 * sum(int(m) for m in np.rint(w[last] * N * 2.0 ** 40)) > h.M      # most of M is in the last tile
    finally:
        ops.close()


def test_second_trip_of_the_1d_loop(ops_of):
    """hist_1d_kernel at d = 256, bins = 4096, N = 9 * 1024 + 1: G = 5120 / 4099 = 1 column a group, 256 groups, want =
    ceil(2048 / 256) = 8 blocks for 10 tiles; 8 MB of cells, no pairs"""
    d, bins, N = 256, 4096, 9 * 1024 + 1
    G = min(H1_CELLS // (bins + 3), d)
    groups = ceil_div(d, G)
    tiles = ceil_div(ceil_div(N, H_PAD) * H_PAD, H_TILE)
    assert (G, groups, ceil_div(H_PASS_WORKGROUPS, groups), tiles) == (1, 256, 8, 10)
    spec, ops = ops_of(d)
    rng = np.random.default_rng(4096)
    pop = weighted(spec, ops, N, rng)
    assert (pop.Wns[8 * H_TILE:] > 0).sum() > 500                 # the two tiles of the second trip carry mass
    h = check_hist(pop, dict(bins=bins), "1-D wrap")
    assert (h.under + h.over + h.nan == 0).all() and (h.mass1.sum(axis=1) == np.uint64(h.M)).all()


# ------------------------------------------------------------------------------------------ 4. the shared workspace

def test_the_three_entry_points_share_one_growing_workspace():
    """one context at d = 33; sum_ws_reserve lays the workspace out differently in each entry point and grows it twice here:
    a small histogram, weighted quantiles at N = 3 * 2048 + 1 with 37 probabilities (three batches), a histogram with all pairs at
    bins2 = 65 (18 MB of cells), the moments and the type-7 quantiles, and the first histogram again.  The context has an
    Epanechnikov kernel, for which abcdez_posterior_quantiles takes no weight array: the fourth population has every position
    alive with the weight 1 / N, handed over as weights to the moments and as wns = NULL to the quantiles."""
    d = 33
    spec = epa(spec_of(d))
    ops = HipOps(spec)
    try:
        rng = np.random.default_rng(44)
        small = weighted(spec, ops, 300, rng)
        large = weighted(spec, ops, 3 * TILE + 1, rng)
        N = 2049
        equal = synthetic(spec, N, rng, np.ones(N, dtype=bool), ops=ops)
        o_small, o_pairs = dict(bins=4), dict(bins=37, pairs="all", bins2=65)
        call = lambda pop, opts: device_hist(ops, (pop.bits, pop.slot0, pop.slot1, pop.wns), pop.N, d, opts)
        first = call(small, o_small)
        wq = device_wq(large, PROBS37)
        pairs = call(large, o_pairs)
        mean, S, W, Q, n_pos = equal.moments()
        cols = (0, 16, 32)
        qs = np.stack([ops.posterior_quantiles(equal.bits, equal.slot0, equal.slot1, None, N, k, PROBS) for k in cols], axis=1)
        again = call(small, o_small)
        ref_small = hist_reference(small.P, small.Wns, **o_small)
        assert_same_hist(first, ref_small, "first")
        assert_same_hist(again, ref_small, "again")
        assert_same_hist(again, first, "the same bits")
        assert_identities(first)
        assert_wq(wq, wquantiles_reference(large.P, large.Wns, PROBS37), "wquantiles")
        assert_same_hist(pairs, hist_reference(large.P, large.Wns, **o_pairs), "pairs")
        assert_identities(pairs)
        ref = equal.reference(cols=cols)
        assert_same(make_summary(mean, S, W, Q, n_pos, qs, PROBS), ref, "moments and quantiles")
        assert n_pos == N and pairs.mass2.nbytes > 16 << 20
    finally:
        ops.close()
