"""Posterior summaries on the device (csrc/abz_summary.hip) where test_gpu_posterior_summary.py does not reach: rows wider than 32
doubles, populations no sampler produces, the growth of the calls' own buffer, and an exact-arithmetic yardstick.

Every comparison with abcdez_amd.summary.summary_reference is BIT FOR BIT (mean, S, W, Q, n_pos, cov, ess, quantiles: assert_same).
The synthetic populations are handed to the two C entry points as plain device pointers (bits, N, slot0, slot1, wns), the way
test_c_abi_refusals does with the engine's own buffers: both row slots in use at every width, the slot that is not current and
every dead row filled with NaN / +-inf, so that one missing guard in a kernel poisons a sum."""
import numpy as np
import pytest
import torch

import abcdez_amd as A
from abcdez_amd.engine import HipOps
from abcdez_amd.summary import make_summary, summary_reference
from test_gpu_posterior_summary import PROBS, assert_same, bits, model, run3
from test_posterior_summary import exact_yardstick, yardstick_population

pytestmark = pytest.mark.gpu

TILE = 2048
POISON = np.array([np.nan, np.inf, -np.inf])


class Synthetic:
    """a packed population on the device (bits, slot0, slot1, wns) with its host-side truth: ``rows`` (the current row of every
    position, poison at the dead ones), ``P`` (push_p of it) and ``Wns`` as uploaded"""

    def __init__(self, spec, ops, N, dbits, slot0, slot1, wns, rows, P, Wns):
        self.spec, self.ops, self.N, self.d = spec, ops, N, spec.d
        self.bits, self.slot0, self.slot1, self.wns = dbits, slot0, slot1, wns
        self.rows, self.P, self.Wns = rows, P, Wns

    def moments(self, want_second=True):
        return self.ops.posterior_moments(self.bits, self.slot0, self.slot1, self.wns, self.N, want_second=want_second)

    def quantiles(self, k, probs=PROBS):
        return self.ops.posterior_quantiles(self.bits, self.slot0, self.slot1, self.wns, self.N, k, probs)

    def summary(self, probs=PROBS, cols=None, corrected=True):
        """the record of engine.posterior_summary through the C ABI; quantiles of the columns ``cols`` only (None: all)"""
        mean, S, W, Q, n_pos = self.moments()
        cols = range(self.d) if cols is None else cols
        qs = np.empty((len(probs), len(cols)))
        for c, k in enumerate(cols):
            qs[:, c] = self.quantiles(k, probs)
        return make_summary(mean, S, W, Q, n_pos, qs, probs, corrected)

    def reference(self, probs=PROBS, cols=None, **kw):
        ref = summary_reference(self.P, self.Wns, quantiles=probs, **kw)
        if cols is not None:
            ref.quantiles = ref.quantiles[:, list(cols)]
        return ref


def synthetic(spec, N, rng, live, values=None, weights=None, ops=None):
    """A fully synthetic packed population for the model ``spec``.  ``live``: boolean mask of the positions that count;
    ``values``: (N, d) rows (default: normal draws with a few exact ties per column; the rows of dead positions are ignored);
    ``weights``: (N,) Wns uploaded as they are (default: 1 / N at the live positions, +0.0 elsewhere).  A random half of the
    bits are set; the slot that is not current at a live position holds NaN, both slots hold NaN / +-inf at a dead one, and the
    columns d .. ld - 1 hold 0.0, as the library keeps them."""
    ops = ops if ops is not None else HipOps(spec)
    d = spec.d
    ld = ops.layout()[0]
    assert d <= ld and ld == spec.ld
    live = np.asarray(live, dtype=bool)
    assert live.shape == (N,)
    if values is None:
        values = rng.standard_normal((N, d))
        if N > 8:
            for k in range(d):                                   # a few exact ties per column, the extrema among them now and then
                src = rng.integers(0, N, 3)
                values[rng.integers(0, N, 3), k] = values[src, k]
    values = np.ascontiguousarray(values, dtype=np.float64)
    assert values.shape == (N, d)
    if weights is None:
        weights = np.where(live, 1.0 / N, 0.0)
    weights = np.ascontiguousarray(weights, dtype=np.float64)
    assert np.array_equal(weights > 0.0, live), "live must be the positions with a positive weight"
    bit = rng.random(N) < 0.5
    if N > 1:
        bit[:2] = (False, True)                                   # both slots in use whatever the draw
    rows = np.where(live[:, None], values, np.resize(POISON, (N, d)))
    slots = [np.zeros((N, ld)), np.zeros((N, ld))]
    for s in (0, 1):
        cur = live & (bit == bool(s))
        slots[s][:, :d] = np.where(cur[:, None], values, np.where(live[:, None], np.nan, np.resize(POISON[::-1] if s else POISON, (N, d))))
    words = np.zeros((N + 31) // 32, dtype=np.uint32)
    idx = np.flatnonzero(bit)
    np.bitwise_or.at(words, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    dev = ops.device
    dbits = torch.from_numpy(words.view(np.int32)).to(dev)
    slot0, slot1 = (torch.from_numpy(s).to(dev) for s in slots)
    wns = torch.from_numpy(weights).to(dev)
    # the truth: push_p is rint on the discrete columns.  Cross-checked against the library's own push_p on the finite rows.
    P = rows.copy()
    disc = np.flatnonzero(np.array(spec.discrete, dtype=bool))
    P[:, disc] = np.rint(P[:, disc])
    cur_rows = torch.from_numpy(np.where(bit[:, None], slots[1], slots[0])).to(dev)
    pushed = torch.empty_like(cur_rows)
    ops.push_p(cur_rows, pushed)
    pushed = pushed.cpu().numpy()
    assert np.array_equal(bits(pushed[live, :d]), bits(P[live])), "the truth's P is not the library's push_p"
    assert (pushed[:, d:] == 0).all()
    return Synthetic(spec, ops, N, dbits, slot0, slot1, wns, rows, P, weights)


def spec_of(d, seed=1):
    prior, sim = model(d)
    return A.ModelSpec(prior, sim, A.IndicatorStrict0toϵ, seed=seed)


# ------------------------------------------------------------------------------------------ 2. wide rows, bit for bit

@pytest.mark.parametrize("d", [33, 64, 65, 100, 129, 200, 255, 256])
def test_wide_rows_of_a_real_run(d):
    """ld = 64, 128, 256 with 0 .. 56 PAD components; d = 33, 65, 129 end the second pass's jb and kb loops one column into a
    block of 4 and the first pass's cb loop one column into a block of 8; d = 255: 32 640 pairs, d = 256: 32 896"""
    N = 2049
    prior, sim = model(d)
    r = run3(prior, sim, N)
    assert r.engine.ops.layout()[0] == r.engine.spec.ld >= d
    dev = r.engine.posterior_summary(cov=True, corrected=True, quantiles=PROBS)
    ref = summary_reference(r.P, r.Wns, cov=True, corrected=True, quantiles=PROBS)
    assert_same(dev, ref, (d, N))
    assert dev.mean.shape == (d,) and dev.cov.shape == (d, d) and dev.quantiles.shape == (len(PROBS), d)
    unc = r.engine.posterior_summary(cov=True, corrected=False)
    assert np.array_equal(bits(unc.cov), bits(ref.S / ref.W)) and unc.quantiles.shape == (0, d)
    first = r.engine.posterior_summary(cov=False)
    assert first.cov is None and np.array_equal(bits(first.mean), bits(ref.mean))


def test_wide_rows_with_a_correlated_prior():
    """the MvNormal prior of test_wide_rows_end_to_end at d = 128"""
    d = 128
    rng = np.random.default_rng(5)
    Lm = np.tril(rng.normal(0, 0.05, (d, d)), -1) + np.diag(rng.uniform(0.8, 1.2, d))
    prior = A.MvNormal(rng.normal(0, 0.2, d), Lm @ Lm.T)
    r = run3(prior, A.MVNormal(tuple(1.0 for _ in range(d))), 2049)
    assert_same(r.engine.posterior_summary(quantiles=PROBS), summary_reference(r.P, r.Wns, quantiles=PROBS), "mvnormal 128")


def test_wide_rows_in_classic_storage():
    prior, sim = model(64)
    m = A.abcdemc(prior, sim, 0.5, None, nparticles=2049, generations=6, verbose=False, rng=5, summary=dict(quantiles=PROBS))
    ref = summary_reference(m.P, None, quantiles=PROBS)
    assert_same(m.summary, ref, "abcdemc 64")
    assert ref.n_pos == 2049 and ref.W == 2049.0 and ref.Q == 2049.0 and m.summary.mean.shape == (64,)


@pytest.fixture(scope="module")
def ops_of():
    """one context per row width for the synthetic cases (a context is independent of N)"""
    made = {}

    def get(d):
        if d not in made:
            spec = spec_of(d)
            made[d] = (spec, HipOps(spec))
        return made[d]
    yield get
    for _, ops in made.values():
        ops.close()


@pytest.mark.parametrize("N", [1, 2, 300, 2048, 2049, 3 * 2048 + 1])
@pytest.mark.parametrize("d", [5, 33, 255, 256])
def test_wide_synthetic_rows(ops_of, d, N):
    """the ragged ends of the cb / jb / kb loops and both slots at every width, independent of what a sampler leaves; d >= 255:
    quantiles of the columns 0, 1, d / 2, d - 2, d - 1 only"""
    spec, ops = ops_of(d)
    rng = np.random.default_rng(1000 * d + N)
    live = rng.random(N) < 0.7
    live[rng.integers(0, N)] = True
    pop = synthetic(spec, N, rng, live, ops=ops)
    cols = None if d < 255 else [0, 1, d // 2, d - 2, d - 1]
    ref = pop.reference(cols=cols)
    assert ref.n_pos == live.sum()
    assert_same(pop.summary(cols=cols), ref, (d, N))
    mean, S, W, Q, n_pos = pop.moments(want_second=False)
    assert S is None and np.array_equal(bits(mean), bits(ref.mean)) and (W, Q, n_pos) == (ref.W, ref.Q, ref.n_pos)


# ------------------------------------------------------------------------------------------ 3. crafted populations

CRAFTED_D = [3, 33]


@pytest.mark.parametrize("d", CRAFTED_D)
def test_a_single_positive_weight(ops_of, d):
    """n_pos = 1, N = 4099, the live position the last one (of a ragged tile): S identically zero, cov = 0 / (W - Q / W) = 0 / 0 =
    NaN on both sides, every quantile equal to the row (the quantile's `if (n == 1) b = a` branch).  The -0.0 component comes
    out as +0.0 on both sides: see test_posterior_summary.py, test_reference_with_a_single_positive_weight."""
    spec, ops = ops_of(d)
    N = 4099
    rng = np.random.default_rng(d)
    live = np.zeros(N, dtype=bool)
    live[N - 1] = True
    values = rng.standard_normal((N, d))
    values[N - 1, :3] = (1.5, -0.0, -2.25e-300)
    pop = synthetic(spec, N, rng, live, values=values, weights=live.astype(np.float64), ops=ops)
    probs = (0.0, 0.3, 0.5, 1.0)
    with np.errstate(invalid="ignore"):
        dev, ref = pop.summary(probs=probs), pop.reference(probs=probs)
    assert_same(dev, ref, ("n_pos 1", d))
    row = values[N - 1]
    assert dev.n_pos == 1 and dev.W == 1.0 and dev.Q == 1.0
    assert np.array_equal(dev.mean, row) and np.array_equal(dev.S, np.zeros((d, d))) and np.isnan(dev.cov).all() and np.isnan(ref.cov).all()
    for i in range(len(probs)):
        assert np.array_equal(dev.quantiles[i], row) and not np.signbit(dev.quantiles[i, 1])


@pytest.mark.parametrize("d", CRAFTED_D)
def test_two_positive_weights_in_different_tiles(ops_of, d):
    spec, ops = ops_of(d)
    N = 4099
    rng = np.random.default_rng(d + 1)
    live = np.zeros(N, dtype=bool)
    live[[0, TILE]] = True
    pop = synthetic(spec, N, rng, live, weights=np.where(live, 0.5, 0.0), ops=ops)
    probs = (0.0, 0.3, 0.5, 1.0)
    dev, ref = pop.summary(probs=probs), pop.reference(probs=probs)
    assert_same(dev, ref, ("n_pos 2", d))
    assert dev.n_pos == 2 and dev.W == 1.0 and dev.Q == 0.5
    lo, hi = pop.P[[0, TILE]].min(axis=0), pop.P[[0, TILE]].max(axis=0)
    assert np.array_equal(dev.quantiles[0], lo) and np.array_equal(dev.quantiles[3], lo + 1.0 * (hi - lo))     # n = 2: j stays 1, g = p


@pytest.mark.parametrize("which", ["tile 1 dead", "only tile 1 live"])
@pytest.mark.parametrize("d", CRAFTED_D)
def test_a_whole_tile_without_a_live_position(ops_of, d, which):
    spec, ops = ops_of(d)
    N = 3 * TILE + 1
    rng = np.random.default_rng(d + 2)
    live = rng.random(N) < 0.8
    tile1 = (np.arange(N) // TILE) == 1
    live = live & ~tile1 if which == "tile 1 dead" else live & tile1
    live[N - 1] = which == "tile 1 dead"                        # the one position of the last tile
    pop = synthetic(spec, N, rng, live, ops=ops)
    ref = pop.reference()
    assert ref.n_pos == live.sum() > 1000
    assert live[tile1].any() == (which == "only tile 1 live") and live[~tile1].any() == (which == "tile 1 dead")
    assert_same(pop.summary(), ref, (which, d))


@pytest.mark.parametrize("d", CRAFTED_D)
def test_weights_that_must_not_count(ops_of, d):
    """-0.0, -1.0, NaN and +0.0 next to live weights: `wv > 0.0` decides all of them; n_pos, W and Q ignore them, and the rows
    behind them hold NaN / +-inf"""
    spec, ops = ops_of(d)
    N = 2 * TILE + 77
    rng = np.random.default_rng(d + 3)
    w = np.full(N, 1.0 / N)
    dead = rng.permutation(N)[:N // 2]
    w[dead] = np.resize(np.array([-0.0, -1.0, np.nan, 0.0]), dead.size)
    w[:8] = (1.0 / N, -0.0, 1.0 / N, -1.0, 1.0 / N, np.nan, 1.0 / N, 0.0)      # one thread's neighbours, whatever the draw
    pop = synthetic(spec, N, rng, w > 0.0, weights=w, ops=ops)
    dev, ref = pop.summary(), pop.reference()
    assert_same(dev, ref, ("weights", d))
    n = int((w > 0.0).sum())
    assert dev.n_pos == n and abs(dev.W - n / N) <= 64 * 2.0 ** -53 * n / N and np.isfinite(dev.S).all() and np.isfinite(dev.quantiles).all()


@pytest.mark.parametrize("d", CRAFTED_D)
def test_unequal_and_subnormal_weights(ops_of, d):
    """Moments only, weights spread over 2^-40 .. 1 and some subnormal ones, whose squares underflow to 0 in Q.
    No quantiles are asked for here: the C entry point refuses weighted quantiles by the ABC kernel family of the model (abck),
    not by looking at the weights, while summary_reference refuses by looking at them -- on this population (an indicator kernel's
    model, unequal weights) the two would disagree about refusing.  That contract is not this test's business."""
    spec, ops = ops_of(d)
    N = 2 * TILE + 77
    rng = np.random.default_rng(d + 4)
    live = rng.random(N) < 0.7
    w = np.where(live, np.exp2(-40.0 * rng.random(N)), 0.0)
    sub = np.flatnonzero(live)[::7]
    w[sub] = np.resize(np.array([5e-324, 2.0 ** -1060, 3e-310]), sub.size)
    assert (w[sub] * w[sub] == 0).all()
    pop = synthetic(spec, N, rng, live, weights=w, ops=ops)
    mean, S, W, Q, n_pos = pop.moments()
    ref = pop.reference(probs=())
    assert_same(make_summary(mean, S, W, Q, n_pos, np.empty((0, d)), ()), ref, ("unequal", d))
    assert n_pos == live.sum() and np.isfinite(S).all()
    with pytest.raises(ValueError, match="weighted quantiles are not provided"):
        pop.reference(probs=(0.5,))


@pytest.mark.parametrize("d", CRAFTED_D)
def test_discrete_columns_with_halfway_values(ops_of, d):
    """Factored(Normal, DiscreteUniform(1, 10), Poisson(2.0)) (d = 33: followed by 30 more Normals); the discrete columns hold
    non-integers and half-way cases: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> -0.0, -1.5 -> -2.  rint on the device, np.rint in the
    truth; -0.0 sorts below +0.0 in the select."""
    prior = A.Factored(A.Normal(0.0, 1.0), A.DiscreteUniform(1, 10), A.Poisson(2.0), *[A.Normal(0.0, 1.0) for _ in range(d - 3)])
    spec = A.ModelSpec(prior, A.MVNormal(tuple([0.25] * d)), A.IndicatorStrict0toϵ, seed=1)
    assert spec.discrete[:3] == (False, True, True) and not any(spec.discrete[3:])
    N = TILE + 300
    rng = np.random.default_rng(d + 5)
    live = rng.random(N) < 0.7
    values = rng.standard_normal((N, d))
    half = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 0.49999999999999994, 0.2, -0.2, 3.7, 2.0 ** 51 + 0.5, 2.0 ** 52 + 1.0])
    values[:, 1] = rng.choice(half, N)
    values[:, 2] = rng.choice(half[:8], N)
    values[:, 0] = rng.choice(half[:5], N)                      # the same values in a continuous column stay as they are
    ops = HipOps(spec)
    try:
        pop = synthetic(spec, N, rng, live, values=values, ops=ops)
        P = pop.P[live]
        assert np.array_equal(P[:, 1], np.rint(P[:, 1])) and np.signbit(P[P[:, 2] == 0, 2]).any() and not np.signbit(P[P[:, 2] == 0, 2]).all()
        assert np.array_equal(bits(P[:, 0]), bits(values[live, 0]))
        for probs in (PROBS, (0.3, 0.31, 0.5, 0.52)):
            assert_same(pop.summary(probs=probs), pop.reference(probs=probs), ("discrete", d))
    finally:
        ops.close()


def test_signed_zeros_denormals_and_extremes_in_a_row_spread_over_lanes(ops_of):
    """the crafted column of test_gpu_posterior_summary.py at d = 33, in the first column, the last one and one in between"""
    d = 33
    spec, ops = ops_of(d)
    N = 5001
    rng = np.random.default_rng(3)
    live = rng.random(N) < 0.8
    live[:64] = True
    values = rng.standard_normal((N, d))
    for k in (0, 16, 32):
        col = rng.choice(np.array([-0.0, 0.0, -1.0, 1.0, -5e-324, 5e-324, -1e150, 1e150, -2.5, 2.5, 1.0 + 2.0 ** -52]), N)
        col[:64] = np.repeat([-0.0, 0.0], 32)
        values[:, k] = col
    pop = synthetic(spec, N, rng, live, values=values, ops=ops)
    for probs in (PROBS, (0.3, 0.31, 0.5, 0.52)):
        assert_same(pop.summary(probs=probs), pop.reference(probs=probs), "crafted 33")


# ------------------------------------------------------------------------------------------ 4. workspace growth

def test_the_summary_buffer_grows_between_calls():
    """one context, d = 256: a quantile at N = 2049 (a small request: the first 1 MiB), then the second moments at
    N = 4 * 2048 + 1 (32 896 trees x 5 tile partials x 8 bytes > 1 MiB: the buffer is freed and allocated anew), then the
    quantile again"""
    d = 256
    spec = spec_of(d)
    ops = HipOps(spec)
    try:
        rng = np.random.default_rng(4)
        small_N, big_N = 2049, 4 * TILE + 1
        small = synthetic(spec, small_N, rng, rng.random(small_N) < 0.7, ops=ops)
        big = synthetic(spec, big_N, rng, rng.random(big_N) < 0.7, ops=ops)
        k = d - 1
        q_first = small.quantiles(k)
        mean, S, W, Q, n_pos = big.moments()
        q_last = small.quantiles(k)
        ref_small = small.reference(cols=[k], cov=False)
        assert np.array_equal(bits(q_first), bits(ref_small.quantiles[:, 0]))
        assert np.array_equal(bits(q_first), bits(q_last))
        assert 256 * 257 // 2 * 5 * 8 > 1 << 20
        assert_same(make_summary(mean, S, W, Q, n_pos, np.empty((0, d)), ()), big.reference(probs=()), "grown")
    finally:
        ops.close()


# ------------------------------------------------------------------------------------------ 5. exact-arithmetic yardstick

def test_device_moments_meet_the_derived_bounds_against_exact_arithmetic():
    """the population of test_reference_meets_derived_bounds_against_exact_arithmetic (column 0 = 1e8 + 1e-3 normal, unequal
    weights, 30 % dead) uploaded as it is: the device meets the bounds derived in exact_yardstick (test_posterior_summary.py) AND
    equals the restatement bit for bit.  Moments only (unequal weights)."""
    X, w = yardstick_population()
    N, d = X.shape
    spec = spec_of(d)
    ops = HipOps(spec)
    try:
        pop = synthetic(spec, N, np.random.default_rng(6), w > 0.0, values=X, weights=w, ops=ops)
        mean, S, W, Q, n_pos = pop.moments()
    finally:
        ops.close()
    dev = make_summary(mean, S, W, Q, n_pos, np.empty((0, d)), ())
    worst = 0.0
    for what, err, bound in exact_yardstick(X, w, dev):
        print(what, float(err), float(bound), float(err / bound))
        assert err <= bound, what
        worst = max(worst, float(err / bound))
    print("worst error / bound on the device", worst)
    assert_same(dev, pop.reference(probs=()), "yardstick")
