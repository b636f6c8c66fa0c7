"""Posterior summaries: weighted mean, covariance, marginal quantiles, effective sample size.

What every test of the reference extracts from a result -- ``mean(r.P[r.Wns .> 0.0])`` (test/runtests.jl:159-162) of the
tuple of src/abcdez_smc.jl:388-393 / src/abcdez_mc.jl:166-171 -- and what an ABC user reports next to it.  The arithmetic
is fixed in include/abcdez_spec.h ("posterior summaries"): every sum is the tile tree over the population positions, no
fused multiply-add, exact order statistics.  The HIP library evaluates it on the device (csrc/abz_summary.hip);
:func:`summary_reference` is the numpy restatement of the same arithmetic, bit for bit -- the yardstick of the tests, and
what an engine without the device call (the CPU test engine) computes from its downloaded population.
"""
from __future__ import annotations

import bisect
import math
import struct
from builtins import range as builtins_range     # hist_reference has a `range` argument
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

TILE = 2048     # ABZ_TILE

WEIGHTED_QUANTILES = ("weighted quantiles are not provided: the positive weights differ (Epanechnikov kernels); "
                      "mean and covariance work for every kernel")


def tile_tree_sum(v):
    """The fixed tile tree of include/abcdez_spec.h over axis 0 of ``v`` (shape (n,) -> float, (n, m) -> array of m):
    tiles of 2048 consecutive elements; slot t < 256 of a tile owns the elements m*512 + 2t + c (m < 4, c < 2), summed as
    ((e00+e01)+(e10+e11))+((e20+e21)+(e30+e31)); the 256 slots are reduced by the pairwise binary tree over t; the tile
    partials are reduced by the same rule until one is left.  Missing elements are +0.0."""
    x = np.asarray(v, dtype=np.float64)
    scalar = x.ndim == 1
    x = x.reshape(x.shape[0], -1)
    if x.shape[0] < 1:
        raise ValueError("tile_tree_sum: nothing to sum")
    while True:
        n, m = x.shape
        nt = -(-n // TILE)
        e = np.zeros((nt * TILE, m))
        e[:n] = x
        e = e.reshape(nt, 4, 256, 2, m)
        s = ((e[:, 0, :, 0] + e[:, 0, :, 1]) + (e[:, 1, :, 0] + e[:, 1, :, 1])) + \
            ((e[:, 2, :, 0] + e[:, 2, :, 1]) + (e[:, 3, :, 0] + e[:, 3, :, 1]))
        while s.shape[1] > 1:
            s = s[:, 0::2] + s[:, 1::2]
        x = s[:, 0]
        if nt == 1:
            return float(x[0, 0]) if scalar else x[0].copy()


def order_keys(x):
    """order-preserving uint64 image of float64 values: the total order of the device's rank select (-0.0 below +0.0)"""
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


def quantile_type7_index(n: int, p: float):
    """(1-based index j of the lower order statistic, weight g of the upper one): abz_quantile_type7_index"""
    h = float(n - 1) * p + 1.0
    j = int(math.floor(h))
    j = max(j, 1)
    if j > n - 1:
        j = n - 1 if n - 1 > 1 else 1
    return j, h - float(j)


def cov_denominator(W: float, Q: float, corrected: bool) -> float:
    """abz_summary_cov_denominator: W, or W - Q / W (for uniform weights the n - 1 of the particles with Wns > 0)"""
    return W - Q / W if corrected else W


def _as_matrix(v):
    """float64 view of per-particle values with a vector lifted to one column: (N,) -> (N, 1)"""
    X = np.asarray(v, dtype=np.float64)
    return X[:, None] if X.ndim == 1 else X


def _options(who: str, value, allowed, named=None) -> dict:
    """a driver keyword that is True (the defaults) or a dict of the options ``allowed`` -> a copy of the dict.  ``named``: the
    options the two refusals list, where their wording is older than the newest options (default: all of them)"""
    named = allowed if named is None else named
    if value is True:
        return {}
    if isinstance(value, dict):
        bad = set(value) - set(allowed)
        if bad:
            raise ValueError(f"{who}: unknown option(s) {sorted(bad)} ({', '.join(named)})")
        return dict(value)
    raise ValueError(f"{who} must be None, True or a dict of the options {', '.join(named)}")


def engine_call(eng, method: str, fallback, **opts):
    """``eng.<method>(**opts)`` for a PopulationEngine; any other engine object: ``fallback(eng.result(), **opts)``, the numpy
    restatement on its downloaded result"""
    if hasattr(eng, method):
        return getattr(eng, method)(**opts)
    return fallback(eng.result(), **opts)


def make_summary(mean, S, W, Q, n_pos, quantiles, probs, corrected=True, wquantiles=None, wprobs=(), M=None, n_mass=None, hist=None):
    """the record ``posterior_summary`` returns, from what the library (or the restatement below) computes"""
    W, Q = float(W), float(Q)
    cov = None if S is None else np.asarray(S, dtype=np.float64) / cov_denominator(W, Q, corrected)
    if wquantiles is None:
        wquantiles = np.empty((0, np.asarray(mean).shape[0]))
    return SimpleNamespace(mean=np.asarray(mean, dtype=np.float64), cov=cov, S=S, W=W, Q=Q, ess=W * W / Q, n_pos=int(n_pos),
                           quantiles=quantiles, probs=tuple(probs), corrected=bool(corrected), wquantiles=wquantiles,
                           wprobs=tuple(wprobs), M=None if M is None else int(M), n_mass=None if n_mass is None else int(n_mass),
                           hist=hist)


def stratum_bits(n: int) -> int:
    """abz_stratum_bits: fraction bits of the resampler's fixed point, 40 up to 2^23 positions"""
    lg = 0
    while lg < 32 and (1 << lg) < n:
        lg += 1
    return 40 if lg <= 23 else 63 - lg


def weight_fix(w, n: int):
    """abz_weight_fix of every weight: rint(w n 2^b) as Python integers (a list); zero, negative and NaN weights carry no mass,
    the result saturates at 2^63"""
    b = stratum_bits(n)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.asarray(w, dtype=np.float64) * float(n) * (2.0 ** b)
    out = []
    for x in v.tolist():
        if not x > 0.0:
            out.append(0)
        elif x >= 2.0 ** 63:
            out.append(1 << 63)
        else:
            out.append(int(np.rint(x)))
    return out


def integer_masses(Wns, N: int, who: str = "summary"):
    """(masses, M, n_mass): the integer masses of the N positions (Python integers; abz_weight_fix of the weights, or 2^b each
    without weights), their total and the number of positions that count (mass >= 1).  Refuses like the library, under the
    prefix ``who``: no mass at all, or a total that reaches 2^63."""
    if Wns is None:
        masses = [1 << stratum_bits(N)] * N
    else:
        w = np.asarray(Wns, dtype=np.float64)
        if w.shape != (N,):
            raise ValueError(f"{who}: one weight per particle expected")
        masses = weight_fix(w, N)
    n_mass = sum(1 for m in masses if m >= 1)
    if n_mass < 1:
        raise ValueError(f"{who}: no particle has a positive weight that carries mass")
    M = sum(masses)
    if M >= 1 << 63:
        raise ValueError(f"{who}: the total mass reaches 2^63 -- the weights are not normalised")
    return masses, M, n_mass


def wquantile_column(values, masses, probs):
    """The weighted quantile of include/abcdez_spec.h ("posterior summaries", weighted quantiles) of ONE column, literally:
    ``values`` and ``masses`` (Python integers >= 1) of the counting positions; sort by (order key, mass), integer partial sums."""
    keys = order_keys(values).tolist()
    order = sorted(range(len(keys)), key=lambda i: (keys[i], masses[i]))
    v = [float(values[i]) for i in order]
    m = [masses[i] for i in order]
    n = len(v)
    cum, s = [], 0
    for x in m:
        s += x
        cum.append(s)                                   # S_1 .. S_n
    M = s
    out = []
    for p in probs:
        span = M - m[0]
        t = min(int(math.floor(p * float(span))), span)
        H = m[0] + t
        k = bisect.bisect_right(cum, H)                 # 0-based index of the smallest S_k > H
        if n == 1 or k >= n:
            out.append(v[n - 1])
            continue
        assert k >= 1
        g = float(H - cum[k - 1]) / float(m[k])
        out.append(float(np.float64(v[k - 1]) + np.float64(g) * (np.float64(v[k]) - np.float64(v[k - 1]))))
    return out


def wquantiles_reference(X, w, probs):
    """(wquantiles (len(probs) x d), M, n_mass) of the population X (N x d) with the weights w (None: every position has the
    mass 2^b); refuses like the library"""
    N, d = X.shape
    masses, M, n_mass = integer_masses(w, N)
    idx = [i for i in range(N) if masses[i] >= 1]
    ml = [masses[i] for i in idx]
    out = np.empty((len(probs), d))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(d):
            out[:, k] = wquantile_column(X[idx, k], ml, probs)
    return out, M, n_mass


HIST_MAX_BINS, HIST_MAX_BINS2 = 4096, 128      # ABZ_HIST_MAX_BINS, ABZ_HIST_MAX_BINS2
HIST_OPTIONS = ("bins", "range", "columns", "pairs", "bins2")


class Hist(SimpleNamespace):
    """the ``hist`` field of a summary record: ``columns`` (the requested parameters), ``lo`` / ``hi`` / ``edges`` (n_cols x
    (bins + 1), for drawing), ``mass1`` (uint64, n_cols x bins) with the tallies ``under`` / ``over`` / ``nan``, ``pairs``,
    ``bins2``, ``edges2``, ``mass2`` (uint64, n_pairs x bins2 x bins2, [pair][b_j][b_k]), ``outside2``, ``M``, ``n_mass``"""

    def density(self):
        """mass1 / M / bin width as float64 (n_cols x bins): a convenience for drawing, not pinned bit for bit"""
        width = (self.hi - self.lo) / float(self.bins)
        return self.mass1.astype(np.float64) / float(self.M) / width[:, None]


def hist_edges(lo, hi, bins):
    """edges[c][j] = lo + j ((hi - lo) / bins), edges[c][bins] = hi"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    e = lo[:, None] + np.arange(bins + 1, dtype=np.float64)[None, :] * ((hi - lo) / float(bins))[:, None]
    e[:, bins] = hi
    return e


def make_hist(columns, bins, lo_hi, mass1, tallies1, pairs, bins2, mass2, outside2, M, n_mass):
    """the ``hist`` record from what the library (or the restatement below) computes"""
    lo_hi = np.asarray(lo_hi, dtype=np.float64).reshape(len(columns), 2)
    lo, hi = lo_hi[:, 0].copy(), lo_hi[:, 1].copy()
    t = np.asarray(tallies1, dtype=np.uint64).reshape(len(columns), 3)
    has2 = len(pairs) > 0
    return Hist(columns=tuple(int(c) for c in columns), bins=int(bins), lo=lo, hi=hi, edges=hist_edges(lo, hi, bins),
                mass1=np.asarray(mass1, dtype=np.uint64).reshape(len(columns), bins), under=t[:, 0].copy(), over=t[:, 1].copy(),
                nan=t[:, 2].copy(), pairs=tuple((int(j), int(k)) for j, k in pairs), bins2=int(bins2) if has2 else None,
                edges2=hist_edges(lo, hi, bins2) if has2 else None,
                mass2=np.asarray(mass2, dtype=np.uint64).reshape(len(pairs), bins2, bins2) if has2 else np.zeros((0, 0, 0), np.uint64),
                outside2=np.asarray(outside2, dtype=np.uint64).reshape(len(pairs)) if has2 else np.zeros(0, np.uint64),
                M=int(M), n_mass=int(n_mass))


def hist_options(hist, d: int):
    """the ``hist`` option (a dict of bins / range / columns / pairs / bins2, or True for the defaults) checked against the limits
    of include/abcdez_spec.h ("histograms") -> (columns, bins, range (n_cols x 2) or None, pairs, bins2).  ``columns`` may come in
    any order and are returned sorted (the order of every per-column field of the record); a per-column ``range`` is given in the
    caller's order of ``columns`` and its rows are sorted along with them."""
    if hist is True:
        hist = {}
    if not isinstance(hist, dict):
        raise ValueError("summary: hist must be True or a dict of the options bins, range, columns, pairs, bins2")
    bad = set(hist) - set(HIST_OPTIONS)
    if bad:
        raise ValueError(f"summary: unknown hist option(s) {sorted(bad)} (bins, range, columns, pairs, bins2)")
    bins = int(hist.get("bins", 64))
    if not 1 <= bins <= HIST_MAX_BINS:
        raise ValueError("summary: hist bins must be in 1 .. 4096")
    cols = hist.get("columns")
    asked = list(range(d)) if cols is None else [int(c) for c in cols]      # the caller's order: that of a per-column range
    cols = sorted(asked)
    if not cols or len(set(cols)) != len(cols) or cols[0] < 0 or cols[-1] >= d:
        raise ValueError("summary: hist columns must be distinct parameter indices in 0 .. length(prior) - 1")
    rng_ = hist.get("range")
    if rng_ is not None:
        rng_ = np.array(rng_, dtype=np.float64)
        if rng_.shape == (2,):
            rng_ = np.tile(rng_, (len(cols), 1))
        if rng_.shape != (len(cols), 2):
            raise ValueError("summary: hist range must be (lo, hi) or one (lo, hi) per requested column")
        with np.errstate(over="ignore", invalid="ignore"):
            ok = np.isfinite(rng_).all() and (rng_[:, 0] < rng_[:, 1]).all() and np.isfinite(rng_[:, 1] - rng_[:, 0]).all()
        if not ok:
            raise ValueError("summary: a hist range must be finite with lo < hi and hi - lo finite")
        rng_ = np.ascontiguousarray(rng_[[asked.index(c) for c in cols]])      # row i belongs to columns[i] as given: sorted along
    pairs = hist.get("pairs")
    if pairs is None:
        pairs = []
    elif isinstance(pairs, str):
        if pairs != "all":
            raise ValueError('summary: hist pairs must be None, "all" or a list of (j, k)')
        if d < 2:
            raise ValueError("summary: hist pairs need at least two parameters")
        pairs = [(j, k) for a, j in enumerate(cols) for k in cols[a + 1:]]
    else:
        pairs = [(int(j), int(k)) for j, k in pairs]
        if pairs and d < 2:
            raise ValueError("summary: hist pairs need at least two parameters")
        for j, k in pairs:
            if not (0 <= j < k < d):
                raise ValueError("summary: a hist pair (j, k) needs two distinct columns with j < k")
            if j not in cols or k not in cols:
                raise ValueError("summary: both columns of a hist pair must be among the requested columns")
        if len(set(pairs)) != len(pairs):
            raise ValueError("summary: a hist pair must not be listed twice")
    bins2 = hist.get("bins2")
    bins2 = min(bins, HIST_MAX_BINS2) if bins2 is None else int(bins2)
    if pairs and not 1 <= bins2 <= HIST_MAX_BINS2:
        raise ValueError("summary: hist bins2 must be in 1 .. 128")
    return cols, bins, rng_, pairs, bins2


def hist_bin(x, lo: float, hi: float, scale: float, bins: int):
    """abz_hist_bin of every x: 0 .. bins - 1, or bins (under), bins + 1 (over), bins + 2 (NaN)"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.floor((x - lo) * scale)                     # one subtraction, one multiplication, a floor
        b = np.where(f >= float(bins), float(bins - 1), np.where(f >= 1.0, f, 0.0)).astype(np.int64)
        return np.where(x != x, bins + 2, np.where(x < lo, bins, np.where(x > hi, bins + 1, b)))


def hist_reference(X, w, bins=64, range=None, columns=None, pairs=None, bins2=None):
    """The histograms of include/abcdez_spec.h ("posterior summaries", histograms) of the population X (N x d) with the weights w
    (None: every position has the mass 2^b), literally: Python-integer masses, abz_hist_bin, integer sums.  Returns the record
    of :func:`make_hist`; refuses like the library."""
    X = _as_matrix(X)
    N, d = X.shape
    cols, bins, rng_, pairs, bins2 = hist_options(dict(bins=bins, range=range, columns=columns, pairs=pairs, bins2=bins2), d)
    masses, M, n_mass = integer_masses(w, N)
    idx = [i for i in builtins_range(N) if masses[i] >= 1]
    m = np.array([masses[i] for i in idx], dtype=np.uint64)        # every mass and every sum is below 2^63: exact in uint64
    nc = len(cols)
    lo_hi = np.empty((nc, 2))
    codes1 = np.empty((nc, len(idx)), dtype=np.int64)
    codes2 = np.empty((nc, len(idx)), dtype=np.int64)
    for c, k in enumerate(cols):
        x = X[idx, k]                                              # rows that do not count are never read
        if rng_ is None:
            keys = order_keys(x)
            lo, hi = float(x[np.argmin(keys)]), float(x[np.argmax(keys)])
            if lo == hi:
                lo, hi = lo - 0.5, hi + 0.5
            with np.errstate(over="ignore", invalid="ignore"):
                if not (lo < hi and math.isfinite(lo) and math.isfinite(hi) and math.isfinite(hi - lo)):
                    raise ValueError(f"summary: the automatic range of column {k} is not usable (a NaN or an infinity among the "
                                     "counting rows, or hi - lo not finite): pass a range")
        else:
            lo, hi = float(rng_[c, 0]), float(rng_[c, 1])
        lo_hi[c] = lo, hi
        codes1[c] = hist_bin(x, lo, hi, float(bins) / (hi - lo), bins)
        codes2[c] = hist_bin(x, lo, hi, float(bins2) / (hi - lo), bins2)
    cells1 = np.zeros((nc, bins + 3), dtype=np.uint64)
    for c in builtins_range(nc):
        np.add.at(cells1[c], codes1[c], m)
    mass2 = np.zeros((len(pairs), bins2 * bins2), dtype=np.uint64)
    outside2 = np.zeros(len(pairs), dtype=np.uint64)
    where = {k: c for c, k in enumerate(cols)}
    for q, (j, k) in enumerate(pairs):
        bj, bk = codes2[where[j]], codes2[where[k]]
        inside = (bj < bins2) & (bk < bins2)
        np.add.at(mass2[q], bj[inside] * bins2 + bk[inside], m[inside])
        outside2[q] = m[~inside].sum(dtype=np.uint64)
    return make_hist(cols, bins, lo_hi, cells1[:, :bins], cells1[:, bins:], pairs, bins2, mass2, outside2, M, n_mass)


def summary_reference(P, Wns=None, cov=True, corrected=True, quantiles=(), wquantiles=(), hist=None):
    """numpy restatement of the summary arithmetic.  ``P``: the push_p-cast population, shape (N,) or (N, d) (``r.P``);
    ``Wns``: the weights (``r.Wns``), or None for unit weights (abcdemc).  Returns the record of :func:`make_summary`:
    ``mean`` (d), ``cov`` (d x d, or None), ``S`` (the unnormalised second central moments), ``quantiles``
    (len(quantiles) x d), ``W``, ``Q``, ``ess = W^2 / Q``, ``n_pos``, and for ``wquantiles`` the weighted quantiles ``wquantiles``
    (len(wquantiles) x d) with the total integer mass ``M`` and ``n_mass`` (both None when none are asked for), and for ``hist``
    (the options of :func:`hist_reference`) the record ``hist`` of the marginal and pairwise histograms (None otherwise)."""
    X = _as_matrix(P)
    N, d = X.shape
    w = np.ones(N) if Wns is None else np.asarray(Wns, dtype=np.float64)
    if w.shape != (N,):
        raise ValueError("summary: one weight per particle expected")
    probs = tuple(float(p) for p in quantiles)
    wprobs = tuple(float(p) for p in wquantiles)
    if any(not 0.0 <= p <= 1.0 for p in probs + wprobs):
        raise ValueError("summary: p must be in [0, 1]")
    live = w > 0.0
    n_pos = int(live.sum())
    if n_pos < 1:
        raise ValueError("summary: no particle has a positive weight")
    wl = np.where(live, w, 0.0)
    Xl = np.where(live[:, None], X, 0.0)                 # dead rows may hold anything: never read for their value
    W = tile_tree_sum(wl)
    Q = tile_tree_sum(wl * wl)
    mean = tile_tree_sum(wl[:, None] * Xl) / W
    S = None
    if cov:
        C = Xl - mean
        S = np.empty((d, d))
        for j in range(d):
            terms = np.where(live[:, None], wl[:, None] * (C[:, j:j + 1] * C[:, j:]), 0.0)
            S[j, j:] = tile_tree_sum(terms)
            S[j:, j] = S[j, j:]
    qs = np.empty((len(probs), d))
    if probs:
        wpos = w[live]
        if not np.all(wpos == wpos[0]):
            raise ValueError(WEIGHTED_QUANTILES)
        for k in range(d):
            vals = X[live, k]
            vals = vals[np.argsort(order_keys(vals), kind="stable")]
            for i, p in enumerate(probs):
                j, g = quantile_type7_index(n_pos, p)
                a = vals[j - 1]
                b = vals[j] if n_pos > 1 else a
                qs[i, k] = a + g * (b - a)
    wq = M = n_mass = None
    if wprobs:
        wq, M, n_mass = wquantiles_reference(X, None if Wns is None else w, wprobs)
    h = None
    if hist is not None and hist is not False:
        hist_options(hist, d)
        h = hist_reference(X, None if Wns is None else w, **({} if hist is True else hist))
        M, n_mass = h.M, h.n_mass
    return make_summary(mean, S, W, Q, n_pos, qs, probs, corrected, wq, wprobs, M, n_mass, h)


# ------------------------------------------------------------------ posterior sample (include/abcdez_spec.h, "POSTERIOR SAMPLE")
RNG_SAMPLE = 10                 # ABZ_RNG_SAMPLE
SAMPLE_MAX_N = (1 << 31) - 1    # ABZ_SAMPLE_MAX_N
SAMPLE_OPTIONS = ("n", "draw", "blobs")
SUMMARY_OPTIONS = ("cov", "corrected", "quantiles", "wquantiles", "hist")
_MASK32 = 0xFFFFFFFF


def philox4x32(ctr, key, rounds: int = 10):
    """Philox4x32-R (Salmon et al., SC'11) of the counter (c0, c1, c2, c3) under the key (k0, k1) in Python integers:
    abz_philox4x32 of include/abcdez_spec.h"""
    c0, c1, c2, c3 = (int(v) & _MASK32 for v in ctr)
    k0, k1 = (int(v) & _MASK32 for v in key)
    for _ in range(rounds):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & _MASK32
        k0, k1 = (k0 + 0x9E3779B9) & _MASK32, (k1 + 0xBB67AE85) & _MASK32
    return [c0, c1, c2, c3]


def abz_rng(seed: int, idx: int, epoch: int, sub: int, purpose: int, rounds: int = 10):
    """abz_rng: the two 64-bit words of the Philox block addressed by (idx, epoch, sub, purpose) under the 64-bit seed"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r = philox4x32((idx, epoch, sub, purpose), (seed & _MASK32, seed >> 32), rounds)
    return (r[1] << 32) | r[0], (r[3] << 32) | r[2]


def sample_reference(P, Wns, n, seed, draw: int = 0, rounds: int = 10):
    """The posterior sample of include/abcdez_spec.h ("posterior summaries", POSTERIOR SAMPLE), literally and in Python integers:
    ``(index, M, n_mass)`` with ``index`` (int64, n) the positions drawn for the strata 0 .. n - 1 -- ``P[index]`` is the sample.
    ``P``: the population (only its length is used; an int N is accepted), ``Wns``: the weights or None (abcdemc: unit masses),
    ``seed``: the run's 64-bit seed (``rng=``), ``rounds``: the Philox rounds of the stream (``abcdez_rng_rounds()``).  Refuses like
    the library."""
    N = int(P) if isinstance(P, (int, np.integer)) else int(np.asarray(P).shape[0])
    n = int(n)
    if N < 1:
        raise ValueError("sample: the population is empty")
    if not 1 <= n <= SAMPLE_MAX_N:
        raise ValueError("sample: n must be in 1 .. 2^31 - 1")
    masses, M, n_mass = integer_masses(Wns, N, "sample")
    if n > M:
        raise ValueError("sample: n exceeds the total mass M")
    q, r = divmod(M, n)
    index = np.empty(n, dtype=np.int64)
    if Wns is None:
        b = stratum_bits(N)
        cum = None
    else:
        cum, c = [], 0
        for m in masses:
            c += m
            cum.append(c)                                  # C_i, inclusive
    draw = int(draw) & _MASK32
    for s in range(n):
        a = s * q + min(s, r)
        h = q + (1 if s < r else 0)
        u = abz_rng(seed, s, draw, 0, RNG_SAMPLE, rounds)[0]
        R = a + ((u * h) >> 64)
        index[s] = (R >> b) if cum is None else bisect.bisect_right(cum, R)      # the smallest i with C_i > R
    return index, M, n_mass


def sample_options(sample) -> dict:
    """the ``sample=`` keyword of the drivers: an integer n, or a dict of n / draw / blobs -> the keywords of posterior_sample"""
    if isinstance(sample, (bool, float)) or sample is None:
        raise ValueError("sample must be None, an integer n or a dict of the options n, draw, blobs")
    if isinstance(sample, (int, np.integer)):
        sample = {"n": int(sample)}
    if not isinstance(sample, dict):
        raise ValueError("sample must be None, an integer n or a dict of the options n, draw, blobs")
    bad = set(sample) - set(SAMPLE_OPTIONS)
    if bad:
        raise ValueError(f"sample: unknown option(s) {sorted(bad)} (n, draw, blobs)")
    if "n" not in sample:
        raise ValueError("sample: the number of draws n is required")
    n, draw, blobs = sample["n"], sample.get("draw", 0), sample.get("blobs")
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= SAMPLE_MAX_N:
        raise ValueError("sample: n must be an integer in 1 .. 2^31 - 1")
    if isinstance(draw, bool) or not isinstance(draw, (int, np.integer)) or not 0 <= int(draw) <= _MASK32:
        raise ValueError("sample: draw must be an integer in 0 .. 2^32 - 1")
    if blobs not in (None, True, False):
        raise ValueError("sample: blobs must be None, True or False")
    return {"n": int(n), "draw": int(draw), "blobs": blobs}


def make_sample(P, index, C, blobs, M, n_mass, n, draw):
    """the record ``posterior_sample`` returns"""
    return SimpleNamespace(P=P, index=np.asarray(index, dtype=np.int64), C=C, blobs=blobs, M=int(M), n_mass=int(n_mass), n=int(n),
                           draw=int(draw))


def engine_sample(eng, n, draw=0, blobs=None):
    """``eng.posterior_sample(n, draw, blobs)`` for a PopulationEngine; any other engine object: the restatement on its result"""
    def restated(res, n, draw, blobs):
        index, M, n_mass = sample_reference(res["P"], res.get("Wns"), n, eng.spec.seed, draw)
        rb = res.get("blobs")
        if blobs and rb is None:
            raise ValueError("sample: blobs=True needs a simulator that returns blobs")
        return make_sample(res["P"][index], index, res["C"][index], None if (rb is None or blobs is False) else rb[index], M, n_mass,
                           n, draw)
    return engine_call(eng, "posterior_sample", restated, n=n, draw=draw, blobs=blobs)


def summary_options(summary) -> dict:
    """the ``summary=`` keyword of the drivers: True, or a dict of cov / corrected / quantiles / wquantiles / hist"""
    return _options("summary", summary, SUMMARY_OPTIONS)


def engine_summary(eng, **opts):
    """``eng.posterior_summary(**opts)`` for a PopulationEngine; any other engine object: the restatement on its result"""
    return engine_call(eng, "posterior_summary", lambda res, **o: summary_reference(res["P"], res.get("Wns"), **o), **opts)


# ------------------------------------------------------------------ posterior predictive (include/abcdez_spec.h, "column summaries")
PREDICTIVE_OPTIONS = ("cov", "corrected", "wquantiles", "hist")
PREDICTIVE_NEEDS_BLOBS = "predictive: needs a simulator that returns blobs (blobs=True)"


def predictive_options(predictive) -> dict:
    """the ``predictive=`` keyword of the drivers: True, or a dict of cov / corrected / wquantiles / hist -> the keywords of
    posterior_predictive"""
    return _options("predictive", predictive, PREDICTIVE_OPTIONS)


def predictive_reference(blobs, Wns=None, cov=False, corrected=True, wquantiles=(), hist=None):
    """numpy restatement of the posterior predictive summary: :func:`summary_reference` of the simulated data ``blobs`` (``r.blobs``:
    (N,) for one number per particle, else (N, n_blob)) under the weights ``Wns`` (``r.Wns``; None: unit weights, abcdemc).  The
    values are taken as they are; rows of particles without weight may hold anything.  ``quantiles`` of the record is empty."""
    if blobs is None:
        raise ValueError(PREDICTIVE_NEEDS_BLOBS)
    X = _as_matrix(blobs)
    if X.ndim != 2:
        raise ValueError("predictive: blobs must be one row of numbers per particle")
    return summary_reference(X, Wns, cov=cov, corrected=corrected, quantiles=(), wquantiles=wquantiles, hist=hist)


def engine_predictive(eng, **opts):
    """``eng.posterior_predictive(**opts)`` for a PopulationEngine; any other engine object: the restatement on its result"""
    return engine_call(eng, "posterior_predictive", lambda res, **o: predictive_reference(res.get("blobs"), res.get("Wns"), **o), **opts)


# ------------------------------------------------------------------ regression adjustment (include/abcdez_spec.h, "REGRESSION ADJUSTMENT")
ADJUST_OPTIONS = ("columns", "target", "ridge", "cov", "corrected", "wquantiles", "hist", "rows", "hcorr", "transform")
ADJUST_NEEDS_BLOBS = "adjust: needs a simulator that returns blobs (blobs=True)"
ADJUST_MAX_C = 256              # ABZ_ADJUST_MAX_C
ADJUST_PIVOT = 2.0 ** -40       # a pivot must exceed this fraction of its diagonal entry


def adjust_options(adjust) -> dict:
    """the ``adjust=`` keyword of the drivers: True, or a dict of columns / target / ridge / cov / corrected / wquantiles / hist /
    rows / hcorr / transform -> the keywords of posterior_adjusted"""
    return _options("adjust", adjust, ADJUST_OPTIONS, ADJUST_OPTIONS[:8])      # the refusals keep their wording of version 670


def adjust_columns(columns, n_blob: int):
    """the ``columns`` option -> a list of blob columns, strictly increasing in 0 .. n_blob - 1 (None: all)"""
    cols = list(range(n_blob)) if columns is None else [int(c) for c in columns]
    if not 1 <= len(cols) <= ADJUST_MAX_C or cols[0] < 0 or cols[-1] >= n_blob or any(a >= b for a, b in zip(cols, cols[1:])):
        raise ValueError("adjust: columns must be strictly increasing blob columns in 0 .. n_blob - 1, at most 256 of them")
    return cols


def adjust_target(target, columns, n_blob: int, data=None):
    """the ``target`` option -> the c doubles t: one per chosen column.  None: ``data`` (the simulator's ``data()``) when it has one
    number per blob column, restricted to ``columns``; otherwise a target is required."""
    if target is None:
        if data is None or len(data) != n_blob:
            raise ValueError("adjust: target is required (the simulator's data are not one number per blob column)")
        t = np.asarray(data, dtype=np.float64)[list(columns)]
    else:
        t = np.atleast_1d(np.asarray(target, dtype=np.float64))
        if t.shape != (len(columns),):
            raise ValueError(f"adjust: target must hold {len(columns)} number(s), one per chosen blob column")
    if not np.isfinite(t).all():
        raise ValueError("adjust: the target is not finite")
    return np.ascontiguousarray(t)


def adjust_ridge(ridge) -> float:
    r = float(ridge)
    if not (0.0 <= r < math.inf):
        raise ValueError("adjust: ridge must be finite and not negative")
    return r


ADJUST_NOT_FINITE = "adjust: a moment of the simulated data is not finite (a NaN or an infinity in the blobs of a particle that counts)"


def adjust_check_means(s_mean, x_mean):
    """the means both passes centre on must be finite: refused before the cross pass"""
    if not (np.isfinite(s_mean).all() and np.isfinite(x_mean).all()):
        raise ValueError(ADJUST_NOT_FINITE)


def adjust_solve(S_ss, S_sx, ridge: float = 0.0, columns=None):
    """The single solve of the regression adjustment (include/abcdez_spec.h, "REGRESSION ADJUSTMENT"), in plain double, literally:
    ``S_ss`` (c x c: the second central moments of the chosen blob columns), ``S_sx`` (c x d) -> beta (c x d) with
    (S_ss + ridge diag(S_ss)) beta = S_sx, by a row-by-row Cholesky factorisation and a forward and a back substitution per column,
    every sum in ascending index from +0.0, no contraction.  ``columns`` only names the blob columns in the refusal."""
    A = np.array(S_ss, dtype=np.float64)
    B = np.array(S_sx, dtype=np.float64)
    if B.ndim == 1:
        B = B[:, None]
    c = A.shape[0]
    if A.shape != (c, c) or B.shape[0] != c or c < 1:
        raise ValueError("adjust: S_ss must be c x c and S_sx c x d")
    ridge = adjust_ridge(ridge)
    if not (np.isfinite(A).all() and np.isfinite(B).all()):
        raise ValueError(ADJUST_NOT_FINITE)
    names = list(range(c)) if columns is None else list(columns)
    a = A.tolist()
    for j in range(c):
        a[j][j] = a[j][j] * (1.0 + ridge)
    L = [[0.0] * c for _ in range(c)]
    for j in range(c):
        Lj = L[j]
        for k in range(j):
            Lk = L[k]
            s = 0.0
            for p in range(k):
                s = s + Lj[p] * Lk[p]
            Lj[k] = (a[j][k] - s) / Lk[k]
        s = 0.0
        for p in range(j):
            s = s + Lj[p] * Lj[p]
        r = a[j][j] - s
        if not (math.isfinite(r) and r > ADJUST_PIVOT * a[j][j]):
            raise ValueError(f"adjust: the simulated data are collinear or constant in column {names[j]}: pass `ridge` or fewer `columns`")
        Lj[j] = math.sqrt(r)
    Ln = np.array(L)
    with np.errstate(over="ignore", invalid="ignore"):
        Z = np.empty_like(B)                            # L z = b: every column k at once, element for element the scalar recurrence
        for j in range(c):
            s = np.zeros(B.shape[1])
            for p in range(j):
                s = s + Ln[j, p] * Z[p]
            Z[j] = (B[j] - s) / Ln[j, j]
        beta = np.empty_like(B)                         # L^T beta = z
        for j in range(c - 1, -1, -1):
            s = np.zeros(B.shape[1])
            for p in range(j + 1, c):
                s = s + Ln[p, j] * beta[p]
            beta[j] = (Z[j] - s) / Ln[j, j]
    if not np.isfinite(beta).all():
        raise ValueError("adjust: a regression coefficient is not finite")
    return beta


def adjust_apply(X, B, live, target, beta):
    """Y (N x d): row i = x_i - sum_j beta[j] (B[i, j] - target[j]), j ascending from +0.0, one subtraction, one multiplication and
    one addition per term, for the rows with ``live``; +0.0 for the others, whose inputs are never read"""
    Xl = np.where(live[:, None], X, 0.0)
    Bl = np.where(live[:, None], B, 0.0)
    acc = np.zeros_like(Xl)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(B.shape[1]):
            acc = acc + beta[j][None, :] * (Bl[:, j] - target[j])[:, None]
        return np.where(live[:, None], Xl - acc, 0.0)


# ---- transforms and the heteroscedastic correction (include/abcdez_spec.h, "REGRESSION ADJUSTMENT": TRANSFORM, HETEROSCEDASTIC CORRECTION)
TF_NONE, TF_LOG, TF_LOGIT = 0, 1, 2             # ABZ_ADJUST_TF_*
_TF_NAMES = {TF_NONE: "identity", TF_LOG: "log", TF_LOGIT: "logit"}


def adjust_hcorr(hcorr) -> bool:
    """the ``hcorr`` option: False or True"""
    if not isinstance(hcorr, (bool, np.bool_)):
        raise ValueError("adjust: hcorr must be False or True")
    return bool(hcorr)


def _transform_entry(entry):
    if entry is None:
        return TF_NONE, 0.0, 0.0
    if isinstance(entry, str):
        if entry == "log":
            return TF_LOG, 0.0, 0.0
        if entry == "logit":
            raise ValueError('adjust: transform: a logit needs its bounds, ("logit", lo, hi)')
        raise ValueError(f'adjust: transform: unknown transform {entry!r} (None, "log" or ("logit", lo, hi))')
    if isinstance(entry, (tuple, list)) and len(entry) == 3 and entry[0] == "logit":
        try:
            lo, hi = float(entry[1]), float(entry[2])
        except (TypeError, ValueError):
            raise ValueError('adjust: transform: the bounds of ("logit", lo, hi) must be numbers') from None
        if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
            raise ValueError('adjust: transform: ("logit", lo, hi) needs finite bounds with lo < hi')
        return TF_LOGIT, lo, hi
    raise ValueError(f'adjust: transform: unknown transform {entry!r} (None, "log" or ("logit", lo, hi))')


def adjust_transform(transform, d: int):
    """the ``transform`` option -> None (every transform is the identity) or (kind int32[d], lo_hi float64[d, 2]).  ``transform`` is
    None, one entry for every parameter, or a list of d entries; an entry is None, "log" or ("logit", lo, hi) with lo < hi finite"""
    if transform is None:
        return None
    single = isinstance(transform, str) or (isinstance(transform, tuple) and len(transform) == 3 and transform[0] == "logit")
    entries = [transform] * d if single else transform
    if not isinstance(entries, (list, tuple)):
        raise ValueError(f'adjust: transform: unknown transform {transform!r} (None, "log" or ("logit", lo, hi))')
    if len(entries) != d:
        raise ValueError(f"adjust: transform must be one entry or a list of {d} entries, one per parameter")
    got = [_transform_entry(e) for e in entries]
    kind = np.array([g[0] for g in got], dtype=np.int32)
    if not kind.any():
        return None
    return kind, np.array([[g[1], g[2]] for g in got], dtype=np.float64).reshape(d, 2)


def _fma(a: float, b: float, c: float) -> float:
    """abz_fma of finite doubles: a b + c rounded once (exact rationals; the conversion of a Fraction to float rounds to nearest even)"""
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        return a * b + c                                # exact, and it carries the sign IEEE gives the zero
    return float(r)


def _d2u(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _u2d(u: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", u & 0xFFFFFFFFFFFFFFFF))[0]


_NAN = _u2d(0x7FF8000000000000)                          # ABZ_NAN


def abz_log(x: float) -> float:
    """abz_log of include/abcdez_spec.h, literally (abz_log_core inlined)"""
    ux = _d2u(x)
    k = 0
    if (ux << 1) & 0xFFFFFFFFFFFFFFFF == 0:
        return -math.inf
    if ux >> 63:
        return _NAN
    if (ux >> 52) == 0x7FF:
        return x
    if (ux >> 52) == 0:
        x = x * 2.0 ** 54
        ux = _d2u(x)
        k = -54
    hx = ux >> 32
    hx = (hx + (0x3FF00000 - 0x3FE6A09E)) & 0xFFFFFFFF
    k += (hx >> 20) - 0x3FF
    hx = (hx & 0x000FFFFF) + 0x3FE6A09E
    m = _u2d((hx << 32) | (ux & 0xFFFFFFFF))
    f = m - 1.0
    s = f / (2.0 + f)
    z = s * s
    R = 1.479819860511658591e-01
    for c in (1.531383769920937332e-01, 1.818357216161805012e-01, 2.222219843214978396e-01, 2.857142874366239149e-01,
              3.999999999940941908e-01, 6.666666666666735130e-01):
        R = _fma(R, z, c)
    R = R * z
    hfsq = 0.5 * f * f
    dk = float(k)
    ln2_hi, ln2_lo = 6.93147180369123816490e-01, 1.90821492927058770002e-10
    return dk * ln2_hi - ((hfsq - _fma(s, hfsq + R, dk * ln2_lo)) - f)


def abz_exp(x: float) -> float:
    """abz_exp of include/abcdez_spec.h, literally"""
    if x != x:
        return x
    if x > 709.782712893383973096:
        return math.inf
    if x < -745.13321910194110842:
        return 0.0
    invln2 = 1.44269504088896338700e+00
    ln2_hi, ln2_lo = 6.93147180369123816490e-01, 1.90821492927058770002e-10
    t = x * invln2
    k = int(t + (-0.5 if x < 0.0 else 0.5))             # the C cast truncates toward zero, as int() does
    dk = float(k)
    hi = _fma(-dk, ln2_hi, x)
    lo = dk * ln2_lo
    r = hi - lo
    rr = r * r
    P = 4.13813679705723846039e-08
    for c in (-1.65339022054652515390e-06, 6.61375632143793436117e-05, -2.77777777770155933842e-03, 1.66666666666666019037e-01):
        P = _fma(P, rr, c)
    c = _fma(-P, rr, r)
    y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi)
    if k > 1000:
        y = y * 2.0 ** 1000
        k -= 1000
    elif k < -1000:
        y = y * 2.0 ** -1000
        k += 1000
    return y * _u2d((k + 1023) << 52)


def _elementwise(f):
    def g(a):
        a = np.asarray(a, dtype=np.float64)
        flat = a.reshape(-1)
        return np.array([f(float(v)) for v in flat], dtype=np.float64).reshape(a.shape)
    return g


ADJUST_MATH = (_elementwise(abz_log), _elementwise(abz_exp))      # the default ``math`` pair: the spec's own log and exp


def adjust_forward(X, tf, math=ADJUST_MATH):
    """abz_adjust_forward of every value: U (n x d) from the push_p-cast rows X of the positions that count"""
    if tf is None:
        return X
    kind, lo_hi = tf
    log = math[0]
    U = np.array(X, dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(U.shape[1]):
            if kind[k] == TF_LOG:
                U[:, k] = log(X[:, k])
            elif kind[k] == TF_LOGIT:
                U[:, k] = log((X[:, k] - lo_hi[k, 0]) / (lo_hi[k, 1] - X[:, k]))
    return U


def adjust_back(V, tf, math=ADJUST_MATH):
    """abz_adjust_back of every value"""
    if tf is None:
        return V
    kind, lo_hi = tf
    exp = math[1]
    Y = np.array(V, dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(Y.shape[1]):
            if kind[k] == TF_LOG:
                Y[:, k] = exp(V[:, k])
            elif kind[k] == TF_LOGIT:
                Y[:, k] = lo_hi[k, 0] + (lo_hi[k, 1] - lo_hi[k, 0]) / (1.0 + exp(-V[:, k]))
    return Y


def adjust_check_transformed(u_mean, tf):
    """a counting row outside the domain of its transform makes the mean of its column non-finite: refused before the cross pass"""
    if tf is None:
        return
    for k in np.flatnonzero(~np.isfinite(u_mean)):
        if tf[0][k] != TF_NONE:
            raise ValueError(f"adjust: transform: parameter {int(k)} has a value outside the domain of its {_TF_NAMES[int(tf[0][k])]} "
                             "transform among the particles that count (log needs x > 0, logit lo < x < hi)")


def adjust_check_logres(z_mean):
    for k in np.flatnonzero(~np.isfinite(z_mean)):
        raise ValueError(f"adjust: hcorr: a residual of parameter {int(k)} is exactly zero or not finite (its log is not finite)")


def adjust_centre(x_mean, beta, s_mean, target):
    """m_k = xmean_k - sum_j beta_jk (smean_j - t_j), j ascending from +0.0: the fitted value at the target"""
    acc = np.zeros(beta.shape[1])
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(beta.shape[0]):
            acc = acc + beta[j] * (s_mean[j] - target[j])
        return np.asarray(x_mean, dtype=np.float64) - acc


def adjust_residual(U, B, live, s_mean, x_mean, beta):
    """E (N x d): e_i = (u_i - xmean) - sum_j beta[j] (B[i, j] - smean[j]), j ascending from +0.0, for the rows with ``live``; +0.0
    for the others, whose inputs are never read"""
    Ul = np.where(live[:, None], U, 0.0)
    Bl = np.where(live[:, None], B, 0.0)
    acc = np.zeros_like(Ul)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(B.shape[1]):
            acc = acc + beta[j][None, :] * (Bl[:, j] - s_mean[j])[:, None]
        return np.where(live[:, None], (Ul - x_mean) - acc, 0.0)


def adjust_scaled(E, B, live, target, gamma, m, math=ADJUST_MATH):
    """V (N x d): v_i = m + e_i exp(-0.5 sum_j gamma[j] (B[i, j] - target[j])) for the rows with ``live``, +0.0 for the others"""
    Bl = np.where(live[:, None], B, 0.0)
    acc = np.zeros_like(E)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(B.shape[1]):
            acc = acc + gamma[j][None, :] * (Bl[:, j] - target[j])[:, None]
        V = np.zeros_like(E)
        V[live] = m + E[live] * math[1](-0.5 * acc[live])
    return V


def make_adjusted(rec, beta, columns, target, ridge, s_mean, x_mean, S_sx, P=None, hcorr=False, transform=None, gamma=None, z_mean=None,
                  S_sz=None):
    """the record ``posterior_adjusted`` returns: the fields of :func:`make_summary` for the adjusted parameters (``rec``) and
    ``beta`` (c x d), ``columns``, ``target``, ``ridge``, ``s_mean`` (c), ``x_mean`` (d: the unadjusted weighted mean), ``S_sx``
    (c x d), ``P`` (N x d adjusted rows, +0.0 for particles without weight; None unless asked for); ``hcorr`` and, when it is on,
    ``gamma`` (c x d: the slopes of the log squared residuals), ``z_mean`` (d) and ``S_sz`` (c x d), None otherwise; ``transform``:
    None, or the tuple of the d entries (None, "log" or ("logit", lo, hi)).  With a transform ``beta``, ``x_mean``, ``S_sx`` (and
    ``gamma``, ``z_mean``, ``S_sz``) are on the TRANSFORMED scale; ``mean``, ``cov``, the quantiles, ``hist`` and ``P`` are on the
    parameters' own."""
    c = len(columns)
    out = SimpleNamespace(**vars(rec))
    out.beta = np.asarray(beta, dtype=np.float64).reshape(c, -1)
    out.columns = tuple(int(k) for k in columns)
    out.target = np.asarray(target, dtype=np.float64).reshape(c)
    out.ridge = float(ridge)
    out.s_mean = np.asarray(s_mean, dtype=np.float64).reshape(c)
    out.x_mean = np.asarray(x_mean, dtype=np.float64).reshape(-1)
    out.S_sx = np.asarray(S_sx, dtype=np.float64).reshape(c, -1)
    out.P = P
    out.hcorr = bool(hcorr)
    out.transform = None if transform is None else tuple(
        None if kd == TF_NONE else "log" if kd == TF_LOG else ("logit", float(lh[0]), float(lh[1])) for kd, lh in zip(*transform))
    out.gamma = None if gamma is None else np.asarray(gamma, dtype=np.float64).reshape(c, -1)
    out.z_mean = None if z_mean is None else np.asarray(z_mean, dtype=np.float64).reshape(-1)
    out.S_sz = None if S_sz is None else np.asarray(S_sz, dtype=np.float64).reshape(c, -1)
    return out


def adjust_reference(P, blobs, Wns=None, target=None, columns=None, ridge=0.0, cov=True, corrected=True, wquantiles=(), hist=None,
                     rows=False, data=None, hcorr=False, transform=None, math=None):
    """numpy restatement of the regression-adjusted posterior (include/abcdez_spec.h, "REGRESSION ADJUSTMENT"), literally: ``P``
    the push_p-cast population (``r.P``), ``blobs`` the simulated data behind it (``r.blobs``), ``Wns`` the weights (None: unit
    weights, abcdemc), ``target`` one number per chosen column (None: ``data``, the simulator's ``data()``, when it has one number
    per blob column).  Moments by :func:`summary_reference`, the cross moments by :func:`tile_tree_sum`, the solve by
    :func:`adjust_solve`, and the summaries of the adjusted rows by :func:`summary_reference` again.  Rows of particles without
    weight may hold anything.  ``hcorr`` and ``transform`` (the options of :func:`adjust_hcorr` / :func:`adjust_transform`) restate
    the spec's HETEROSCEDASTIC CORRECTION and TRANSFORM; ``math`` is the pair (log, exp) over float64 arrays they use, by default the
    literal :func:`abz_log` / :func:`abz_exp` (bit for bit the device's; slow -- a test passes the oracle's, a law test numpy's).
    With both options off nothing changes.  Returns the record of :func:`make_adjusted`."""
    if blobs is None:
        raise ValueError(ADJUST_NEEDS_BLOBS)
    X, B = _as_matrix(P), _as_matrix(blobs)
    if X.ndim != 2 or B.ndim != 2 or B.shape[0] != X.shape[0]:
        raise ValueError("adjust: P and blobs must hold one row per particle")
    N, d = X.shape
    nb = B.shape[1]
    cols = adjust_columns(columns, nb)
    t = adjust_target(target, cols, nb, data)
    ridge = adjust_ridge(ridge)
    hcorr = adjust_hcorr(hcorr)
    tf = adjust_transform(transform, d)
    math = ADJUST_MATH if math is None else math
    w = np.ones(N) if Wns is None else np.asarray(Wns, dtype=np.float64)
    if w.shape != (N,):
        raise ValueError("summary: one weight per particle expected")
    live = w > 0.0
    wl = np.where(live, w, 0.0)
    if tf is not None:                                  # U: rows that do not count are +0.0 and never read
        U = np.zeros((N, d))
        U[live] = adjust_forward(X[live], tf, math)
        X = U
    mx = summary_reference(X, Wns, cov=False)
    ms = summary_reference(B, Wns, cov=True)
    Bc = B[:, cols]
    s_mean, x_mean = ms.mean[cols], mx.mean
    adjust_check_transformed(x_mean, tf)
    adjust_check_means(s_mean, x_mean)

    def cross(V, v_mean):
        with np.errstate(over="ignore", invalid="ignore"):
            Cs = np.where(live[:, None], Bc, 0.0) - s_mean
            Cv = np.where(live[:, None], V, 0.0) - v_mean
            out = np.empty((len(cols), d))
            for j in range(len(cols)):
                out[j] = tile_tree_sum(np.where(live[:, None], wl[:, None] * (Cs[:, j:j + 1] * Cv), 0.0))
        return out

    S_sx = cross(X, x_mean)
    S_ss = ms.S[np.ix_(cols, cols)]
    beta = adjust_solve(S_ss, S_sx, ridge, cols)
    gamma = z_mean = S_sz = None
    if hcorr:
        E = adjust_residual(X, Bc, live, s_mean, x_mean, beta)
        Z = np.zeros((N, d))
        with np.errstate(all="ignore"):
            Z[live] = math[0](E[live] * E[live])
        z_mean = summary_reference(Z, Wns, cov=False).mean
        adjust_check_logres(z_mean)
        S_sz = cross(Z, z_mean)
        gamma = adjust_solve(S_ss, S_sz, ridge, cols)
        V = adjust_scaled(E, Bc, live, t, gamma, adjust_centre(x_mean, beta, s_mean, t), math)
    else:
        V = adjust_apply(X, Bc, live, t, beta)
    Y = V
    if tf is not None:
        Y = np.zeros((N, d))
        Y[live] = adjust_back(V[live], tf, math)
    rec = summary_reference(Y, Wns, cov=cov, corrected=corrected, quantiles=(), wquantiles=wquantiles, hist=hist)
    return make_adjusted(rec, beta, cols, t, ridge, s_mean, x_mean, S_sx, Y if rows else None, hcorr, tf, gamma, z_mean, S_sz)


def engine_adjusted(eng, **opts):
    """``eng.posterior_adjusted(**opts)`` for a PopulationEngine; any other engine object: the restatement on its result"""
    def restated(res, **o):
        if res.get("blobs") is None:
            raise ValueError(ADJUST_NEEDS_BLOBS)
        return adjust_reference(res["P"], res["blobs"], res.get("Wns"), data=tuple(eng.spec.sim.data()), **o)
    return engine_call(eng, "posterior_adjusted", restated, **opts)
