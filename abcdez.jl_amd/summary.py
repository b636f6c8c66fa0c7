"""Posterior summaries: weighted mean, covariance, marginal quantiles, effective sample size.

What every test of the reference extracts from a result -- ``mean(r.P[r.Wns .> 0.0])`` (test/runtests.jl:159-162) of the
tuple of src/abcdez_smc.jl:388-393 / src/abcdez_mc.jl:166-171 -- and what an ABC user reports next to it.  The arithmetic
is fixed in include/abcdez_spec.h ("posterior summaries"): every sum is the tile tree over the population positions, no
fused multiply-add, exact order statistics.  The HIP library evaluates it on the device (csrc/abz_summary.hip);
:func:`summary_reference` is the numpy restatement of the same arithmetic, bit for bit -- the yardstick of the tests, and
what an engine without the device call (the CPU test engine) computes from its downloaded population.
"""
from __future__ import annotations

import math
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


def make_summary(mean, S, W, Q, n_pos, quantiles, probs, corrected=True, wquantiles=None, wprobs=(), M=None, n_mass=None):
    """the record ``posterior_summary`` returns, from what the library (or the restatement below) computes"""
    W, Q = float(W), float(Q)
    cov = None if S is None else np.asarray(S, dtype=np.float64) / cov_denominator(W, Q, corrected)
    if wquantiles is None:
        wquantiles = np.empty((0, np.asarray(mean).shape[0]))
    return SimpleNamespace(mean=np.asarray(mean, dtype=np.float64), cov=cov, S=S, W=W, Q=Q, ess=W * W / Q, n_pos=int(n_pos),
                           quantiles=quantiles, probs=tuple(probs), corrected=bool(corrected), wquantiles=wquantiles,
                           wprobs=tuple(wprobs), M=None if M is None else int(M), n_mass=None if n_mass is None else int(n_mass))


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
    import bisect
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
    masses = [1 << stratum_bits(N)] * N if w is None else weight_fix(w, N)
    idx = [i for i in range(N) if masses[i] >= 1]
    if not idx:
        raise ValueError("summary: no particle has a positive weight that carries mass")
    M = sum(masses)
    if M >= 1 << 63:
        raise ValueError("summary: the total mass reaches 2^63 -- the weights are not normalised")
    ml = [masses[i] for i in idx]
    out = np.empty((len(probs), d))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(d):
            out[:, k] = wquantile_column(X[idx, k], ml, probs)
    return out, M, len(idx)


def summary_reference(P, Wns=None, cov=True, corrected=True, quantiles=(), wquantiles=()):
    """numpy restatement of the summary arithmetic.  ``P``: the push_p-cast population, shape (N,) or (N, d) (``r.P``);
    ``Wns``: the weights (``r.Wns``), or None for unit weights (abcdemc).  Returns the record of :func:`make_summary`:
    ``mean`` (d), ``cov`` (d x d, or None), ``S`` (the unnormalised second central moments), ``quantiles``
    (len(quantiles) x d), ``W``, ``Q``, ``ess = W^2 / Q``, ``n_pos``, and for ``wquantiles`` the weighted quantiles ``wquantiles``
    (len(wquantiles) x d) with the total integer mass ``M`` and ``n_mass`` (both None when none are asked for)."""
    X = np.asarray(P, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
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
    return make_summary(mean, S, W, Q, n_pos, qs, probs, corrected, wq, wprobs, M, n_mass)


def summary_options(summary) -> dict:
    """the ``summary=`` keyword of the drivers: True, or a dict of cov / corrected / quantiles / wquantiles"""
    if summary is True:
        return {}
    if isinstance(summary, dict):
        bad = set(summary) - {"cov", "corrected", "quantiles", "wquantiles"}
        if bad:
            raise ValueError(f"summary: unknown option(s) {sorted(bad)} (cov, corrected, quantiles, wquantiles)")
        return dict(summary)
    raise ValueError("summary must be None, True or a dict of the options cov, corrected, quantiles, wquantiles")


def engine_summary(eng, **opts):
    """``eng.posterior_summary(**opts)`` for a PopulationEngine; any other engine object: the restatement on its result"""
    if hasattr(eng, "posterior_summary"):
        return eng.posterior_summary(**opts)
    res = eng.result()
    return summary_reference(res["P"], res.get("Wns"), **opts)
