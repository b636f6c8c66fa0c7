"""The posterior sample on the device (csrc/abz_sample.hip) against abcdez_amd.summary.sample_reference: ``index``, ``M`` and
``n_mass`` BIT FOR BIT, ``P`` and ``C`` against the downloaded result indexed by it -- after short real runs of all four ABC
kernels, on crafted populations handed to the C entry point as plain device pointers (the technique of
tests/test_gpu_posterior_summary_edges.py: both row slots in use, the slot that is not current and every dead row poisoned), for
abcdemc's classic storage without weights (the closed form), with blobs, in a continued run, and through raw ctypes."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import abcdez_amd as A
from abcdez_amd import _lib
from abcdez_amd.engine import HipOps, PopulationEngine
from abcdez_amd.summary import sample_reference, stratum_bits, weight_fix
from test_gpu_posterior_summary import bits, model
from test_gpu_posterior_summary_edges import synthetic
from test_gpu_shim_sequence import ShimEngine

pytestmark = pytest.mark.gpu

ABCKS = {"indicator_strict": A.IndicatorStrict0toeps, "indicator": A.Indicator0toeps, "epa_strict": A.EpaStrict0toeps,
         "epa": A.Epa0toeps}


def ns_of(N):
    return (1, 7, N, 3 * N + 1)


def rounds_of(ops):
    return ops.stream_version()[1]


def assert_sample_of_result(s, res_P, res_C, Wns, seed, rounds, what):
    index, M, n_mass = sample_reference(len(res_C), Wns, s.n, seed, s.draw, rounds=rounds)
    assert (s.M, s.n_mass) == (M, n_mass), what
    assert s.index.dtype == np.int64 and np.array_equal(s.index, index), what
    assert np.array_equal(bits(s.P), bits(res_P[index])), what
    assert np.array_equal(bits(s.C), bits(res_C[index])), what


# ------------------------------------------------------------------------------------------ real runs, all four kernels
@pytest.mark.parametrize("d", [1, 5, 33])
@pytest.mark.parametrize("abck", list(ABCKS))
def test_sample_of_a_real_run_is_the_reference(abck, d):
    """d = 1: rows of one double, P a vector; d = 5: rows padded to 8; d = 33: rows of 64 doubles, two loads per lane"""
    prior, sim = model(d)
    N = 4096
    # four generations that resample once and end on a prologue: dead positions, and unequal weights for the Epanechnikov kernels
    r = A.abcdesmc(prior, sim, 0.0, None, nparticles=N, α=0.6, δess=0.25, ABCk=ABCKS[abck], verbose=False, rng=5, max_iters=4)
    assert r.iters == 4 and r.P.shape == ((N,) if d == 1 else (N, d))
    print(abck, d, "dead", int((r.Wns == 0).sum()), "distinct positive weights", np.unique(r.Wns[r.Wns > 0]).size)
    for k, n in enumerate(ns_of(N)):
        s = r.engine.posterior_sample(n, draw=k)
        assert s.P.shape == ((n,) if d == 1 else (n, d)) and s.C.shape == (n,) and s.blobs is None and (s.n, s.draw) == (n, k)
        assert_sample_of_result(s, r.P, r.C, r.Wns, 5, rounds_of(r.engine.ops), (abck, d, n))
        assert np.all(r.Wns[s.index] > 0)


# ------------------------------------------------------------------------------------------ crafted populations
def crafted_spec(d):
    if d == 1:
        prior = A.Normal(0.0, math.sqrt(10.0))
        sim = A.Normal1D(0.4)
    else:   # a discrete column among the continuous ones: push_p is rint there and the identity elsewhere
        prior = A.Factored(*[A.DiscreteUniform(-50, 50) if k == 1 else A.Normal(0.0, 1.0) for k in range(d)])
        sim = A.MVNormal(tuple([0.25] * d))
    return A.ModelSpec(prior, sim, A.Epa0toeps, seed=77)


@pytest.fixture(scope="module")
def ops_of():
    made = {}

    def get(d):
        if d not in made:
            spec = crafted_spec(d)
            made[d] = (spec, HipOps(spec))
        return made[d]
    yield get
    made.clear()


def crafted_weights(N, pattern, rng):
    w = rng.random(N) + 0.05
    w[rng.random(N) < 0.3] = 0.0
    if pattern == "zero_run":              # a run of weightless positions across the first tile boundary (or up to the end)
        w[min(2040, N // 2):min(2060, N)] = 0.0
        w[0] = 0.0
    elif pattern == "heavy":               # one position holds almost all the mass
        w *= 1e-9
        w[(2 * N) // 3] = 1.0
    w[N // 2 if pattern != "zero_run" else N // 4] += 0.5      # never all dead
    return w / w.sum()


@pytest.mark.parametrize("pattern", ["plain", "zero_run", "heavy"])
@pytest.mark.parametrize("N", [1, 2047, 2049, 5000])
@pytest.mark.parametrize("d", [1, 3, 33])
def test_crafted_populations_through_the_c_entry(ops_of, d, N, pattern):
    """N = 1, 2047: one tile; 2049: a tile boundary and a last tile of one position; 5000: three tiles, the last ragged"""
    spec, ops = ops_of(d)
    rng = np.random.default_rng(1000 * d + N + len(pattern))
    w = crafted_weights(N, pattern, rng)
    values = rng.standard_normal((N, d)) * 7.3
    syn = synthetic(spec, N, rng, w > 0, values=values, weights=w, ops=ops)
    dist = rng.random(N)
    stamps = rng.integers(0, 1 << 62, N, dtype=np.int64)
    d_dist, d_stamp = torch.from_numpy(dist).to(ops.device), torch.from_numpy(stamps).to(ops.device)
    m = weight_fix(w, N)
    for k, n in enumerate(ns_of(N)):
        idx, P, th, dl, st, M, n_mass = ops.posterior_sample(syn.bits, syn.slot0, syn.slot1, syn.wns, N, n, draw=k, delta=d_dist,
                                                              stamp=d_stamp, want_theta=True)
        index, M_ref, n_mass_ref = sample_reference(N, w, n, spec.seed, k, rounds=rounds_of(ops))
        what = (d, N, pattern, n)
        assert (M, n_mass) == (M_ref, n_mass_ref) == (sum(m), sum(1 for x in m if x >= 1)), what
        got = idx.cpu().numpy().astype(np.int64)
        assert np.array_equal(got, index), what
        assert np.array_equal(bits(P.cpu().numpy()), bits(syn.P[index])), what                  # push_p-cast, dense n x d
        rows = th.cpu().numpy()
        assert rows.shape == (n, spec.ld) and np.array_equal(bits(rows[:, :d]), bits(syn.rows[index])) and (rows[:, d:] == 0).all(), what
        assert np.array_equal(dl.cpu().numpy(), dist[index]) and np.array_equal(st.cpu().numpy(), stamps[index]), what
    # without the optional outputs, and the same weights on classic storage (bits NULL: slot0 is the row array)
    cur = torch.from_numpy(np.pad(np.where((w > 0)[:, None], syn.rows, np.nan), ((0, 0), (0, spec.ld - d)))).to(ops.device)
    idx, P, th, dl, st, M, n_mass = ops.posterior_sample(None, cur, None, syn.wns, N, 7, draw=1)
    index = sample_reference(N, w, 7, spec.seed, 1, rounds=rounds_of(ops))[0]
    assert th is None and dl is None and st is None and np.array_equal(idx.cpu().numpy(), index)
    assert np.array_equal(bits(P.cpu().numpy()), bits(syn.P[index]))


def test_refusals_leave_the_outputs_alone(ops_of):
    spec, ops = ops_of(3)
    N = 100
    rng = np.random.default_rng(3)
    rows = torch.from_numpy(np.pad(rng.standard_normal((N, 3)), ((0, 0), (0, 1)))).to(ops.device)
    lib, ctx = ops.lib, ops.ctx
    sentinel = 0x5A5A5A5A
    M, n_mass = C.c_uint64(), C.c_int64()

    def call(wns, n, N_=N):
        rows_out = min(max(int(n), 1), 16)                                   # (the refused n are never written)
        idx = torch.full((rows_out,), sentinel, dtype=torch.int32, device=ops.device)
        P = torch.full((rows_out, 3), -7.0, dtype=torch.float64, device=ops.device)
        w = None if wns is None else torch.from_numpy(np.ascontiguousarray(wns, dtype=np.float64)).to(ops.device)
        rc = lib.abcdez_posterior_sample(ctx, None, N_, rows.data_ptr(), None, None if w is None else w.data_ptr(), n, 0, None, None,
                                         idx.data_ptr(), P.data_ptr(), None, None, None, C.byref(M), C.byref(n_mass))
        torch.cuda.synchronize()
        return rc, lib.abcdez_last_error().decode(), idx.cpu().numpy(), P.cpu().numpy()

    rc, msg, idx, P = call(np.zeros(N), 5)
    assert rc != 0 and "carries mass" in msg and (idx == sentinel).all() and (P == -7.0).all()
    rc, msg, idx, P = call(np.full(N, 1e6), 5)
    assert rc != 0 and "2^63" in msg and (idx == sentinel).all() and (P == -7.0).all()
    tiny = np.zeros(N)
    tiny[3] = 3.0 / (N * 2.0 ** 40)                                          # M = 3
    rc, msg, idx, P = call(tiny, 5)
    assert rc != 0 and "exceeds" in msg and (idx == sentinel).all() and (P == -7.0).all()
    rc, msg, idx, P = call(tiny, 3)
    assert rc == 0 and idx.tolist() == [3, 3, 3] and (M.value, n_mass.value) == (3, 1)
    for bad_n in (0, -1, 1 << 31):
        rc, msg, idx, P = call(np.full(N, 1.0 / N), bad_n)
        assert rc != 0 and "n must be" in msg and (idx == sentinel).all()
    dl = torch.zeros(5, dtype=torch.float64, device=ops.device)
    idx = torch.zeros(5, dtype=torch.int32, device=ops.device)
    P = torch.zeros((5, 3), dtype=torch.float64, device=ops.device)
    rc = lib.abcdez_posterior_sample(ctx, None, N, rows.data_ptr(), None, None, 5, 0, None, None, idx.data_ptr(), P.data_ptr(), None,
                                     dl.data_ptr(), None, C.byref(M), C.byref(n_mass))
    assert rc != 0 and "delta_out" in lib.abcdez_last_error().decode()
    with pytest.raises(_lib.AbcdezError, match="packed storage"):
        ops.posterior_sample(idx, rows, None, None, N, 5)


# ------------------------------------------------------------------------------------------ abcdemc: classic storage, no weights
def test_abcdemc_takes_the_closed_form():
    prior, sim = model(5)
    N = 500
    r = A.abcdemc(prior, sim, 1.0, None, nparticles=N, generations=6, verbose=False, rng=8, sample=dict(n=1234, draw=4))
    s = r.sample
    b = stratum_bits(N)
    index, M, n_mass = sample_reference(N, None, 1234, 8, 4, rounds=rounds_of(r.engine.ops))
    assert (s.M, s.n_mass) == (N << b, N) == (M, n_mass)
    assert np.array_equal(s.index, index) and np.array_equal(bits(s.P), bits(r.P[index])) and np.array_equal(bits(s.C), bits(r.C[index]))
    assert np.array_equal(r.engine.posterior_sample(N).index, np.arange(N))                     # n = N: the identity
    assert np.array_equal(r.engine.posterior_sample(4 * N, draw=2).index, np.repeat(np.arange(N), 4))


# ------------------------------------------------------------------------------------------ blobs
BLOB_CASES = {
    "socks": (A.Factored(A.NegativeBinomial(900 / 195, (900 / 195) / (30 + 900 / 195)), A.Beta(15, 2)), A.Socks(0, 11, blobs=True), 0.01,
              1500, A.IndicatorStrict0toeps),
    "mvn3": (A.Factored(*[A.Normal(0.0, 1.0)] * 3), A.MVNormal((1.0, 0.5, 0.2), blobs=True), 1.0, 1000, A.Epa0toeps),
}


@pytest.mark.parametrize("name", list(BLOB_CASES))
def test_sampled_blobs_are_the_results_blobs(name):
    prior, sim, eps, N, abck = BLOB_CASES[name]
    r = A.abcdesmc(prior, sim, eps, None, nparticles=N, ABCk=abck, verbose=False, rng=31, sample=dict(n=333, draw=1, blobs=True))
    s = r.sample
    assert r.blobs.ndim == 2 and r.blobs.shape[1] > 1 and s.blobs.shape == (333, r.blobs.shape[1])
    assert_sample_of_result(s, r.P, r.C, r.Wns, 31, rounds_of(r.engine.ops), name)
    assert np.array_equal(bits(s.blobs), bits(r.blobs[s.index]))
    assert r.engine.posterior_sample(10, blobs=False).blobs is None
    d = r.engine.posterior_sample(3 * N + 1)                                  # blobs default on when the engine carries stamps
    assert np.array_equal(bits(d.blobs), bits(r.blobs[d.index]))


def test_download_false_with_a_sample_only():
    prior, sim = model(5)
    kw = dict(nparticles=2049, α=0.6, δess=0.33, ABCk=A.Epa0toeps, verbose=False, rng=5, max_iters=3)
    r = A.abcdesmc(prior, sim, 0.0, None, download=False, sample=100, **kw)
    full = A.abcdesmc(prior, sim, 0.0, None, **kw)
    assert r.P is None and r.Wns is None and r.C is None
    assert_sample_of_result(r.sample, full.P, full.C, full.Wns, 5, rounds_of(r.engine.ops), "download=False")
    with pytest.raises(ValueError, match="blobs=True needs"):
        r.engine.posterior_sample(5, blobs=True)


# ------------------------------------------------------------------------------------------ a continued run
def test_a_run_continued_after_a_sample_is_bit_identical():
    """two engines on the same key, the next generation's select enqueued ahead behind every group of sweeps; one is asked for a
    sample between the generations (the five generations include resamplings)"""
    prior, sim = model(3)
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
                assert e.posterior_sample(777, draw=gen).n_mass >= 1
        e.discard_select_ahead()
    assert out[0] == out[1]
    assert engs[0].draw == engs[1].draw >= 1, "the run was meant to resample"
    a, b = engs[0].result(), engs[1].result()
    for f in ("P", "theta", "logpi", "C", "Wns", "alive"):
        assert np.array_equal(a[f], b[f]), f
    assert engs[0].ops.smc_select_stats() == engs[1].ops.smc_select_stats()      # the selects enqueued ahead were all still used
    assert_sample_of_result(engs[0].posterior_sample(2 * N), b["P"], b["C"], b["Wns"], 9, rounds_of(engs[0].ops), "continued")


# ------------------------------------------------------------------------------------------ raw ctypes, as the Julia shim calls it
def test_raw_ctypes_call_in_the_manner_of_the_shim():
    """posterior_sample(e; n, draw) of julia/ABCdeZHIP.jl transliterated: device memory from abcdez_dev_alloc, the outputs read with
    abcdez_memcpy_d2h, no torch and no engine.py"""
    prior = A.Factored(A.Normal(1, 0.5), A.DiscreteUniform(1, 10))
    N, n, draw = 400, 150, 6
    e = ShimEngine(prior, A.NormalTimesDU(5.5), A.Epa0toeps, 31, N)
    e.init()
    e.reset_weights()
    e.prologue(0.6, math.inf, 0.0, math.inf, 0.5 * N)                         # unequal weights, dead particles
    idx, P, dl = e.devalloc(4 * n), e.devalloc(8 * n * e.d), e.devalloc(8 * n)
    M, n_mass = C.c_uint64(), C.c_int64()
    e.ck(e.lib.abcdez_posterior_sample(e.ctx, e.bits[e.bc], N, e.slot[0], e.slot[1], e.wns, n, draw, e.delta[e.cur], None, idx, P, None,
                                       dl, None, C.byref(M), C.byref(n_mass)))
    h_idx, h_P, h_dl = np.empty(n, dtype=np.uint32), np.empty((n, e.d)), np.empty(n)
    for h, dptr in ((h_idx, idx), (h_P, P), (h_dl, dl)):
        e.ck(e.lib.abcdez_memcpy_d2h(e.ctx, h.ctypes.data, dptr, h.nbytes))
    full_P, Wns, full_C, _ = e.download(packed=True)
    index, M_ref, n_mass_ref = sample_reference(N, Wns, n, 31, draw, rounds=e.lib.abcdez_rng_rounds())
    assert (M.value, n_mass.value) == (M_ref, n_mass_ref) and 0 < n_mass_ref < N
    assert np.array_equal(h_idx.astype(np.int64), index)
    assert np.array_equal(bits(h_P), bits(full_P[index])) and np.array_equal(bits(h_dl), bits(full_C[index]))
    assert (h_P[:, 1] == np.rint(h_P[:, 1])).all()                            # the discrete column is cast
    for p in (idx, P, dl):
        e.lib.abcdez_dev_free(p)
    e.close()
