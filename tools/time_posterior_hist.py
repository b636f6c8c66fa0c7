#!/usr/bin/env python3
"""Marginal and pairwise histograms on the device against the route without them, same process, one GPU: an smc32-shaped
population (d = 32 MVN, 2^22 particles) at the end of a run with an indicator kernel and of one with an Epanechnikov kernel.
  (a)  engine.posterior_summary(cov=False, hist=dict(bins=64))                              32 marginals
  (b)  ... hist=dict(bins=64, pairs="all", bins2=32) and bins2=64                           plus all 496 pairs
  (m)  engine.posterior_summary(cov=False)                                                  the first-moment pass, for scale
  (d)  engine.result()                                                                      the download the other route starts with
  (h)  numpy binning of the downloaded P, Wns on one host thread (indices by the same floor rule, np.bincount with the weights;
       a floating-point sum, which is what a user would write): the 32 marginals, and the 496 pairs at bins2 = 32 and 64, for both runs
The runs are stopped after a few generations: the cost depends on N, d and the share of counting positions, not on how far the run
got.  One warm-up and `REPS` alternating repetitions of the device calls, HIP events around each call (every call ends in its own
read-back and synchronisation), medians and spread; the download is timed with the wall clock, `REPS` times; the host binning
once per run and size (seconds each).  Bytes by the model of DESIGN.md 4.6 "Histograms" and the rate they imply are reported next to the
times.  Writes profiles/r08_posterior_hist.json (or the path given as the first argument)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import abcdez_amd as A

REPS = 7
d = 32
N = int(os.environ.get("ABCDEZ_TIME_N", 1 << 22))
GENS = 6
BINS = 64
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r08_posterior_hist.json")
assert torch.cuda.is_available(), "this measurement needs the GPU"
prior = A.Factored(*[A.Normal(0.0, 1.0) for _ in range(d)])
sim = A.MVNormal(tuple([1.0] * d))
CASES = {"marginals": dict(bins=BINS), "pairs32": dict(bins=BINS, pairs="all", bins2=32), "pairs64": dict(bins=BINS, pairs="all", bins2=64)}


def run(abck):
    return A.abcdesmc(prior, sim, 0.0, None, nparticles=N, ABCk=abck, verbose=False, rng=1, nsims_max=10 ** 12, max_iters=GENS,
                      summary=True, download=False)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    got = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), got


def alternate(fns, reps=REPS):
    """{name: (median ms, all ms, last result)}; one warm-up each, then the candidates in turn, `reps` times"""
    for fn in fns.values():
        fn()
    ms = {k: [] for k in fns}
    got = {}
    for _ in range(reps):
        for k, fn in fns.items():
            t, got[k] = event_ms(fn)
            ms[k].append(t)
    return {k: (statistics.median(v), v, got[k]) for k, v in ms.items()}


def bytes_model(n, n_mass, nc, bins, npairs, bins2, automatic=True):
    """the passes' own traffic (csrc/abz_hist.hip): rows and weights in, masses and bin indices out and in again"""
    ld = 32
    b = 0
    if automatic:
        b += -(-nc // 8) * n * 8 + n_mass * ld * 8                      # range: the weights per launch, every row once
    b += n * 8 + n_mass * ld * 8 + n * 8 + n_mass * nc * (2 + (1 if npairs else 0))     # bin: weights, rows in; masses, indices out
    groups = -(-nc // min(nc, 5120 // (bins + 3)))
    b += groups * n * 8 + n * nc * 2                                   # 1-D: masses per column group, u16 indices once
    if npairs:
        per = bins2 * bins2
        B = min(16, 8192 // per) if per <= 8192 else 1
        seg = 1 if per <= 8192 else -(-bins2 // (8192 // bins2))
        batches = sum(-(-(nc - 1 - j) // B) for j in range(nc - 1)) * seg
        b += batches * n * 9 + npairs * n                              # pairs: masses and column j per batch, column k per pair
    return b


def host_binning(P, w, h, bins2):
    """(seconds for the 32 marginals, seconds for the pairs, worst |host - device| / M over the marginals)"""
    t0 = time.perf_counter()
    worst = 0.0
    for c in range(d):
        x = P[:, c]
        b = np.clip(np.floor((x - h.lo[c]) * (BINS / (h.hi[c] - h.lo[c]))), 0, BINS - 1).astype(np.int64)
        got = np.bincount(b, weights=w, minlength=BINS)
        worst = max(worst, float(np.abs(got / got.sum() - h.mass1[c] / h.M).max()))
    t1 = time.perf_counter()
    idx = [np.clip(np.floor((P[:, c] - h.lo[c]) * (bins2 / (h.hi[c] - h.lo[c]))), 0, bins2 - 1).astype(np.int64) for c in range(d)]
    t2 = time.perf_counter()
    done = 0
    for j in range(d):
        for k in range(j + 1, d):
            np.bincount(idx[j] * bins2 + idx[k], weights=w, minlength=bins2 * bins2)
            done += 1
        print("host pairs", done, flush=True)
    t3 = time.perf_counter()
    return t1 - t0, (t2 - t1) + (t3 - t2), worst


rec = {"config": {"d": d, "N": N, "bins": BINS, "reps": REPS, "pairs": d * (d - 1) // 2}}
for label, abck in (("indicator", A.IndicatorStrict0toϵ), ("epanechnikov", A.Epa0toϵ)):
    r = run(abck)
    eng = r.engine
    eng._stream()
    fns = {k: (lambda o=o: eng.posterior_summary(cov=False, hist=o)) for k, o in CASES.items()}
    fns["moments_only"] = lambda: eng.posterior_summary(cov=False)
    res = alternate(fns)
    print(label, {k: v[0] for k, v in res.items()}, flush=True)
    h = res["marginals"][2].hist
    out = {"generations": r.iters, "n_pos": res["marginals"][2].n_pos, "n_mass": h.n_mass, "M": h.M,
           "moments_only_ms": res["moments_only"][0], "moments_only_all_ms": res["moments_only"][1]}
    for k, o in CASES.items():
        ms = res[k][0] - res["moments_only"][0]
        npairs = len(res[k][2].hist.pairs)
        by = bytes_model(N, h.n_mass, d, BINS, npairs, o.get("bins2", 0))
        out[k] = {"ms": res[k][0], "all_ms": res[k][1], "spread": (max(res[k][1]) - min(res[k][1])) / res[k][0],
                  "minus_moments_ms": ms, "bytes_model": by, "model_TB_per_s": by / (ms * 1e-3) / 1e12,
                  "readback_bytes": 8 * (d * (BINS + 3) + npairs * o.get("bins2", 0) ** 2)}
    dl = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        got = eng.result()
        dl.append(time.perf_counter() - t)
    P, w = got["P"], got["Wns"]
    out["download_s"] = statistics.median(dl)
    out["download_all_s"] = dl
    out["download_bytes"] = int(sum(v.nbytes for v in got.values() if isinstance(v, np.ndarray)))
    live = w > 0
    Pl, wl = P[live], w[live]
    for bins2 in (32, 64):
        t1, t2, worst = host_binning(Pl, wl, h, bins2)
        out.setdefault("host_binning_marginals_s", t1)
        out["host_binning_496_pairs_bins2_%d_s" % bins2] = t2
        out["host_vs_device_worst_abs_diff_of_bin_shares"] = worst
    del Pl, wl
    rec[label] = out
    del r, eng, got, P, w
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec))
