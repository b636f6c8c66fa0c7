#!/usr/bin/env python3
"""The posterior predictive summary on the device against the route it replaces, same process, one GPU:
  lv      Lotka-Volterra RK4 (the `lv` configuration's model, tests/golden/lv_data.json), 2^20 particles, blobs on
  wiener  WienerRMS with 16 time points, 2^22 particles, blobs on
each stopped after a few generations (the cost depends on N, the blob width and the share of counting positions, not on how far
the run got).  Timed, one warm-up and `REPS` repetitions each, medians reported and every repetition listed:
  (p)  engine.posterior_predictive(wquantiles=(0.025, 0.5, 0.975)) as a whole (wall clock: it ends in its own read-backs), and its
       two parts on their own: the blob rebuild (packed gather of the rows, abcdez_blob_eval for all N particles, the bit-for-bit
       check of the re-run distances) and the summaries (abcdez_columns_moments + abcdez_columns_wquantiles on the rebuilt matrix)
  (o)  the route of old: engine.result() -- the same rebuild, then the pinned download of the population and the N x n_blob blobs --
       split into rebuild (the figure above: the code is the same) and download (result() minus that), plus on the host the numpy
       weighted mean and, per column, an argsort weighted quantile at the same three probabilities
Writes profiles/r10_posterior_predictive.json (or the path given as the first argument).  ABCDEZ_TIME_SCALE=k divides both N by 2^k
(a smaller box); ABCDEZ_TIME_REPS sets the repetitions (default 10)."""
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import abcdez_amd as A

REPS = int(os.environ.get("ABCDEZ_TIME_REPS", 10))
SHIFT = int(os.environ.get("ABCDEZ_TIME_SCALE", 0))
PROBS = (0.025, 0.5, 0.975)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r10_posterior_predictive.json")
assert torch.cuda.is_available(), "this measurement needs the GPU"


def lv_sim():
    with open(os.path.join(ROOT, "tests", "golden", "lv_data.json")) as f:
        g = json.load(f)
    return A.LotkaVolterraRK4(tuple(g["obs"]), x0=g["x0"], y0=g["y0"], dt=g["dt"], steps_per_obs=g["steps_per_obs"], noise=g["noise"],
                              blobs=True)


WIEN = tuple(math.sqrt(0.25 * t * t + 4.0 * t) for t in range(16))
CASES = {
    "lv": dict(prior=A.Factored(*[A.Uniform(0.0, 2.0)] * 4), sim=lv_sim(), eps=1.0, N=(1 << 20) >> SHIFT, abck=A.IndicatorStrict0toeps,
               gens=4),
    "wiener": dict(prior=A.Factored(A.Uniform(-2, 2), A.Uniform(0, 4)), sim=A.WienerRMS(WIEN, blobs=True), eps=0.0, N=(1 << 22) >> SHIFT,
                   abck=A.Epa0toeps, gens=4),
}


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    got = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, got


def med(v):
    return statistics.median(v)


def rebuild(eng):
    """the first half of posterior_predictive (and of result() with blobs), as the engine does it"""
    th, _, dl = eng.state
    X = torch.zeros((eng.N, eng.ops.blob_width()), dtype=torch.float64, device=eng.device)
    redo = torch.empty_like(dl)
    eng.ops.blob_eval(th, eng.stamp[eng.cur], X, redo)
    assert torch.equal(redo.view(torch.int64), dl.view(torch.int64))
    return X


def summaries(eng, X):
    nb = eng.spec.n_blob
    mean = eng.ops.columns_moments(X, eng.wns, m=nb, want_second=False)[0]
    q = eng.ops.columns_wquantiles(X, eng.wns, PROBS, m=nb)[0]
    return mean, q


def host_summaries(blobs, w):
    """what a user of the parent commit does with r.blobs and r.Wns: weighted mean, and per column a weighted quantile by argsort
    and the cumulated weights"""
    B = blobs.reshape(blobs.shape[0], -1)
    W = w.sum()
    mean = (w[:, None] * B).sum(0) / W
    q = np.empty((len(PROBS), B.shape[1]))
    for k in range(B.shape[1]):
        o = np.argsort(B[:, k], kind="stable")
        c = np.cumsum(w[o])
        q[:, k] = B[o[np.minimum(np.searchsorted(c, np.array(PROBS) * c[-1]), len(o) - 1)], k]
    return mean, q


rec = {"config": {"reps": REPS, "scale_shift": SHIFT, "probs": PROBS}}
for label, c in CASES.items():
    N = c["N"]
    r = A.abcdesmc(c["prior"], c["sim"], c["eps"], None, nparticles=N, ABCk=c["abck"], verbose=False, rng=1, nsims_max=10 ** 13,
                   max_iters=c["gens"], summary=dict(cov=False), download=False)
    eng = r.engine
    eng._stream()
    nb, width = eng.spec.n_blob, eng.ops.blob_width()
    out = {"N": N, "n_blob": nb, "blob_width": width, "generations": r.iters, "n_pos": r.summary.n_pos,
           "matrix_bytes": N * width * 8, "blob_download_bytes": N * nb * 8}
    t = {"predictive_ms": [], "rebuild_ms": [], "summaries_ms": [], "result_ms": [], "host_mean_ms": [], "host_quantiles_ms": []}
    for k in range(REPS + 1):                                                    # the first round warms up
        a, p = wall(lambda: eng.posterior_predictive(wquantiles=PROBS))
        b, X = wall(lambda: rebuild(eng))
        s, (mean, q) = wall(lambda: summaries(eng, X))
        del X
        e, got = wall(eng.result)
        w = got["Wns"]
        t0 = time.perf_counter()
        B = got["blobs"].reshape(N, -1)
        hm = (w[:, None] * B).sum(0) / w.sum()
        t1 = time.perf_counter()
        hq = host_summaries(got["blobs"], w)[1]
        t2 = time.perf_counter()
        if k:
            for name, v in zip(t, (a, b, s, e, (t1 - t0) * 1e3, (t2 - t1) * 1e3)):
                t[name].append(v)
        assert np.allclose(p.mean, hm, rtol=1e-9, atol=1e-12) and np.array_equal(p.mean, mean)
        print(label, k, round(a, 3), round(b, 3), round(s, 3), round(e, 3), round((t2 - t0) * 1e3, 1), flush=True)
    m = {name: med(v) for name, v in t.items()}
    out["device_route"] = {"total_ms": m["predictive_ms"], "rebuild_ms": m["rebuild_ms"], "summaries_ms": m["summaries_ms"]}
    out["old_route"] = {"result_ms": m["result_ms"], "rebuild_ms": m["rebuild_ms"], "download_ms": m["result_ms"] - m["rebuild_ms"],
                        "host_mean_ms": m["host_mean_ms"], "host_quantiles_ms": m["host_quantiles_ms"],
                        "total_ms": m["result_ms"] + m["host_mean_ms"] + m["host_quantiles_ms"]}
    out["all"] = t
    out["band_of_column_0"] = [float(v) for v in p.wquantiles[:, 0]]
    out["host_band_of_column_0"] = [float(v) for v in hq[:, 0]]
    print(label, out["device_route"], out["old_route"], flush=True)
    rec[label] = out
    del r, eng, got, B, p
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "all"} for k, v in rec.items()}))
