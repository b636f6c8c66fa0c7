#!/usr/bin/env python3
"""The posterior sample on the device against what it replaces, same process, one GPU:
  smc32   d = 32 MVN, 2^22 particles, Epanechnikov kernel (unequal weights), no blobs
  lv      Lotka-Volterra RK4, 2^20 particles, indicator kernel, blobs on (32 doubles per particle)
for n = 10^4 and n = 2^20 each:
  (s)  engine.posterior_sample(n)                     draw, gather (and with blobs the simulator re-run for the n rows), n rows to the host
  (o)  engine.result() + wsample_stratified(r.Wns, engine=) + host indexing P[idx], C[idx], blobs[idx]   -- the route of old.  It
       draws N indices whatever n is; for n < N the first n of a shuffle-free prefix would not be a sample, so the route is timed
       as it is used: all N indices, all N rows indexed, and with blobs the simulator re-run for all N particles inside result()
The runs are stopped after a few generations: the cost depends on N, d, n and the share of counting positions, not on how far the run
got.  One warm-up and `REPS` repetitions; (s) between HIP events AND by the wall clock (the call ends in its own read-back), (o) by the
wall clock, its three parts separately.  Bytes by the model of DESIGN.md 4.6 "Posterior sample" next to the times.  Writes
profiles/r09_posterior_sample.json (or the path given as the first argument).  ABCDEZ_TIME_SCALE=k divides both N by 2^k (a
smaller box)."""
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

REPS = 5
SHIFT = int(os.environ.get("ABCDEZ_TIME_SCALE", 0))
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r09_posterior_sample.json")
assert torch.cuda.is_available(), "this measurement needs the GPU"


def lv_sim():
    with open(os.path.join(ROOT, "tests", "golden", "lv_data.json")) as f:
        g = json.load(f)
    return A.LotkaVolterraRK4(tuple(g["obs"]), x0=g["x0"], y0=g["y0"], dt=g["dt"], steps_per_obs=g["steps_per_obs"], noise=g["noise"],
                              blobs=True)


CASES = {
    "smc32": dict(prior=A.Factored(*[A.Normal(0.0, 1.0) for _ in range(32)]), sim=A.MVNormal(tuple([1.0] * 32)), eps=0.0,
                  N=(1 << 22) >> SHIFT, abck=A.Epa0toeps, gens=6),
    "lv": dict(prior=A.Factored(*[A.Uniform(0.0, 2.0)] * 4), sim=lv_sim(), eps=1.0, N=(1 << 20) >> SHIFT, abck=A.IndicatorStrict0toeps,
               gens=4),
}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t = time.perf_counter()
    a.record()
    got = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t) * 1e3, got


def med(v):
    return statistics.median(v)


rec = {"config": {"reps": REPS, "scale_shift": SHIFT}}
for label, c in CASES.items():
    N = c["N"]
    r = A.abcdesmc(c["prior"], c["sim"], c["eps"], None, nparticles=N, ABCk=c["abck"], verbose=False, rng=1, nsims_max=10 ** 13,
                   max_iters=c["gens"], summary=dict(cov=False), download=False)
    eng = r.engine
    eng._stream()
    d, ld, nb = eng.spec.d, eng.spec.ld, eng.spec.n_blob
    out = {"N": N, "d": d, "n_blob": nb, "generations": r.iters, "n_pos": r.summary.n_pos}
    for n in (10 ** 4, (1 << 20) >> SHIFT):
        eng.posterior_sample(n)
        ev, wall, s = [], [], None
        for k in range(REPS):
            e, w, s = timed(lambda: eng.posterior_sample(n, draw=k))
            ev.append(e)
            wall.append(w)
        # count, tile sums and scan read the weights, the scan writes C; the search reads ~22 words a stratum from C and the offsets;
        # the gather reads n rows (whole 64-byte pieces at least) and writes P, the distances (and rows, stamps with blobs)
        by = 3 * N * 8 + N * 8 + n * (22 * 8 + 4) + n * (max(ld * 8, 64) + d * 8 + 16 + 4) + (n * (ld * 8 + 16) if nb else 0)
        out["sample_n_%d" % n] = {"n": n, "event_ms": med(ev), "event_all_ms": ev, "wall_ms": med(wall), "wall_all_ms": wall,
                                  "n_mass": s.n_mass, "bytes_model_without_blob_rerun": by,
                                  "host_bytes": int(s.P.nbytes + s.C.nbytes + 4 * n + (s.blobs.nbytes if s.blobs is not None else 0))}
        print(label, n, out["sample_n_%d" % n]["event_ms"], out["sample_n_%d" % n]["wall_ms"], flush=True)
    parts = {"result_ms": [], "wsample_ms": [], "index_ms": []}
    for k in range(REPS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = eng.result()
        t1 = time.perf_counter()
        idx = A.wsample_stratified(got["Wns"], draw=k, engine=eng)
        t2 = time.perf_counter()
        P, Cc = got["P"][idx], got["C"][idx]
        B = got["blobs"][idx] if got["blobs"] is not None else None
        t3 = time.perf_counter()
        if k:                                                                    # the first round warms up
            parts["result_ms"].append((t1 - t0) * 1e3)
            parts["wsample_ms"].append((t2 - t1) * 1e3)
            parts["index_ms"].append((t3 - t2) * 1e3)
    out["old_route"] = {k: med(v) for k, v in parts.items()}
    out["old_route"]["total_ms"] = sum(out["old_route"].values())
    out["old_route"]["all"] = parts
    out["old_route"]["download_bytes"] = int(sum(v.nbytes for v in got.values() if isinstance(v, np.ndarray)))
    out["old_route"]["draws"] = int(idx.size)
    print(label, "old route", {k: v for k, v in out["old_route"].items() if k != "all"}, flush=True)
    rec[label] = out
    del r, eng, got, P, Cc, B, idx, s
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec))
