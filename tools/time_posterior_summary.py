#!/usr/bin/env python3
"""Posterior summaries of the bench workload (d = 32 MVN, 2^22 particles, eps_target 6.0) by two routes, same process, same box:
  (a) on the device: engine.posterior_summary(cov=True, quantiles=(0.025, 0.5, 0.975))
  (b) what there was before: engine.result() -- the download of the rows -- plus numpy mean, covariance and quantiles of the
      particles with a positive weight.
One warm-up and five repetitions each, medians, wall clock with the device drained before and after; the stages of (a) also by
HIP events (first-moment pass + finish alone; both passes; the 32 column gathers with three selects each).  The second pass
has no launch of its own in the ABI: its time is the difference of the two moment calls, which run the same first pass.
Writes profiles/posterior_summary_timing.json (or the path given as the first argument)."""
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

PROBS = (0.025, 0.5, 0.975)
d, N = 32, 1 << 22
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "posterior_summary_timing.json")
prior = A.Factored(*[A.Normal(0.0, 1.0) for _ in range(d)])
sim = A.MVNormal(tuple([1.0] * d))
r = A.abcdesmc(prior, sim, 6.0, None, nparticles=N, verbose=False, rng=1, nsims_max=10 ** 12, summary=True, download=False)
eng = r.engine


def wall(fn, reps=5):
    fn()                                                  # warm-up
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts, got


def events(fn, reps=5):
    fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def route_a():
    return eng.posterior_summary(cov=True, corrected=True, quantiles=PROBS)


def route_b():
    res = eng.result()
    live = res["Wns"] > 0
    X, w = res["P"][live], res["Wns"][live]
    return (np.average(X, axis=0, weights=w), np.cov(X.T, aweights=w), np.quantile(X, PROBS, axis=0))


def download_only():
    return eng.result()


eng._stream()
pop = (eng.bits[eng.bc], eng.buf[0][0], eng.buf[1][0], eng.wns)
first_ms = events(lambda: eng.ops.posterior_moments(*pop, N, want_second=False))
both_ms = events(lambda: eng.ops.posterior_moments(*pop, N, want_second=True))
quant_ms = events(lambda: [eng.ops.posterior_quantiles(*pop, N, k, PROBS) for k in range(d)])
a_s, a_all, sa = wall(route_a)
b_s, b_all, sb = wall(route_b)
dl_s, _, _ = wall(download_only)
rows_bytes = N * d * 8
second_ms = both_ms - first_ms
rec = {
    "config": {"d": d, "N": N, "eps_target": 6.0, "generations": r.iters, "n_pos": sa.n_pos, "probs": list(PROBS)},
    "a_device_summary_s": a_s, "a_all_s": a_all,
    "b_download_plus_numpy_s": b_s, "b_all_s": b_all, "b_download_only_s": dl_s,
    "a_beats_b": a_s < b_s, "speedup_b_over_a": b_s / a_s,
    "a_stages_ms": {"first_moment_pass_and_finish": first_ms, "both_moment_passes_and_finishes": both_ms,
                    "second_moment_pass_and_finish_by_difference": second_ms, "column_gathers_and_selects_32x3": quant_ms},
    "rows_bytes_one_read": rows_bytes,
    "first_pass_GBps_of_rows": rows_bytes / (first_ms * 1e-3) / 1e9,
    "second_pass_GBps_of_rows": rows_bytes / (second_ms * 1e-3) / 1e9,
    "mean_max_abs_diff_a_vs_b": float(np.abs(sa.mean - sb[0]).max()),
    "cov_max_abs_diff_a_vs_b": float(np.abs(sa.cov - sb[1]).max()),
    "quantile_max_abs_diff_a_vs_b": float(np.abs(sa.quantiles - sb[2]).max()),
}
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec))
