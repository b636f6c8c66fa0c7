#!/usr/bin/env python3
"""Weighted marginal quantiles on the device against the unweighted path, same process, one GPU: an smc32-shaped population
(d = 32 MVN, 2^22 particles) and five probabilities.
  (a) engine.posterior_summary(cov=False, wquantiles=P)   one library call for the 32 columns, one read-back
  (b) engine.posterior_summary(cov=False, quantiles=P)    a column gather and five rank selects per column, 160 read-backs
Both on a run with an indicator kernel (where both apply; the results are compared), then (a) alone on a run with an
Epanechnikov kernel, whose unequal weights (b) refuses.  The runs are stopped after a few generations: the summaries' cost depends
on N, d and the share of live positions, not on how far the run got.  One warm-up and `REPS` alternating repetitions, HIP events
around each call (every call ends in its own read-back and synchronisation), medians; the first-moment pass both share is timed
alone and reported next to them.  Writes profiles/r07_wquantiles.json (or the path given as the first argument)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import abcdez_amd as A

PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)
REPS = 7
d = 32
N = int(os.environ.get("ABCDEZ_TIME_N", 1 << 22))
GENS = 6
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r07_wquantiles.json")
assert torch.cuda.is_available(), "this measurement needs the GPU"
prior = A.Factored(*[A.Normal(0.0, 1.0) for _ in range(d)])
sim = A.MVNormal(tuple([1.0] * d))


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


r = run(A.IndicatorStrict0toϵ)
eng = r.engine
eng._stream()
res = alternate({
    "wquantiles": lambda: eng.posterior_summary(cov=False, wquantiles=PROBS),
    "quantiles": lambda: eng.posterior_summary(cov=False, quantiles=PROBS),
    "moments_only": lambda: eng.posterior_summary(cov=False),
})
sw, sq = res["wquantiles"][2], res["quantiles"][2]
span = np.asarray(sq.quantiles).max(axis=0) - np.asarray(sq.quantiles).min(axis=0)
rec = {
    "config": {"d": d, "N": N, "generations": r.iters, "probs": list(PROBS), "reps": REPS, "n_pos": sw.n_pos, "n_mass": sw.n_mass},
    "indicator": {
        "wquantiles_ms": res["wquantiles"][0], "wquantiles_all_ms": res["wquantiles"][1],
        "quantiles_ms": res["quantiles"][0], "quantiles_all_ms": res["quantiles"][1],
        "moments_only_ms": res["moments_only"][0],
        "wquantiles_minus_moments_ms": res["wquantiles"][0] - res["moments_only"][0],
        "quantiles_minus_moments_ms": res["quantiles"][0] - res["moments_only"][0],
        "max_abs_diff_over_central_95_width": float((np.abs(sw.wquantiles - sq.quantiles) / span).max()),
    },
}
del r, eng
torch.cuda.empty_cache()
r = run(A.Epa0toϵ)
eng = r.engine
eng._stream()
res = alternate({
    "wquantiles": lambda: eng.posterior_summary(cov=False, wquantiles=PROBS),
    "moments_only": lambda: eng.posterior_summary(cov=False),
})
se = res["wquantiles"][2]
rec["epanechnikov"] = {
    "generations": r.iters, "n_pos": se.n_pos, "n_mass": se.n_mass, "M": se.M,
    "wquantiles_ms": res["wquantiles"][0], "wquantiles_all_ms": res["wquantiles"][1], "moments_only_ms": res["moments_only"][0],
    "wquantiles_minus_moments_ms": res["wquantiles"][0] - res["moments_only"][0],
    "passes_bytes_model": 11 * 16 * se.n_pos * d,       # m_(1) comes with the gather; 8 digit passes, closing pass, gather's write + read
}
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec))
