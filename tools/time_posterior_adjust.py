#!/usr/bin/env python3
"""The regression-adjusted posterior on the device against the route it replaces, same process, one GPU, HIP events:
  lv      Lotka-Volterra RK4 (the `lv` configuration's model, tests/golden/lv_data.json), 2^20 particles, 32-double blobs, d = 4
  smc32   MVNormal(blobs=True) in 32 dimensions, 2^22 particles, 32-double blobs, d = 32
each stopped after a few generations.  One warm-up and `REPS` repetitions each, medians reported with the spread (min, max) and
every repetition listed:
  (a)  engine.posterior_adjusted(wquantiles=(0.025, 0.5, 0.975)) as a whole, and its parts on their own: the blob rebuild, the
       moments of both halves + the cross pass, the host solve, the apply pass, the summaries of the adjusted rows
  (o)  the route of old: engine.result() with blobs (rebuild + pinned download), and on the host the same adjustment with
       vectorised numpy (weighted centring, np.linalg.lstsq on the sqrt(w)-scaled matrices, one matrix product, mean and
       covariance of the adjusted rows; no quantiles), plus the blob
       download alone (the N x n_blob matrix to pinned memory)
and the byte model of the two new passes -- cross: 8 N + 8 (ld n + lds n) bytes read, n the counting positions; apply: the same
reads + 8 d N written -- as a fraction of the part's HBM rate.
Writes profiles/r11_posterior_adjust.json (or the path given as the first argument).  ABCDEZ_TIME_SCALE=k divides both N by 2^k;
ABCDEZ_TIME_REPS sets the repetitions (default 9, at least 7)."""
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
from abcdez_amd import summary as S

REPS = max(7, int(os.environ.get("ABCDEZ_TIME_REPS", 9)))
SHIFT = int(os.environ.get("ABCDEZ_TIME_SCALE", 0))
PROBS = (0.025, 0.5, 0.975)
HBM_GBS = 8000.0                 # MI355X: 8 TB/s peak HBM3E bandwidth
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r11_posterior_adjust.json")
assert torch.cuda.is_available(), "this measurement needs the GPU"


def lv_sim():
    with open(os.path.join(ROOT, "tests", "golden", "lv_data.json")) as f:
        g = json.load(f)
    return A.LotkaVolterraRK4(tuple(g["obs"]), x0=g["x0"], y0=g["y0"], dt=g["dt"], steps_per_obs=g["steps_per_obs"], noise=g["noise"],
                              blobs=True)


CASES = {
    "lv": dict(prior=A.Factored(*[A.Uniform(0.0, 2.0)] * 4), sim=lv_sim(), eps=1.0, N=(1 << 20) >> SHIFT, abck=A.IndicatorStrict0toeps,
               gens=4, ridge=0.0),
    "smc32": dict(prior=A.Factored(*[A.Normal(0.0, 1.0)] * 32), sim=A.MVNormal(tuple([1.0] * 32), blobs=True), eps=0.0,
                  N=(1 << 22) >> SHIFT, abck=A.IndicatorStrict0toeps, gens=4, ridge=0.0),
}


def ev(fn):
    """(milliseconds between two HIP events around fn on the current stream, after a final synchronisation; fn's result)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    got = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), got


def rebuild(eng):
    th, _, dl = eng.state
    X = torch.zeros((eng.N, eng.ops.blob_width()), dtype=torch.float64, device=eng.device)
    redo = torch.empty_like(dl)
    eng.ops.blob_eval(th, eng.stamp[eng.cur], X, redo)
    assert torch.equal(redo.view(torch.int64), dl.view(torch.int64))
    return X


def host_adjust(P, B, w, t, ridge):
    """the adjustment as a user of the parent commit does it from r.P, r.blobs, r.Wns: vectorised numpy, lstsq"""
    live = w > 0
    P, B, w = P[live].reshape(live.sum(), -1), B[live].reshape(live.sum(), -1), w[live]
    W = w.sum()
    xm, sm = (w[:, None] * P).sum(0) / W, (w[:, None] * B).sum(0) / W
    r = np.sqrt(w)[:, None]
    beta = np.linalg.lstsq(r * (B - sm), r * (P - xm), rcond=None)[0]
    Y = P - (B - t) @ beta
    mean = (w[:, None] * Y).sum(0) / W
    C = Y - mean
    return beta, mean, (w[:, None] * C).T @ C / W               # mean and covariance only: no host quantiles are charged to this route


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


rec = {"config": {"reps": REPS, "scale_shift": SHIFT, "probs": PROBS, "hbm_gb_per_s": HBM_GBS}}
for label, c in CASES.items():
    N = c["N"]
    r = A.abcdesmc(c["prior"], c["sim"], c["eps"], None, nparticles=N, ABCk=c["abck"], verbose=False, rng=1, nsims_max=10 ** 13,
                   max_iters=c["gens"], summary=dict(cov=False), download=False)
    eng = r.engine
    eng._stream()
    d, nb, lds, ld = eng.spec.d, eng.spec.n_blob, eng.ops.blob_width(), eng.spec.ld
    cols = list(range(nb))
    tgt = S.adjust_target(None, cols, nb, tuple(eng.spec.sim.data()))
    pop = eng._live_population()
    wns = eng.wns
    n_pos = r.summary.n_pos
    out = {"N": N, "d": d, "ld": ld, "n_blob": nb, "blob_width": lds, "generations": r.iters, "n_pos": n_pos,
           "device_bytes": N * (lds + d) * 8, "blob_download_bytes": N * nb * 8}
    names = ("adjusted_ms", "rebuild_ms", "moments_cross_ms", "cross_only_ms", "solve_ms", "apply_ms", "summaries_ms", "result_ms",
             "blob_download_ms", "host_adjust_ms")
    t = {k: [] for k in names}
    for k in range(REPS + 1):                                                    # the first round warms up
        a, adj = ev(lambda: eng.posterior_adjusted(wquantiles=PROBS, ridge=c["ridge"]))
        b, Sb = ev(lambda: rebuild(eng))

        def moments_cross():
            xm = eng.ops.posterior_moments(*pop, N, want_second=False)[0]
            sm, Sss = eng.ops.columns_moments(Sb, wns, m=nb, want_second=True)[:2]
            return xm, sm, Sss, eng.ops.adjust_cross(*pop, N, Sb, cols, sm, xm)
        mc, (xm, sm, Sss, Ssx) = ev(moments_cross)
        co, _ = ev(lambda: eng.ops.adjust_cross(*pop, N, Sb, cols, sm, xm))
        t0 = time.perf_counter()
        beta = S.adjust_solve(Sss, Ssx, c["ridge"], cols)
        sv = (time.perf_counter() - t0) * 1e3
        ap, Y = ev(lambda: eng.ops.adjust_apply(*pop, N, Sb, cols, tgt, beta))

        def summaries():
            return eng.ops.columns_moments(Y, wns, m=d, want_second=True)[0], eng.ops.columns_wquantiles(Y, wns, PROBS, m=d)[0]
        sm_ms, (ymean, yq) = ev(summaries)
        bd, _ = ev(lambda: eng._to_host([Sb[:, :nb]]))
        del Sb, Y
        e, got = ev(eng.result)
        t0 = time.perf_counter()
        hbeta, hmean, hcov = host_adjust(got["P"], got["blobs"], got["Wns"], tgt, c["ridge"])
        ha = (time.perf_counter() - t0) * 1e3
        if k:
            for name, v in zip(names, (a, b, mc, co, sv, ap, sm_ms, e, bd, ha)):
                t[name].append(v)
        assert np.array_equal(adj.mean, ymean) and np.allclose(adj.mean, hmean, rtol=1e-4, atol=1e-7), (adj.mean, hmean)   # lstsq solves by SVD
        print(label, k, *(round(v, 3) for v in (a, b, mc, co, sv, ap, sm_ms, e, bd, ha)), flush=True)
    m = {name: spread(v) for name, v in t.items()}
    cross_bytes = 8 * N + 8 * (ld * n_pos + lds * n_pos)
    apply_bytes = cross_bytes + 8 * d * N
    out["device_route"] = {k: m[k] for k in ("adjusted_ms", "rebuild_ms", "moments_cross_ms", "cross_only_ms", "solve_ms", "apply_ms",
                                             "summaries_ms")}
    out["old_route"] = {"result_ms": m["result_ms"], "blob_download_ms": m["blob_download_ms"], "host_adjust_ms": m["host_adjust_ms"],
                        "total_ms": m["result_ms"]["median"] + m["host_adjust_ms"]["median"]}
    out["byte_model"] = {
        "cross_bytes": cross_bytes, "cross_gb_per_s": cross_bytes / (m["cross_only_ms"]["median"] * 1e6),
        "cross_fraction_of_hbm": cross_bytes / (m["cross_only_ms"]["median"] * 1e6) / HBM_GBS,
        "apply_bytes": apply_bytes, "apply_gb_per_s": apply_bytes / (m["apply_ms"]["median"] * 1e6),
        "apply_fraction_of_hbm": apply_bytes / (m["apply_ms"]["median"] * 1e6) / HBM_GBS}
    out["faster_than_blob_download_alone"] = bool(m["adjusted_ms"]["median"] < m["blob_download_ms"]["median"])
    out["all"] = t
    out["raw_mean"] = [float(v) for v in adj.x_mean]
    out["adjusted_mean"] = [float(v) for v in adj.mean]
    out["adjusted_band_of_parameter_0"] = [float(v) for v in adj.wquantiles[:, 0]]
    print(label, out["device_route"], out["old_route"], out["byte_model"], flush=True)
    rec[label] = out
    del r, eng, got, adj, pop, wns
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "all"} for k, v in rec.items()}))
