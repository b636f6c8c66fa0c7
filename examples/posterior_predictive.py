#!/usr/bin/env python3
"""A posterior predictive check without moving the simulations to the host: Lotka-Volterra (x' = ax - bxy, y' = -cy + exy by
classical RK4, noisy observations of (x, y)), unknown θ = (a, b, c, e).  With ``blobs=True`` every particle carries the simulated
data behind its distance (the reference's blobs, docs/src/index.md:298-324); ``predictive=dict(wquantiles=(0.025, 0.5, 0.975))``
summarises them where the population lives -- the weighted mean and the 95 % band of the accepted simulations per observation --
and ``download=False`` keeps the N x n_blob matrix on the device: a few hundred numbers come back, printed here beside the data.

    python examples/posterior_predictive.py [nparticles]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from abcdez_amd import Factored, LotkaVolterraRK4, Uniform, abcdesmc

# ten observations (x, y) of the system at θ* = (1, 0.4, 1, 0.3) from (1, 0.5), one per time unit, with N(0, 0.1²) noise
OBS = (1.03, 0.58, 2.37, 0.16, 5.75, 0.38, 11.55, 1.69, 3.52, 9.01, 0.52, 5.03, 0.3, 2.05, 0.54, 0.93, 1.26, 0.39, 2.91, 0.25)


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 16
    prior = Factored(*[Uniform(0.0, 2.0)] * 4)
    sim = LotkaVolterraRK4(OBS, x0=1.0, y0=0.5, dt=0.02, steps_per_obs=50, noise=0.1, blobs=True)
    t = time.perf_counter()
    r = abcdesmc(prior, sim, 1.0, None, nparticles=N, verbose=False, rng=1, download=False, summary=dict(cov=False),
                 predictive=dict(wquantiles=(0.025, 0.5, 0.975)))
    dt = time.perf_counter() - t
    p = r.predictive
    print(f"{N} particles, {r.iters} generations to ϵ = {r.ϵ:.3f} in {dt:.2f} s; posterior mean of θ = {r.summary.mean.round(3)}")
    print(f"{p.n_pos} particles count (ess {p.ess:.0f}); {p.mean.size} simulated numbers per particle summarised on the device")
    print(" obs  series      data      2.5 %     median    97.5 %     mean   inside")
    lo, mid, hi = p.wquantiles
    for k, y in enumerate(OBS):
        print(f"{k // 2:4d}  {'xy'[k % 2]}      {y:9.3f}  {lo[k]:9.3f}  {mid[k]:9.3f}  {hi[k]:9.3f}  {p.mean[k]:9.3f}   {'yes' if lo[k] <= y <= hi[k] else 'NO'}")


if __name__ == "__main__":
    main()
