#!/usr/bin/env python3
"""The regression-adjusted posterior (Beaumont, Zhang and Balding 2002) of a run stopped at a loose ϵ: Lotka-Volterra (x' = ax - bxy,
y' = -cy + exy by classical RK4, noisy observations of (x, y)), unknown θ = (a, b, c, e).  With ``blobs=True`` every particle
carries the simulated data behind its distance; ``adjust=dict(wquantiles=(0.025, 0.5, 0.975))`` regresses the parameters on those
data under the population's weights and moves every particle to where it would sit had its simulation hit the observation,
θ - βᵀ(s - s_obs) -- on the device, next to the raw summary of the same population.  The raw band of a loose ϵ is wide; the adjusted
band is what a much tighter (and much more expensive) ϵ would give.  ``ridge`` keeps the 20 x 20 normal equations well posed.
The rate constants are positive, and a straight line subtracted from them need not be: the second table repeats the adjustment on
the same engine with ``transform="log"`` (the regression runs on log θ and the rows are transformed back, so none is negative) and
``hcorr=True`` (the heteroscedastic correction of Blum and François 2010: residuals rescaled to the spread at the observation).

    python examples/regression_adjustment.py [nparticles] [ϵ]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from abcdez_amd import Factored, LotkaVolterraRK4, Uniform, abcdesmc

# ten observations (x, y) of the system at θ* = (1, 0.4, 1, 0.3) from (1, 0.5), one per time unit, with N(0, 0.1²) noise
OBS = (1.03, 0.58, 2.37, 0.16, 5.75, 0.38, 11.55, 1.69, 3.52, 9.01, 0.52, 5.03, 0.3, 2.05, 0.54, 0.93, 1.26, 0.39, 2.91, 0.25)
TRUE = (1.0, 0.4, 1.0, 0.3)
PROBS = (0.025, 0.5, 0.975)


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 16
    eps = float(sys.argv[2]) if len(sys.argv) > 2 else 4.0
    prior = Factored(*[Uniform(0.0, 2.0)] * 4)
    sim = LotkaVolterraRK4(OBS, x0=1.0, y0=0.5, dt=0.02, steps_per_obs=50, noise=0.1, blobs=True)
    t = time.perf_counter()
    r = abcdesmc(prior, sim, eps, None, nparticles=N, verbose=False, rng=1, download=False, summary=dict(cov=False, wquantiles=PROBS),
                 adjust=dict(cov=False, wquantiles=PROBS, ridge=1e-6))
    dt = time.perf_counter() - t
    raw, adj = r.summary, r.adjusted
    print(f"{N} particles, {r.iters} generations and {r.nsims} simulations to ϵ = {r.ϵ:.3f} in {dt:.2f} s; {adj.n_pos} particles count")
    print(" θ    truth      raw 2.5 %    median    97.5 %   |  adjusted 2.5 %    median    97.5 %   width ratio")
    for k, name in enumerate("abce"):
        a, b = raw.wquantiles[:, k], adj.wquantiles[:, k]
        print(f" {name}  {TRUE[k]:7.3f}    {a[0]:9.3f} {a[1]:9.3f} {a[2]:9.3f}   |       {b[0]:9.3f} {b[1]:9.3f} {b[2]:9.3f}   {(b[2] - b[0]) / (a[2] - a[0]):9.2f}")
    low = (0.0,) + PROBS
    plain = r.engine.posterior_adjusted(cov=False, wquantiles=low, ridge=1e-6)
    logged = r.engine.posterior_adjusted(cov=False, wquantiles=low, ridge=1e-6, transform="log", hcorr=True)
    print(' θ    plain: smallest adjusted value   |  transform="log", hcorr=True: smallest     2.5 %    median    97.5 %')
    for k, name in enumerate("abce"):
        b = logged.wquantiles[:, k]
        print(f" {name}            {plain.wquantiles[0, k]:9.3f}              |                          {b[0]:9.3f} {b[1]:9.3f} {b[2]:9.3f} {b[3]:9.3f}")


if __name__ == "__main__":
    main()
