"""The same numbers through both value sources give the same bits.  The gathers of the posterior calls (sum_first / sum_second,
wq_gather, hist_range / hist_bin) are one kernel text each over two sources of values (csrc/abz_summary.h): the population's
parameter rows, push_p-cast, and a dense per-particle matrix taken as it is.  Here ONE device array is both: a population in
classic storage (bits = NULL, slot0 the row array) under a prior without a discrete factor -- abz_push_p (include/abcdez_spec.h)
is ``pd->discrete ? abz_rint(x) : x``, so it returns the stored value unchanged, which the test verifies through the library's
own push_p first -- handed to the columns_* calls as X with ldx = ld and m = d.  Every pair of calls must return bit-identical
arrays, M and n_mass included; what the numbers themselves must be is pinned by the tests of either call against summary.py.

Shapes: N = 2049 (two tiles, the second holding a single position) and N = 1; d = 5 (a tail for every column blocking of 2, 4 and
8) and d = 17 (one column past a 16-column quantile chunk and past two 8-column range launches); unit weights, and weights with
zeros -- a whole wavefront of either mapping (the moment passes' thread t owns m*512 + 2t + c, the gathers' one position each),
scattered ones and the last position; the rows of the weightless positions hold NaN, which neither source may read."""
import numpy as np
import pytest
import torch

import abcdez_amd as A
from abcdez_amd.engine import HipOps

pytestmark = pytest.mark.gpu

PROBS = (0.0, 0.025, 0.5, 0.975, 1.0)
BINS, BINS2 = 7, 5


def same_bits(a, b, what):
    if a is None or b is None:
        assert a is None and b is None, what
        return
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (what, a, b)


def same_tuple(pop, col, what):
    assert len(pop) == len(col), what
    for f, (x, y) in enumerate(zip(pop, col)):
        if isinstance(x, np.ndarray) or x is None:
            same_bits(x, y, (what, f))
        elif isinstance(x, float):
            same_bits(np.float64(x), np.float64(y), (what, f))
        else:
            assert type(x) is type(y) and x == y, (what, f, x, y)


@pytest.fixture(scope="module", params=[5, 17])
def ops(request):
    d = request.param
    spec = A.ModelSpec(A.Factored(*[A.Normal(0.0, 1.0) for _ in range(d)]), A.MVNormal(tuple([0.25] * d)), A.Epa0toeps, seed=3)
    assert not any(spec.discrete)
    o = HipOps(spec)
    yield o
    o.close()


def weights_with_zeros(N, rng):
    w = rng.random(N) + 0.05
    if N == 1:
        return w                                        # the one position cannot be weightless: the calls would refuse
    w[rng.random(N) < 0.3] = 0.0
    for m in range(4):                                  # positions 128 .. 255 of every quarter: wavefront 1 of the moment passes'
        w[m * 512 + 128:m * 512 + 256] = 0.0            # tile 0, wavefronts 2 and 3 of the gathers' blocks 0, 2, 4 and 6
    w[-1] = 0.0                                         # the last position, alone in its tile at N = 2049
    w[N // 4] += 0.5
    return w / w.sum()


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "zeros"])
@pytest.mark.parametrize("N", [1, 2049])
def test_population_and_matrix_sources_give_the_same_bits(ops, N, weighted):
    d = ops.spec.d
    ld = ops.layout()[0]
    assert ld == ops.spec.ld >= d
    rng = np.random.default_rng(1000 * d + 10 * N + weighted)
    w = weights_with_zeros(N, rng) if weighted else None
    live = np.ones(N, dtype=bool) if w is None else w > 0
    rows = np.zeros((N, ld))
    V = rng.standard_normal((N, d)) * 2.5
    if N > 8:
        for k in range(d):                              # a few exact ties per column
            V[rng.integers(0, N, 3), k] = V[rng.integers(0, N, 3), k]
    rows[:, :d] = np.where(live[:, None], V, np.nan)
    X = torch.from_numpy(rows).to(ops.device)
    dw = None if w is None else torch.from_numpy(w).to(ops.device)
    what = (N, d, weighted)

    pushed = torch.empty_like(X)                        # push_p of this prior returns the stored value unchanged
    ops.push_p(X, pushed)
    same_bits(pushed.cpu().numpy()[:, :d], rows[:, :d], (what, "push_p"))

    for want_second in (True, False):
        same_tuple(ops.posterior_moments(None, X, None, dw, N, want_second=want_second),
                   ops.columns_moments(X, dw, m=d, want_second=want_second), (what, "moments", want_second))
    same_tuple(ops.posterior_wquantiles(None, X, None, dw, N, PROBS), ops.columns_wquantiles(X, dw, PROBS, m=d), (what, "wquantiles"))
    same_tuple(ops.posterior_wquantiles(None, X, None, dw, N, PROBS, k0=1, nk=d - 2),
               ops.columns_wquantiles(X, dw, PROBS, m=d, k0=1, nk=d - 2), (what, "wquantiles of a column range"))
    given = np.tile(np.array([-3.0, 2.0]), (d, 1))
    for rg in (None, given):
        opts = dict(bins=BINS, range=rg, pairs=[(0, d - 1)], bins2=BINS2)
        pop = ops.posterior_histograms(None, X, None, dw, N, **opts)
        col = ops.columns_histograms(X, dw, m=d, **opts)
        same_tuple(pop, col, (what, "histograms", "automatic" if rg is None else "given"))
        assert pop[5] > 0 and 1 <= pop[6] <= int(live.sum()), what       # M and n_mass: the calls did count something
