"""Compile-time resources of the kernels of csrc/abz_adjust_hcorr.hip, after the pattern of tests/test_adjust_kernel_resources.py.
The scaled apply keeps TWO accumulator sets per thread (the beta sum centred on smean, the gamma sum centred on t) and stages both
coefficient matrices through LDS.  With ADJ_KS = 4 columns per trip that is 8 accumulators and 2 x 256 x 4 coefficients, the plain
apply's budget: about 21 KiB of LDS per workgroup (seven workgroups per CU, as the plain apply has eight at 19 KiB) and, with the
inlined abz_exp and the back-transform, 85 registers -- five waves per SIMD.  Two sets of 8 would double the LDS (four workgroups
per CU) for no gain in a pass that is bound by the rows it reads.  Pinned here: no scratch, no spills, the static LDS limit, five
waves for the scaled apply, six for the log residuals, and for the cross pass over a dense matrix the occupancy of its twin over
the population (the same kernel text, csrc/abz_adjust.h)."""
import pytest

from test_kernel_resources import HIPCC, resource_table

KERNELS = {"adj_transform_kernel": 1, "adj_cross_kernel": 1, "adj_logres_kernel": 2, "adj_scaled_kernel": 4}      # name -> instances


@pytest.mark.skipif(HIPCC is None, reason="needs hipcc")
def test_the_hcorr_kernels_run_without_scratch_and_keep_their_occupancy():
    rows = resource_table("abz_adjust_hcorr.hip")
    assert len(rows) == sum(KERNELS.values()), sorted(rows)
    for k, n in KERNELS.items():
        assert sum(k in name for name in rows) == n, (k, sorted(rows))
    twin = [r for name, r in resource_table("abz_adjust.hip").items() if "adj_cross_kernel" in name]
    assert len(twin) == 1
    cross_floor = int(twin[0]["Occupancy [waves/SIMD]"])
    for name, r in rows.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
        assert r["Dynamic Stack"] == "False", (name, r)
        assert int(r["LDS Size [bytes/block]"]) <= 64 * 1024, (name, r)          # the static limit
        floor = cross_floor if "adj_cross_kernel" in name else 6 if "adj_logres_kernel" in name else 5
        assert int(r["Occupancy [waves/SIMD]"]) >= floor, (name, r, floor)
        if "adj_scaled_kernel" in name:
            assert int(r["LDS Size [bytes/block]"]) <= 22 * 1024, (name, r)      # seven workgroups per CU
        print(name, "VGPRs", r["VGPRs"], "LDS", r["LDS Size [bytes/block]"], "waves/SIMD", r["Occupancy [waves/SIMD]"])
