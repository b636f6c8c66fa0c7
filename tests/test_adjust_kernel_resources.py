"""Compile-time resources of the regression adjustment's two kernels (csrc/abz_adjust.hip), by the technique of
tests/test_columns_kernel_resources.py.  The cross pass holds 4 centred blob columns of 8 rows per thread (64 registers) next to the
streamed parameter column and collects 4 x 256 x 4 partial sums in LDS; the apply pass keeps 8 accumulators and stages 256 x 8
coefficients in LDS.  An array that ended up in scratch memory would go out to HBM and back per position, invisible in every
parity test.  The occupancy is compared with the shipped kin of the cross pass: the second-moment pass over a dense matrix
(sum_second_kernel<ColView>, csrc/abz_summary.hip) of the same tree."""
import pytest

from test_kernel_resources import HIPCC, resource_table

KERNELS = ("adj_cross_kernel", "adj_apply_kernel")


@pytest.mark.skipif(HIPCC is None, reason="needs hipcc")
def test_the_adjust_kernels_run_without_scratch_and_keep_their_twins_occupancy():
    rows = resource_table("abz_adjust.hip")
    assert len(rows) == len(KERNELS), sorted(rows)
    for k in KERNELS:
        assert any(k in name for name in rows), (k, sorted(rows))
    twin = [r for name, r in resource_table("abz_summary.hip").items() if "sum_second_kernel" in name and "ColView" in name]
    assert len(twin) == 1
    floor = int(twin[0]["Occupancy [waves/SIMD]"])
    assert floor >= 1
    for name, r in rows.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
        assert r["Dynamic Stack"] == "False", (name, r)
        assert int(r["LDS Size [bytes/block]"]) <= 64 * 1024, (name, r)          # the static limit
        assert int(r["Occupancy [waves/SIMD]"]) >= floor, (name, r, floor)
        print(name, "VGPRs", r["VGPRs"], "LDS", r["LDS Size [bytes/block]"], "waves/SIMD", r["Occupancy [waves/SIMD]"], "twin", floor)
