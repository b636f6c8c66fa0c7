"""Compile-time resources of the column-summary gathers (csrc/abz_columns.hip), by the technique of
tests/test_wquantile_kernel_resources.py.  They are the twins of the population's gathers for a dense per-particle matrix: the
moment passes hold 64 doubles of terms per thread, the quantile gather and the range pass 16 / 8 columns of running minima and
maxima -- an array that ended up in scratch memory would go out to HBM and back per position, invisible in every parity test --
and the second-moment pass keeps 4 x 256 x 4 partial sums in LDS (32 KB), which must leave room for several workgroups per CU."""
import pytest

from test_kernel_resources import HIPCC, resource_table

KERNELS = ("col_first_kernel", "col_second_kernel", "col_wq_gather_kernel", "col_hist_range_kernel", "col_hist_bin_kernel")


@pytest.mark.skipif(HIPCC is None, reason="needs hipcc")
def test_every_columns_kernel_runs_without_scratch_and_fits_the_lds():
    rows = resource_table("abz_columns.hip")
    assert len(rows) == len(KERNELS), sorted(rows)
    for k in KERNELS:
        assert any(k in name for name in rows), (k, sorted(rows))
    for name, r in rows.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs Spill"]) == 0, (name, r)
        assert r["Dynamic Stack"] == "False", (name, r)
        assert int(r["LDS Size [bytes/block]"]) <= 40 * 1024, (name, r)          # four workgroups per CU
        assert int(r["Occupancy [waves/SIMD]"]) >= 3, (name, r)
        print(name, "VGPRs", r["VGPRs"], "LDS", r["LDS Size [bytes/block]"], "waves/SIMD", r["Occupancy [waves/SIMD]"])
