"""Compile-time resources of the column-summary gathers: the instantiations over the dense-matrix source (ColView,
csrc/abz_summary.h) of the five kernels that read values (csrc/abz_summary.hip, abz_wquantile.hip, abz_hist.hip), by the technique
of tests/test_wquantile_kernel_resources.py.  The moment passes hold 64 doubles of terms per thread, the quantile gather and the
range pass 16 / 8 columns of running minima and maxima -- an array that ended up in scratch memory would go out to HBM and back
per position, invisible in every parity test -- and the second-moment pass keeps 4 x 256 x 4 partial sums in LDS (32 KB), which
must leave room for several workgroups per CU."""
import pytest

from test_kernel_resources import HIPCC, resource_table

SOURCE = "ColView"
KERNELS = {"abz_summary.hip": ("sum_first_kernel", "sum_second_kernel"), "abz_wquantile.hip": ("wq_gather_kernel",),
           "abz_hist.hip": ("hist_range_kernel", "hist_bin_kernel")}


def matrix_source_rows():
    """mangled name -> resources of the five matrix-source instantiations, each found exactly once in its file"""
    rows = {}
    for src, kernels in KERNELS.items():
        table = resource_table(src)
        for k in kernels:
            hits = {name: r for name, r in table.items() if k in name and SOURCE in name}
            assert len(hits) == 1, (k, sorted(table))
            rows.update(hits)
    return rows


@pytest.mark.skipif(HIPCC is None, reason="needs hipcc")
def test_every_columns_kernel_runs_without_scratch_and_fits_the_lds():
    rows = matrix_source_rows()
    assert len(rows) == sum(len(k) for k in KERNELS.values()), sorted(rows)
    for name, r in rows.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs Spill"]) == 0, (name, r)
        assert r["Dynamic Stack"] == "False", (name, r)
        assert int(r["LDS Size [bytes/block]"]) <= 40 * 1024, (name, r)          # four workgroups per CU
        assert int(r["Occupancy [waves/SIMD]"]) >= 3, (name, r)
        print(name, "VGPRs", r["VGPRs"], "LDS", r["LDS Size [bytes/block]"], "waves/SIMD", r["Occupancy [waves/SIMD]"])
