"""Compile-time resources of the histogram kernels (csrc/abz_hist.hip), by the technique of tests/test_kernel_resources.py.  The
bounds are those of DESIGN.md 4.6 "Histograms": the pair pass keeps 8192 cells of 64-bit masses in LDS (64 KB: two workgroups per
CU), the 1-D pass 5120 (40 KB: four per CU); the range pass holds 8 columns of running minima and maxima per thread and the pair
pass 16 columns of packed bin indices in registers -- an array that ended up in scratch memory would go out to HBM and back per
position, invisible in every parity test."""
import pytest

from test_kernel_resources import HIPCC, resource_table

KERNELS = ("hist_range_kernel", "hist_setup_kernel", "hist_bin_kernel", "hist_1d_kernel", "hist_pair_kernel")
LDS_BOUND = {"hist_1d_kernel": 40 * 1024, "hist_pair_kernel": 64 * 1024}          # every other kernel: below 1 KB
WAVES_BOUND = {"hist_1d_kernel": 4, "hist_pair_kernel": 2}                        # waves per SIMD; every other kernel: >= 4
# hist_range_kernel and hist_bin_kernel are one text each over the two value sources (csrc/abz_summary.h).  The bounds below are
# the population's; those of the dense-matrix instantiations are in tests/test_columns_kernel_resources.py
TEMPLATES, MATRIX_SOURCE = ("hist_range_kernel", "hist_bin_kernel"), "ColView"


@pytest.mark.skipif(HIPCC is None, reason="needs hipcc")
def test_every_histogram_kernel_runs_without_scratch_and_within_its_lds():
    rows = resource_table("abz_hist.hip")
    assert len(rows) == len(KERNELS) + len(TEMPLATES), sorted(rows)
    for k in KERNELS:
        assert sum(k in name and MATRIX_SOURCE not in name for name in rows) == 1, (k, sorted(rows))
        assert sum(k in name and MATRIX_SOURCE in name for name in rows) == (1 if k in TEMPLATES else 0), (k, sorted(rows))
    for name, r in rows.items():
        if MATRIX_SOURCE in name:
            continue
        k = next(k for k in KERNELS if k in name)
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
        assert r["Dynamic Stack"] == "False", (name, r)
        assert int(r["LDS Size [bytes/block]"]) <= LDS_BOUND.get(k, 1024), (name, r)
        assert int(r["Occupancy [waves/SIMD]"]) >= WAVES_BOUND.get(k, 4), (name, r)
        assert int(r["VGPRs"]) <= 64, (name, r)                      # the bound DESIGN.md states; 55 at most when written
        print(name, "VGPRs", r["VGPRs"], "LDS", r["LDS Size [bytes/block]"], "waves/SIMD", r["Occupancy [waves/SIMD]"])
