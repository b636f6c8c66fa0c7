"""Compile-time resources of the weighted-quantile kernels (csrc/abz_wquantile.hip), by the technique of
tests/test_kernel_resources.py.  The digit pass keeps one 256-bin histogram of 64-bit masses per probability of a batch in LDS
(32 KB) and must leave room for several workgroups per CU; the gather and the closing pass hold 16 columns / 16 slots of running
minima and maxima per thread in registers -- an array that ended up in scratch memory would go out to HBM and back per position,
invisible in every parity test."""
import pytest

from test_kernel_resources import HIPCC, resource_table

KERNELS = ("wq_gather_kernel", "wq_targets_kernel", "wq_pass_kernel", "wq_scan_kernel", "wq_close_kernel", "wq_final_kernel")
SOURCES = ("PopSource", "ColView")                 # wq_gather_kernel is one text over the two value sources (csrc/abz_summary.h)


@pytest.mark.skipif(HIPCC is None, reason="needs hipcc")
def test_every_wquantile_kernel_runs_without_scratch_and_fits_the_lds():
    rows = resource_table("abz_wquantile.hip")
    assert len(rows) == len(KERNELS) + len(SOURCES) - 1, sorted(rows)
    for k in KERNELS:
        assert any(k in name for name in rows), (k, sorted(rows))
    for s in SOURCES:
        assert sum("wq_gather_kernel" in name and s in name for name in rows) == 1, (s, sorted(rows))
    for name, r in rows.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs Spill"]) == 0, (name, r)
        assert r["Dynamic Stack"] == "False", (name, r)
        assert int(r["LDS Size [bytes/block]"]) <= 40 * 1024, (name, r)          # four workgroups per CU
        assert int(r["Occupancy [waves/SIMD]"]) >= 3, (name, r)
        print(name, "VGPRs", r["VGPRs"], "LDS", r["LDS Size [bytes/block]"], "waves/SIMD", r["Occupancy [waves/SIMD]"])
