"""Compile-time resources of the posterior-summary kernels (csrc/abz_summary.hip), by the technique of
tests/test_kernel_resources.py: hipcc cross-compiles gfx950 without a GPU and reports what every kernel uses.  The two moment
passes keep 64 doubles of terms (first pass) or 4 + 4 centred columns of 8 rows (second pass) per thread in registers: a
register array that ends up in scratch memory would go out to HBM and back per position, invisible in every parity test."""
import pytest

from test_kernel_resources import HIPCC, resource_table

KERNELS = ("sum_first_kernel", "sum_second_kernel", "sum_finish_kernel", "sum_column_kernel")
SOURCES = ("PopSource", "ColView")                 # the two moment passes are one text each over the two value sources (csrc/abz_summary.h)


@pytest.mark.skipif(HIPCC is None, reason="needs hipcc")
def test_every_summary_kernel_runs_without_scratch_or_spills_and_fits_the_lds():
    rows = resource_table("abz_summary.hip")
    assert len(rows) == len(KERNELS) + 2 * (len(SOURCES) - 1), sorted(rows)
    for k in KERNELS:
        assert any(k in name for name in rows), (k, sorted(rows))
    for k in KERNELS[:2]:
        for s in SOURCES:
            assert sum(k in name and s in name for name in rows) == 1, (k, s, sorted(rows))
    for name, r in rows.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
        assert r["Dynamic Stack"] == "False", (name, r)
        assert int(r["LDS Size [bytes/block]"]) <= 160 * 1024, (name, r)
        assert int(r["Occupancy [waves/SIMD]"]) >= 1, (name, r)
        print(name, "VGPRs", r["VGPRs"], "LDS", r["LDS Size [bytes/block]"], "waves/SIMD", r["Occupancy [waves/SIMD]"])
