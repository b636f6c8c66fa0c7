"""Compile-time resources of the posterior-sample kernels (csrc/abz_sample.hip), by the technique of tests/test_kernel_resources.py.
The bounds are those of DESIGN.md 4.6 "Posterior sample": nothing in scratch (a staged row that ended up there would go out to HBM
and back per sampled row, invisible in every parity test), no dynamic stack, at most 16 KB of LDS, registers for at least four
wavefronts per SIMD, and per kernel the VGPR count the compiler reported when the kernel was written plus a margin of 8."""
import pytest

from test_kernel_resources import HIPCC, resource_table

# VGPRs reported when written: count 26, setup 5, search 14, gather 26
VGPR_BOUND = {"sample_count_kernel": 34, "sample_setup_kernel": 13, "sample_search_kernel": 22, "sample_gather_kernel": 34}


@pytest.mark.skipif(HIPCC is None, reason="needs hipcc")
def test_every_sample_kernel_runs_without_scratch_and_fills_the_simd():
    rows = resource_table("abz_sample.hip")
    assert len(rows) == len(VGPR_BOUND), sorted(rows)
    for k in VGPR_BOUND:
        assert sum(k in name for name in rows) == 1, (k, sorted(rows))
    for name, r in rows.items():
        k = next(k for k in VGPR_BOUND if k in name)
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
        assert r["Dynamic Stack"] == "False", (name, r)
        assert int(r["LDS Size [bytes/block]"]) <= 16 * 1024, (name, r)
        assert int(r["Occupancy [waves/SIMD]"]) >= 4, (name, r)
        assert int(r["VGPRs"]) <= VGPR_BOUND[k], (name, r)
        print(name, "VGPRs", r["VGPRs"], "LDS", r["LDS Size [bytes/block]"], "waves/SIMD", r["Occupancy [waves/SIMD]"])
