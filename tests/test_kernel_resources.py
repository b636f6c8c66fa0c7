"""Compile-time resources of the hot kernel (hipcc cross-compiles gfx950 without a GPU).

Round 5 lost 15 % of the d = 32 sweep's fabric traffic budget to ONE 16-byte staging register that the compiler kept in scratch
memory (a conditionally written array: 16 bytes per lane out to HBM and back; profiles/HISTORY.md) -- invisible in every parity test.
This pins what the DESIGN.md numbers rest on: no scratch, no spills, an LDS footprint that leaves room for six workgroups per CU,
registers for five waves per SIMD."""
import functools
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "abcdez.jl_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")


@functools.lru_cache(maxsize=None)
def resource_table(src):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Ibuild",
           "-I../../include", "--cuda-device-only", "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rows, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass", line)
        if not m:
            continue
        t = m.group(1)
        if t.startswith("Function Name:"):
            cur = {}
            rows[t.split(":", 1)[1].strip()] = cur
        elif cur is not None and ":" in t:
            k, v = t.split(":", 1)
            cur[k.strip()] = v.strip()
    return rows


@pytest.mark.skipif(HIPCC is None, reason="needs hipcc")
def test_the_d32_sweep_kernel_has_no_scratch_and_fits_its_occupancy():
    rows = resource_table("abz_smc_swarm.hip")
    # smc_swarm_packed_kernel<ABZ_SIM_MVN = 1, L = 4, C = 8, PLAIN = true>: BASELINE configs[2]
    name = "_Z23smc_swarm_packed_kernelILi1ELi4ELi8ELb1EEv13SmcPackedArgs"
    assert name in rows, sorted(rows)[:5]
    r = rows[name]
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r
    assert int(r["LDS Size [bytes/block]"]) <= 163840 // 6, r          # room for six workgroups per CU
    assert int(r["VGPRs"]) <= 96 and int(r["Occupancy [waves/SIMD]"]) >= 5, r
    # the same body for the other row widths that spread a row over lanes: no scratch either
    for other in ("_Z23smc_swarm_packed_kernelILi1ELi2ELi8ELb1EEv13SmcPackedArgs", "_Z23smc_swarm_packed_kernelILi1ELi8ELi8ELb1EEv13SmcPackedArgs",
                  "_Z23smc_swarm_packed_kernelILi1ELi4ELi4ELb1EEv13SmcPackedArgs"):
        assert int(rows[other]["ScratchSize [bytes/lane]"]) == 0, (other, rows[other])


@pytest.mark.skipif(HIPCC is None, reason="needs hipcc")
def test_the_lotka_volterra_sweep_is_two_launches_that_fill_the_simd():
    """BASELINE configs[3]: the simulator launch (smc_lv_phase2_kernel) keeps five wavefronts per SIMD by registers and five
    workgroups per CU by LDS, nothing in scratch -- late in a run it sustains the part's fp64 FMA rate"""
    rows = resource_table("abz_smc_swarm.hip")
    for plain in ("0", "1"):
        p2 = rows["_Z20smc_lv_phase2_kernelILb%sEEv13SmcPackedArgs10LvHandList" % plain]
        p1 = rows["_Z20smc_lv_phase1_kernelILb%sEEv13SmcPackedArgs10LvHandList" % plain]
        for r in (p1, p2):
            assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0, r
        assert int(p2["Occupancy [waves/SIMD]"]) >= 5 and int(p2["LDS Size [bytes/block]"]) <= 163840 // 5, p2
