"""The batch-inverse kernels' gfx950 code (k_batch_inverse_m / k_batch_inverse_q of kernels_trace.hip; cross-compiled, no
GPU needed): no scratch, no spills, and a register count inside the occupancy tier their E was measured at.

The tier is 96 VGPRs (512 per SIMD lane / 5 waves): BATCH_INV_E_M31 = 16 and BATCH_INV_E_QM31 = 8 were chosen by the sweep of
tools/field_ops_rate.py (profiles/field_ops_rate.json, docs/HISTORY.md), where the kernels had 67 and 83 VGPRs and were the
fastest pair at 2^24 and 2^26 rows although E = 8 / 4 (35 and 43 VGPRs) runs 8 waves.  Every figure of the chosen build was
taken at 5 waves per SIMD: a change that pushes either kernel past 96 leaves that regime (4 waves at 128) and wants the sweep
repeated, not this bound raised."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
VGPR_TIER = 96


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_field_ops") / "kernels_trace.s"
    src = os.path.join(ROOT, "luminair_amd", "csrc", "kernels_trace.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S", src,
                        "-o", str(out)], capture_output=True, text=True, cwd=os.path.dirname(src), timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = out.read_text()
    ks = {}
    for m in re.finditer(r"\.name:\s+(\S*k_batch_inverse_[mq]\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                         r"\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?"
                         r"\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", asm):
        ks[m.group(1)] = dict(scratch=int(m.group(2)), sgpr_spill=int(m.group(3)), vgpr=int(m.group(4)),
                              vgpr_spill=int(m.group(5)))
    assert len(ks) == 2, sorted(ks)          # one instantiation each: E is a constant, not a switch
    assert any("k_batch_inverse_m" in k for k in ks) and any("k_batch_inverse_q" in k for k in ks), sorted(ks)
    return ks


def test_batch_inverse_kernels_have_no_scratch_and_no_spills(kernels):
    for name, k in kernels.items():
        assert k["scratch"] == 0 and k["sgpr_spill"] == 0 and k["vgpr_spill"] == 0, (name, k)


def test_batch_inverse_kernels_stay_in_their_occupancy_tier(kernels):
    for name, k in kernels.items():
        assert k["vgpr"] <= VGPR_TIER, (name, k["vgpr"])
