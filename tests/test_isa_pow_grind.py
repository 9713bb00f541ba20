"""The proof-of-work grind kernel's gfx950 code (cross-compiled, no GPU needed): no register spills, at most 64 VGPRs so that
8 waves fit a SIMD, and the zero message words of both forms folded out of the compression (blake2s.h b2_half_z)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
VGPR_BUDGET = 64     # 512 VGPRs per SIMD lane / 8 waves


@pytest.fixture(scope="module")
def grind_kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_pow") / "kernels_merkle.s"
    src = os.path.join(ROOT, "luminair_amd", "csrc", "kernels_merkle.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S", src,
                        "-o", str(out)], capture_output=True, text=True, cwd=os.path.dirname(src), timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = out.read_text()
    ks = {}
    for m in re.finditer(r"\.name:\s+(\S*k_pow_grind\S*)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?"
                         r"\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", asm):
        start = asm.find("\n%s:" % m.group(1))
        body = asm[start:asm.find("s_endpgm", start)]
        ks[m.group(1)] = dict(sgpr_spill=int(m.group(2)), vgpr=int(m.group(3)), vgpr_spill=int(m.group(4)), body=body)
    assert len(ks) == 2, sorted(ks)          # k_pow_grind<true> (KAT form) and <false> (hashed forms)
    return ks


def test_grind_kernel_registers(grind_kernels):
    for name, k in grind_kernels.items():
        assert k["sgpr_spill"] == 0 and k["vgpr_spill"] == 0, name
        assert k["vgpr"] <= VGPR_BUDGET, (name, k["vgpr"])


def test_grind_kernel_skips_zero_message_words(grind_kernels):
    """one v_add3_u32 per non-zero message word and round: KAT form 2 words x 10 rounds; hashed forms 10 words x 10
    rounds less the 4 of the first half round, which take the initial state as literals (b2_half_first)"""
    add3 = {name: k["body"].count("v_add3_u32") for name, k in grind_kernels.items()}
    kat, = [n for n in add3 if "ILb1E" in n]
    hashed, = [n for n in add3 if "ILb0E" in n]
    assert add3[kat] == 20 and add3[hashed] == 96, add3
    for k in grind_kernels.values():
        assert k["body"].count("s_setprio") >= 160        # the issue phases of every half round are in place
