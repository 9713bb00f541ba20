"""The many-digest grind kernel's gfx950 code (k_grind_many; cross-compiled, no GPU needed), held to what
tests/test_isa_pow_grind.py holds the solo kernel to: no spills, no scratch, at most 64 VGPRs, the zero message words
folded out of the compression - and the workgroup-uniform pending index and digest words fetched by scalar loads."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
VGPR_BUDGET = 64     # 512 VGPRs per SIMD lane / 8 waves


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_grind_many") / "kernels_merkle.s"
    src = os.path.join(ROOT, "luminair_amd", "csrc", "kernels_merkle.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S", src,
                        "-o", str(out)], capture_output=True, text=True, cwd=os.path.dirname(src), timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = out.read_text()
    ks = {}
    for m in re.finditer(r"\.name:\s+(\S*k_grind_many\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                         r"\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?"
                         r"\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", asm):
        start = asm.find("\n%s:" % m.group(1))
        body = asm[start:asm.find("s_endpgm", start)]
        ks[m.group(1)] = dict(scratch=int(m.group(2)), sgpr_spill=int(m.group(3)), vgpr=int(m.group(4)),
                              vgpr_spill=int(m.group(5)), body=body)
    assert len(ks) == 2, sorted(ks)          # k_grind_many<true> (KAT form) and <false> (hashed forms)
    return ks


def test_grind_many_kernel_registers(kernels):
    for name, k in kernels.items():
        assert k["sgpr_spill"] == 0 and k["vgpr_spill"] == 0 and k["scratch"] == 0, (name, k["scratch"])
        assert k["vgpr"] <= VGPR_BUDGET, (name, k["vgpr"])


def test_grind_many_kernel_skips_zero_message_words(kernels):
    """as k_pow_grind: one v_add3_u32 per non-zero message word and round, less the 4 of the hashed forms' first half round"""
    add3 = {name: k["body"].count("v_add3_u32") for name, k in kernels.items()}
    kat, = [n for n in add3 if "ILb1E" in n]
    hashed, = [n for n in add3 if "ILb0E" in n]
    assert add3[kat] == 20 and add3[hashed] == 96, add3


def test_grind_many_kernel_reads_its_tables_with_scalar_loads(kernels):
    """pending[blockIdx.y] is one s_load_dword, the digest one s_load_dwordx8; the only vector load is best[idx]
    (pow_best_now: one u64 past the vector L1)"""
    for name, k in kernels.items():
        body = k["body"]
        assert re.search(r"\bs_load_dword\s", body), name
        assert re.search(r"\bs_load_dwordx8\s", body), name
        vector_loads = re.findall(r"\b(?:global|flat|buffer)_load_\w+", body)
        assert vector_loads == ["global_load_dwordx2"], (name, vector_loads)
