"""The two decommitment kernels in gfx950 code (cross-compiled, no GPU needed): both exist, keep everything in registers
(no scratch, no spills) and need no LDS - a lane copies one hash or one word."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "luminair_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("k_tree_decommit", "k_col_gather")


@pytest.fixture(scope="module")
def decommit_kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_decommit") / "kernels_merkle.s"
    src = os.path.join(CSRC, "kernels_merkle.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S", src,
                        "-o", str(out)], capture_output=True, text=True, cwd=CSRC, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = out.read_text()
    ks = {}
    for doc in asm.split("  - .agpr_count:")[1:]:          # one metadata record per kernel
        name = re.search(r"\.name:\s+(\S+)", doc).group(1)
        short = [k for k in KERNELS if k in name]
        if not short:
            continue
        f = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, doc).group(1))   # noqa: E731
        start = asm.find("\n%s:" % name)
        ks[short[0]] = dict(lds=f("group_segment_fixed_size"), scratch=f("private_segment_fixed_size"),
                            sgpr_spill=f("sgpr_spill_count"), vgpr_spill=f("vgpr_spill_count"), vgpr=f("vgpr_count"),
                            body=asm[start:asm.find("s_endpgm", start)])
    return ks


def test_both_kernels_exist_for_gfx950(decommit_kernels):
    assert sorted(decommit_kernels) == sorted(KERNELS)


def test_no_scratch_no_spills_no_lds(decommit_kernels):
    for name, k in decommit_kernels.items():
        assert k["scratch"] == 0 and k["sgpr_spill"] == 0 and k["vgpr_spill"] == 0, (name, k)
        assert "scratch_" not in k["body"], name
        assert k["lds"] == 0, (name, k["lds"])
        assert k["vgpr"] <= 64, (name, k["vgpr"])


def test_a_hash_moves_as_two_16_byte_loads_and_stores(decommit_kernels):
    body = decommit_kernels["k_tree_decommit"]["body"]
    assert len(re.findall(r"\b(?:global|flat|buffer)_load_dwordx4\b", body)) == 2
    assert len(re.findall(r"\b(?:global|flat|buffer)_store_dwordx4\b", body)) == 2
