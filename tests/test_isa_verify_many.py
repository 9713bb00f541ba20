"""The two kernels of `lmn_verify_many` in gfx950 code (cross-compiled, no GPU needed), by the code object's metadata
alone: both exist, and neither has a private segment or spills a register - a node's message words and the hash state are
indexed at compile time, so nothing a lane holds lives in scratch memory."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "luminair_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("k_verify_values", "k_verify_trees")


@pytest.fixture(scope="module")
def verify_kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_verify_many") / "kernels_merkle.s"
    src = os.path.join(CSRC, "kernels_merkle.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S", src,
                        "-o", str(out)], capture_output=True, text=True, cwd=CSRC, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    ks = {}
    for doc in out.read_text().split("  - .agpr_count:")[1:]:          # one metadata record per kernel
        name = re.search(r"\.name:\s+(\S+)", doc).group(1)
        hit = [k for k in KERNELS if k in name]
        if not hit:
            continue
        f = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, doc).group(1))   # noqa: E731
        ks.setdefault(hit[0], []).append(dict(name=name, scratch=f("private_segment_fixed_size"), sgpr_spills=f("sgpr_spill_count"),
                                              vgpr_spills=f("vgpr_spill_count"), lds=f("group_segment_fixed_size")))
    return ks


def test_both_kernels_exist_for_gfx950(verify_kernels):
    for k in KERNELS:
        assert len(verify_kernels.get(k, [])) == 1, (k, verify_kernels.get(k))


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_private_segment_and_no_spills(verify_kernels, kernel):
    (k,) = verify_kernels[kernel]
    assert (k["scratch"], k["sgpr_spills"], k["vgpr_spills"]) == (0, 0, 0), k


def test_lds_leaves_room_for_several_workgroups_per_cu(verify_kernels):
    # 160 KiB of LDS per CU: a wave per proof / a workgroup per tree must not be alone on its CU
    for kernel in KERNELS:
        (k,) = verify_kernels[kernel]
        assert 0 < k["lds"] <= 40 * 1024, k
