"""The row sinks' chunk transpose in gfx950 code (cross-compiled, no GPU needed): the kernel exists, keeps its 8 loads in
registers (no scratch, no spills), and its LDS - none static, CHUNK_ROWS x (ncols | 1) words dynamic at the widest launch
launch_rows_chunk admits - stays within 32 KB, so that two workgroups fit a CU beside each other."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "luminair_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LDS_BUDGET = 32 * 1024


@pytest.fixture(scope="module")
def chunk_kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_rows") / "kernels_trace.s"
    src = os.path.join(CSRC, "kernels_trace.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S", src,
                        "-o", str(out)], capture_output=True, text=True, cwd=CSRC, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = out.read_text()
    ks = {}
    for doc in asm.split("  - .agpr_count:")[1:]:          # one metadata record per kernel
        name = re.search(r"\.name:\s+(\S+)", doc).group(1)
        if "k_rows_chunk" not in name:
            continue
        f = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, doc).group(1))   # noqa: E731
        start = asm.find("\n%s:" % name)
        ks[name] = dict(lds=f("group_segment_fixed_size"), scratch=f("private_segment_fixed_size"),
                        sgpr_spill=f("sgpr_spill_count"), vgpr_spill=f("vgpr_spill_count"), vgpr=f("vgpr_count"),
                        body=asm[start:asm.find("s_endpgm", start)])
    return ks


def _launch_constants():
    text = open(os.path.join(CSRC, "kernels.h")).read()
    rows = int(re.search(r"constexpr int CHUNK_ROWS = (\d+);", text).group(1))
    max_cols = int(re.search(r"constexpr int CHUNK_MAX_COLS = (\d+);", text).group(1))
    return rows, max_cols


def test_chunk_kernel_exists_for_gfx950(chunk_kernels):
    assert len(chunk_kernels) == 1, sorted(chunk_kernels)


def test_chunk_kernel_uses_no_scratch(chunk_kernels):
    for name, k in chunk_kernels.items():
        assert k["scratch"] == 0 and k["sgpr_spill"] == 0 and k["vgpr_spill"] == 0, (name, k["scratch"])
        assert "scratch_" not in k["body"], name
        assert k["vgpr"] <= 128, (name, k["vgpr"])          # 256 lanes x 2 workgroups per CU fit the register file many times


def test_two_workgroups_fit_a_cu_at_the_widest_launch(chunk_kernels):
    rows, max_cols = _launch_constants()
    dynamic = rows * (max_cols | 1) * 4                     # launch_rows_chunk's smem at ncols = CHUNK_MAX_COLS
    for name, k in chunk_kernels.items():
        assert k["lds"] + dynamic <= LDS_BUDGET, (name, k["lds"], dynamic)
    # and the widest component of the protocol is inside what the launch admits
    spec = open(os.path.join(CSRC, "constraints.h")).read()       # kSpecs: the table of the components' shapes
    widest = max(int(m) for m in re.findall(r"\{LMN_KIND_\w+, (\d+),", spec))
    assert widest <= max_cols, (widest, max_cols)


def test_chunk_kernel_keeps_eight_loads_in_flight(chunk_kernels):
    """the 8 loads of a batch are issued before the first s_waitcnt that waits for any of them"""
    for name, k in chunk_kernels.items():
        loads = [m.start() for m in re.finditer(r"\n\s+(global_load_dword|buffer_load_dword|flat_load_dword)\b", k["body"])]
        assert len(loads) >= 8, (name, len(loads))
        best = 0
        for i in range(len(loads) - 7):
            if "s_waitcnt vmcnt" not in k["body"][loads[i]:loads[i + 7]]:
                best = 8
                break
        assert best == 8, name
