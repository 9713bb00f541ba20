"""The trace-check kernels in gfx950 code (cross-compiled, no GPU needed): every instantiation of k_trace_check and
k_trace_check_collect exists, keeps its row in registers (no scratch, no spills), stays inside 64 KB of LDS - the
row-major forms stage 256 rows at an odd pitch, the column-major ones need none beyond LessThan's range-check sums - and
claims tuple slots with a 64-bit compare-and-swap."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "luminair_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
N_COLS = {0: 15, 1: 16, 2: 13, 3: 12, 4: 1, 5: 14, 6: 15, 7: 13, 8: 16, 9: 12, 10: 1, 11: 12, 12: 1, 13: 22, 14: 1, 15: 7, 16: 11}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_trace_check") / "kernels_trace.s"
    src = os.path.join(CSRC, "kernels_trace.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S", src,
                        "-o", str(out)], capture_output=True, text=True, cwd=CSRC, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = out.read_text()
    ks = {}
    for doc in asm.split("  - .agpr_count:")[1:]:          # one metadata record per kernel
        name = re.search(r"\.name:\s+(\S+)", doc).group(1)
        if "k_trace_check" not in name:
            continue
        f = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, doc).group(1))   # noqa: E731
        start = asm.find("\n%s:" % name)
        m = re.search(r"k_trace_checkILi(\d+)ELb([01])E", name)
        key = ("collect",) if "k_trace_check_collect" in name else (int(m.group(1)), bool(int(m.group(2))))
        ks[key] = dict(name=name, lds=f("group_segment_fixed_size"), scratch=f("private_segment_fixed_size"),
                       sgpr_spill=f("sgpr_spill_count"), vgpr_spill=f("vgpr_spill_count"), vgpr=f("vgpr_count"),
                       body=asm[start:asm.find("s_endpgm", start)])
    return ks


def test_both_kernels_exist_for_every_kind_and_layout(kernels):
    assert ("collect",) in kernels
    assert sorted(k for k in kernels if k != ("collect",)) == sorted((kind, cols) for kind in N_COLS for cols in (False, True))


def test_no_scratch_no_spills(kernels):
    for key, k in kernels.items():
        assert k["scratch"] == 0 and k["sgpr_spill"] == 0 and k["vgpr_spill"] == 0, (key, k["name"])
        assert "scratch_" not in k["body"], key


def test_lds_within_64_kb_and_as_the_layout_implies(kernels):
    for key, k in kernels.items():
        assert k["lds"] <= 64 * 1024, (key, k["lds"])
        if key == ("collect",):
            continue
        kind, cols = key
        tile = 0 if cols else 256 * (N_COLS[kind] | 1) * 4      # 256 rows at an odd word pitch
        sums = 2 * 256 * 8 if kind == 13 else 0                 # LessThan: the 256 range-check keys, sum and first mention
        assert tile + sums <= k["lds"] <= tile + sums + 64, (key, k["lds"])


def test_tuple_slots_are_claimed_by_a_64_bit_compare_and_swap(kernels):
    for key, k in kernels.items():
        if key == ("collect",):
            continue
        cas = re.findall(r"\b(?:global|flat|buffer)_atomic_cmpswap_x2\b", k["body"])
        assert cas, key
    assert not re.findall(r"atomic_cmpswap", kernels[("collect",)]["body"])


def test_row_major_forms_read_their_rows_from_lds_and_column_major_forms_use_none(kernels):
    """the row-major forms stage the workgroup's words in LDS and every lane reads its row from there; the column-major
    forms read column words directly and touch LDS only for LessThan's range-check sums"""
    for (kind, cols), k in ((key, k) for key, k in kernels.items() if key != ("collect",)):
        lds_reads = re.findall(r"\bds_(?:read|load)_", k["body"])
        lds_writes = re.findall(r"\bds_(?:write|store)_", k["body"])
        if not cols:
            assert lds_reads and lds_writes, kind
        elif kind != 13:
            assert not lds_reads and not lds_writes, kind
