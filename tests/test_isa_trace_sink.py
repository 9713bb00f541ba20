"""The column forms of the device producers in gfx950 code (cross-compiled, no GPU needed): the elementwise and the LUT
kernel that fill a row sink's columns (`lmn_rows_append_*`) build a row in registers and store it column by column, so the
code object's metadata shows no LDS (group segment size 0) and no scratch for them."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "luminair_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ELEMENTWISE_KINDS = (0, 1, 2, 7, 8, 13, 15, 16)


@pytest.fixture(scope="module")
def column_kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_sink") / "kernels_trace.s"
    src = os.path.join(CSRC, "kernels_trace.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S", src,
                        "-o", str(out)], capture_output=True, text=True, cwd=CSRC, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    ks = {}
    for doc in out.read_text().split("  - .agpr_count:")[1:]:          # one metadata record per kernel
        name = re.search(r"\.name:\s+(\S+)", doc).group(1)
        if "k_sink_elementwise" not in name and "k_sink_lut" not in name:
            continue
        f = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, doc).group(1))   # noqa: E731
        ks[name] = dict(lds=f("group_segment_fixed_size"), scratch=f("private_segment_fixed_size"))
    return ks


def test_column_kernels_exist_for_gfx950(column_kernels):
    elementwise = [n for n in column_kernels if "k_sink_elementwise" in n]
    lut = [n for n in column_kernels if "k_sink_lut" in n]
    assert len(elementwise) == len(ELEMENTWISE_KINDS), sorted(elementwise)   # one instance per elementwise kind
    assert len(lut) == 1, sorted(lut)


def test_column_kernels_declare_no_lds(column_kernels):
    for name, k in column_kernels.items():
        assert k["lds"] == 0, (name, k["lds"])


def test_column_kernels_use_no_scratch(column_kernels):
    for name, k in column_kernels.items():
        assert k["scratch"] == 0, (name, k["scratch"])
