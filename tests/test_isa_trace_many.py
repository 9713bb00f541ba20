"""The many-member trace kernels' gfx950 code (k_trace_many_elementwise / k_trace_many_reduce / k_trace_many_lut of
kernels_trace.hip; cross-compiled, no GPU needed), read from the code object's metadata: no scratch, and the LDS of the
single forms whose row rules they share.  Their VGPR counts are recorded in docs/HISTORY.md; no bound is asserted on them."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_trace_many") / "kernels_trace.s"
    src = os.path.join(ROOT, "luminair_amd", "csrc", "kernels_trace.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S", src,
                        "-o", str(out)], capture_output=True, text=True, cwd=os.path.dirname(src), timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    ks = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", out.read_text(), re.S):
        f = dict(re.findall(r"\.(\w+):\s+(\S+)", m.group(0)))
        ks[f["name"]] = dict(lds=int(f["group_segment_fixed_size"]), scratch=int(f["private_segment_fixed_size"]),
                             vgpr=int(f["vgpr_count"]), sgpr_spill=int(f["sgpr_spill_count"]),
                             vgpr_spill=int(f["vgpr_spill_count"]))
    return ks


def _pairs(kernels):
    """(many kernel, its single form): the same kernel family and the same template arguments (`ILi13E`, `ILb1E`), which
    follow the name in the mangled symbol; the parameter lists differ"""
    by_key = {}
    for name in kernels:
        m = re.search(r"\d+k_trace_(many_)?(elementwise|reduce|lut)(I[^E]*E)?", name)
        if m:
            by_key[(m.group(1) is not None, m.group(2), m.group(3))] = name
    return [(name, by_key.get((False, fam, targs))) for (many, fam, targs), name in sorted(by_key.items()) if many]


def test_one_many_kernel_per_single_form(kernels):
    pairs = _pairs(kernels)
    assert len(pairs) == 8 + 2 + 1, [p[0] for p in pairs]      # eight elementwise kinds, sum / max, the LUT form
    for many, single in pairs:
        assert single in kernels, (many, single)


def test_many_kernels_use_no_scratch(kernels):
    for many, _ in _pairs(kernels):
        k = kernels[many]
        assert k["scratch"] == 0 and k["sgpr_spill"] == 0 and k["vgpr_spill"] == 0, (many, k)


def test_many_kernels_lds_equals_the_single_forms(kernels):
    for many, single in _pairs(kernels):
        assert kernels[many]["lds"] == kernels[single]["lds"] > 0, (many, kernels[many], kernels[single])


def test_report_vgpr_counts(kernels):
    for many, single in _pairs(kernels):
        print("%-90s vgpr %3d (single form %3d) lds %5d" % (many, kernels[many]["vgpr"], kernels[single]["vgpr"],
                                                          kernels[many]["lds"]))
