"""`Col.batch_inverse` / `Col.batch_inverse_secure` (lmn_col_batch_inverse*, k_batch_inverse_m / _q) through the TEST-ONLY
emulation build (tests/emu): the checks of tests/field_ops_checks.py.  The same checks on the MI355X, plus 2^20 and 2^22
rows: tests/test_gpu_field_ops.py."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from luminair_amd import backend          # noqa: E402
import field_ops_checks as checks         # noqa: E402

EMU = os.path.join(ROOT, "tests", "emu", "libluminair_emu.so")


@pytest.fixture(scope="module")
def emu_lib():
    csrc = os.path.join(ROOT, "luminair_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".cpp", ".h"))]
    srcs += [os.path.join(ROOT, "tests", "emu", f) for f in ("emu_runtime.cpp", "build_emu.sh")]
    if not os.path.exists(EMU) or any(os.path.getmtime(s) > os.path.getmtime(EMU) for s in srcs):
        r = subprocess.run([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return backend.Library(EMU)


@pytest.fixture(scope="module")
def ctx(emu_lib):
    c = backend.Context(0, emu_lib.default_config(), emu_lib)
    yield c
    c.close()


@pytest.mark.parametrize("log", checks.LOGS)
def test_emu_batch_inverse_every_class_and_column_count(ctx, log):
    checks.check_m31_classes(ctx, log)


@pytest.mark.parametrize("log", checks.LOGS)
def test_emu_batch_inverse_one_zero_and_all_zero_but_one(ctx, log):
    checks.check_m31_one_zero(ctx, log)


@pytest.mark.parametrize("log", checks.LOGS)
def test_emu_batch_inverse_secure_every_class(ctx, log):
    checks.check_qm31_classes(ctx, log)


@pytest.mark.parametrize("log", checks.LOGS)
def test_emu_batch_inverse_secure_every_coordinate_support(ctx, log):
    checks.check_qm31_subsets(ctx, log)


@pytest.mark.parametrize("log", checks.LOGS)
def test_emu_batch_inverse_secure_one_zero_and_all_zero_but_one(ctx, log):
    checks.check_qm31_one_zero(ctx, log)


@pytest.mark.parametrize("secure", [False, True])
@pytest.mark.parametrize("log", checks.VIEW_LOGS)
def test_emu_batch_inverse_on_views(ctx, log, secure):
    checks.check_views(ctx, log, secure)


def test_emu_batch_inverse_refusals(ctx):
    checks.check_refusals(ctx)
