"""`Context.grind_many` (lmn_ctx_grind_many, k_grind_many) through the TEST-ONLY emulation build (tests/emu): the checks
of tests/grind_many_checks.py at the sizes the emulation affords (tests/test_pow_grind_emu.py sets the budget).  The same
checks on the MI355X: tests/test_gpu_grind_many.py."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from luminair_amd import backend          # noqa: E402
import grind_many_checks as checks        # noqa: E402

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


@pytest.fixture
def ctx(emu_lib):
    c = backend.Context(0, emu_lib.default_config(), emu_lib)
    yield c
    c.close()


@pytest.fixture
def small_window_ctx(emu_lib, monkeypatch):
    c = checks.small_window_context(emu_lib, monkeypatch)
    yield c
    c.close()


@pytest.mark.parametrize("variant", checks.FORMS)
@pytest.mark.parametrize("n,pow_bits", [(64, 0), (64, 1), (64, 8), (1, 12), (2, 12), (5, 12), (1, 16), (2, 16), (5, 16)])
def test_emu_grind_many_equals_host_loop(emu_lib, ctx, variant, n, pow_bits):
    checks.check_equals_host_loop(emu_lib, ctx, variant, n, pow_bits)


@pytest.mark.parametrize("variant", checks.FORMS)
def test_emu_grind_many_spread_nonces_in_either_order(emu_lib, small_window_ctx, variant):
    checks.check_spread(emu_lib, small_window_ctx, variant)


@pytest.mark.parametrize("variant", checks.FORMS)
def test_emu_grind_many_duplicate_digests(emu_lib, small_window_ctx, variant):
    checks.check_duplicates(emu_lib, small_window_ctx, variant)


def test_emu_grind_many_refusals_and_empty_call(emu_lib, ctx):
    checks.check_refusals(emu_lib, ctx)


def test_emu_grind_many_of_one_agrees_with_grind(emu_lib, small_window_ctx):
    checks.check_agrees_with_single_grind(emu_lib, small_window_ctx)


def test_emu_grind_many_largest_call(emu_lib, ctx):
    checks.check_largest_call(emu_lib, ctx)
