"""Settings prepared once (`lmn_settings_prepare` and the `*_prepared` prove entries) through the TEST-ONLY emulation build
(tests/emu): the checks of tests/prepared_checks.py; the batch entry runs on the emulated batch library, as
tests/test_batch_emu.py's scenarios do.  The same checks on the MI355X: tests/test_gpu_prepared.py."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from luminair_amd import backend          # noqa: E402
import prepared_checks as checks          # noqa: E402

EMU = os.path.join(ROOT, "tests", "emu", "libluminair_emu.so")
EMU_BATCH = os.path.join(ROOT, "tests", "emu", "libluminair_emu_batch.so")


def _build(so, *args):
    csrc = os.path.join(ROOT, "luminair_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".cpp", ".h"))]
    srcs += [os.path.join(ROOT, "tests", "emu", f) for f in ("emu_runtime.cpp", "build_emu.sh")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        r = subprocess.run([os.path.join(ROOT, "tests", "emu", "build_emu.sh"), *args], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return so


@pytest.fixture(scope="module")
def emu_lib():
    return backend.Library(_build(EMU))


@pytest.fixture(scope="module")
def emu_batch(emu_lib):
    return _build(EMU_BATCH, "batch")


@pytest.mark.parametrize("name", list(checks.CASES))
def test_emu_prepared_proof_equals_lmn_prove(emu_lib, name):
    checks.check_case(emu_lib, name)


@pytest.mark.parametrize("log_blowup", [2, 3])
def test_emu_prepared_proof_at_other_blowups(emu_lib, log_blowup):
    checks.check_case(emu_lib, "three_sizes_and_range_check", log_blowup)


def test_emu_prepared_without_lookups_is_the_empty_tree(emu_lib):
    checks.check_no_lookups(emu_lib)


def test_emu_prepared_two_pies_in_a_row(emu_lib):
    checks.check_two_pies_in_a_row(emu_lib)


def test_emu_prepared_shared_by_two_threads(emu_lib):
    checks.check_two_threads(emu_lib)


def test_emu_prepared_submit_wait_and_destroy_in_between(emu_lib):
    checks.check_submit_wait(emu_lib)


def test_emu_prepared_survives_arena_growth(emu_lib):
    checks.check_arena_growth(emu_lib, big_rows=300)


def test_emu_prepared_does_not_read_the_callers_luts_again(emu_lib):
    checks.check_luts_overwritten(emu_lib)


def test_emu_prepare_refusals(emu_lib):
    checks.check_prepare_refusals(emu_lib)


def test_emu_prepared_prove_refusals_leave_the_context_usable(emu_lib):
    # (the emulation takes any device number; the sharded refusal uses the callback transport)
    checks.check_prove_refusals(emu_lib, other_device=1, sharded=True)


def test_emu_batch_prepared_equals_lmn_prove_with_fewer_launches_waits_and_transfers(emu_lib, emu_batch):
    checks.check_batch(emu_lib, emu_batch)


def test_emu_batch_prepared_bad_member_fails_alone(emu_lib, emu_batch):
    checks.check_batch_bad_member(emu_lib, emu_batch)


def test_emu_prepared_python_layer(emu_lib, emu_batch):
    checks.check_python_layer(emu_lib, emu_batch)
