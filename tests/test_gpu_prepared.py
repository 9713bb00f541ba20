"""Settings prepared once (`lmn_settings_prepare` and the `*_prepared` prove entries) on the MI355X: the checks of
tests/prepared_checks.py, and BASELINE config 4's own 2^17-row exp2 LUT - the size the feature is for."""
import os
import sys

import pytest

from luminair_amd import backend
from luminair_amd.batch import BATCH_LIB

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prepared_checks as checks          # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip_lib_path):
    return backend.default_library()


@pytest.mark.parametrize("name", list(checks.CASES))
def test_gpu_prepared_proof_equals_lmn_prove(lib, name):
    checks.check_case(lib, name)


@pytest.mark.parametrize("log_blowup", [2, 3])
def test_gpu_prepared_proof_at_other_blowups(lib, log_blowup):
    checks.check_case(lib, "three_sizes_and_range_check", log_blowup)


def test_gpu_prepared_without_lookups_is_the_empty_tree(lib):
    checks.check_no_lookups(lib)


def test_gpu_prepared_config4_lut(lib):
    checks.check_config4(lib)


def test_gpu_prepared_two_pies_in_a_row(lib):
    checks.check_two_pies_in_a_row(lib)


def test_gpu_prepared_shared_by_two_threads(lib):
    checks.check_two_threads(lib)


def test_gpu_prepared_submit_wait_and_destroy_in_between(lib):
    checks.check_submit_wait(lib)


def test_gpu_prepared_survives_arena_growth(lib):
    checks.check_arena_growth(lib, big_rows=1 << 14)


def test_gpu_prepared_does_not_read_the_callers_luts_again(lib):
    checks.check_luts_overwritten(lib)


def test_gpu_prepare_refusals(lib):
    checks.check_prepare_refusals(lib)


def test_gpu_prepared_prove_refusals_leave_the_context_usable(lib):
    import torch
    checks.check_prove_refusals(lib, other_device=1 if torch.cuda.device_count() > 1 else None)


def test_gpu_batch_prepared_equals_lmn_prove_with_fewer_launches_waits_and_transfers(lib):
    checks.check_batch(lib, BATCH_LIB)


def test_gpu_batch_prepared_bad_member_fails_alone(lib):
    checks.check_batch_bad_member(lib, BATCH_LIB)


def test_gpu_prepared_python_layer(lib):
    checks.check_python_layer(lib, BATCH_LIB)
