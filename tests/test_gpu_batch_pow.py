"""Proof of work on the device in the lock-step batch library (libluminair_hip_batch.so) on the MI355X: the scenarios of
tests/batch_pow_checks.py at pow_bits 16, against the main library's solo context."""
import os
import sys

import pytest

from luminair_amd import backend
from luminair_amd.batch import BATCH_LIB

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_pow_checks as checks         # noqa: E402

pytestmark = pytest.mark.gpu

POW_BITS = 16


@pytest.fixture(scope="module")
def libs(hip_lib_path):
    return BATCH_LIB, backend.default_library()


@pytest.mark.parametrize("variant", [backend.VARIANT_KAT, backend.VARIANT_PINNED])
def test_gpu_batch_device_grind_proofs_equal_solo(libs, variant):
    checks.scenario_byte_equal(libs[0], libs[1], variant, POW_BITS)


def test_gpu_batch_grind_rounds_leave_the_lockstep_counters_alone(libs):
    # (at pow_bits 16 a nonce is 2^16 on average, a round 2^14: four members almost surely differ; the scenario asserts it)
    checks.scenario_rounds_and_lockstep_counts(libs[0], libs[1], POW_BITS, 50)


def test_gpu_batch_bad_member_fails_alone_and_the_others_grind_once(libs):
    checks.scenario_bad_member_fails_alone(libs[0], libs[1], POW_BITS)


def test_gpu_two_batch_groups_grind_at_once(libs):
    checks.scenario_two_groups(libs[0], libs[1], POW_BITS)


def test_gpu_batch_library_context_grinds_on_the_device(libs):
    checks.scenario_context_entry_points(libs[0], libs[1], POW_BITS)
