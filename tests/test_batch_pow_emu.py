"""Proof of work on the device in the lock-step batch library, on the CPU: the scenarios of tests/batch_pow_checks.py on
the emulated batch library (`tests/emu/build_emu.sh batch`) at pow_bits 12, against the emulation build's solo context.
The same scenarios on the MI355X: tests/test_gpu_batch_pow.py."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from luminair_amd import backend          # noqa: E402
import batch_pow_checks as checks         # noqa: E402
from test_batch_emu import EMU, _build     # noqa: E402

POW_BITS = 12
# 64-row Add pies config2_add_only(64, seed0 .. seed0 + 3) whose nonces at pow_bits 12 need different numbers of 2^14-nonce
# rounds (the scenario asserts it; 2 % of the pies need a second round): seed 137 has nonce 21336, found by proving seeds
# 0 .. 499 on the host path
ROUNDS_SEED0 = 134


@pytest.fixture(scope="module")
def libs():
    batch_so = _build()
    return batch_so, backend.Library(EMU)


@pytest.mark.parametrize("variant", [backend.VARIANT_KAT, backend.VARIANT_PINNED])
def test_emu_batch_device_grind_proofs_equal_solo(libs, variant):
    checks.scenario_byte_equal(libs[0], libs[1], variant, POW_BITS)


def test_emu_batch_grind_rounds_leave_the_lockstep_counters_alone(libs):
    checks.scenario_rounds_and_lockstep_counts(libs[0], libs[1], POW_BITS, ROUNDS_SEED0)


def test_emu_batch_bad_member_fails_alone_and_the_others_grind_once(libs):
    checks.scenario_bad_member_fails_alone(libs[0], libs[1], POW_BITS)


def test_emu_two_batch_groups_grind_at_once(libs):
    checks.scenario_two_groups(libs[0], libs[1], POW_BITS)


def test_emu_batch_library_context_grinds_on_the_device(libs):
    checks.scenario_context_entry_points(libs[0], libs[1], POW_BITS)
