"""Proofs verified in batches (`lmn_verify_many`: k_verify_values, k_verify_trees) on a real MI355X: the checks of
tests/verify_many_checks.py, in process - the fixed matrix, not the random cases (those run on the emulation build)."""
import pytest

import verify_many_checks as vm
from luminair_amd import backend
from luminair_amd.batch import BATCH_LIB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip_lib_path):
    return backend.default_library()


def test_gpu_verify_many_symbol_in_both_libraries(lib, hip_lib_path):
    assert "lmn_verify_many" in backend.EXPORTS
    getattr(lib.lib, "lmn_verify_many")
    getattr(backend.Library(BATCH_LIB).lib, "lmn_verify_many")
    assert lib.lib.lmn_abi_version() == 6


@pytest.mark.parametrize("shape", vm.SHAPES, ids=lambda s: s.name)
def test_gpu_accepted_proof_alone(lib, shape):
    vm.check_accepted_alone(lib, shape)


def test_gpu_accepted_proofs_of_several_claims_in_one_call(lib):
    vm.check_accepted_together(lib)


def test_gpu_300_copies_span_two_chunks(lib):
    vm.check_accepted_300_copies(lib)


@pytest.mark.parametrize("shape", vm.TAMPER_SHAPES, ids=lambda s: s.name)
def test_gpu_tamper_matrix_equals_the_host_verifier(lib, shape):
    vm.check_tamper_reference(lib, shape)   # the reference's own verdicts first: host code
    vm.check_tamper_matrix(lib, shape)


@pytest.mark.parametrize("shape", [vm.SHAPES[0], vm.SHAPES[4]], ids=lambda s: s.name)
def test_gpu_front_failures_are_decided_on_the_host(lib, shape):
    vm.check_front_failures(lib, shape)


def test_gpu_mixed_call_and_the_bucket_cap(lib):
    vm.check_mixed_call(lib)


def test_gpu_refusals_leave_the_context_usable(lib):
    vm.check_refusals(lib)


def test_gpu_sharded_context_is_refused(lib):
    vm.check_sharded_context_refused(lib)


def test_gpu_batch_library_outside_any_batch(hip_lib_path):
    vm.check_batch_library(BATCH_LIB)


def test_gpu_python_entry_points(lib):
    vm.check_python_entry_points(lib)
