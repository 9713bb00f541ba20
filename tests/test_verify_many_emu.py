"""Proofs verified in batches (`lmn_verify_many`) on the TEST-ONLY emulation build: the front / back split of the host
verifier, the stager, k_verify_values and k_verify_trees with lanes run as fibres, and every refusal.  The checks are in
tests/verify_many_checks.py; tests/test_gpu_verify_many.py runs them on the MI355X (all but the random cases)."""
import os
import subprocess

import pytest

import verify_many_checks as vm
from luminair_amd import backend


@pytest.fixture(scope="module")
def emu_lib(root):
    so = os.path.join(root, "tests", "emu", "libluminair_emu.so")
    srcs = [os.path.join(root, "luminair_amd", "csrc", f) for f in os.listdir(os.path.join(root, "luminair_amd", "csrc"))
            if f.endswith((".hip", ".cpp", ".h"))] + [os.path.join(root, "tests", "emu", "emu_runtime.cpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run([os.path.join(root, "tests", "emu", "build_emu.sh")], check=True, capture_output=True)
    return backend.Library(so)


def test_verify_many_symbol_is_exported_and_bound(emu_lib):
    assert "lmn_verify_many" in backend.EXPORTS
    getattr(emu_lib.lib, "lmn_verify_many")
    assert backend.API_VERSION == 6 and emu_lib.lib.lmn_abi_version() == 6


def test_verify_many_symbol_in_the_batch_library():
    from test_batch_emu import _build
    getattr(backend.Library(_build()).lib, "lmn_verify_many")


@pytest.mark.parametrize("shape", vm.SHAPES, ids=lambda s: s.name)
def test_accepted_proof_alone(emu_lib, shape):
    vm.check_accepted_alone(emu_lib, shape)


def test_accepted_proofs_of_several_claims_in_one_call(emu_lib):
    vm.check_accepted_together(emu_lib)


def test_300_copies_span_two_chunks(emu_lib):
    vm.check_accepted_300_copies(emu_lib)


@pytest.mark.parametrize("shape", vm.TAMPER_SHAPES, ids=lambda s: s.name)
def test_reference_rejects_every_tampered_proof(emu_lib, shape):
    vm.check_tamper_reference(emu_lib, shape)


@pytest.mark.parametrize("shape", vm.TAMPER_SHAPES, ids=lambda s: s.name)
def test_tamper_matrix_equals_the_host_verifier(emu_lib, shape):
    vm.check_tamper_matrix(emu_lib, shape)


@pytest.mark.parametrize("shape", [vm.SHAPES[0], vm.SHAPES[4]], ids=lambda s: s.name)
def test_front_failures_are_decided_on_the_host(emu_lib, shape):
    vm.check_front_failures(emu_lib, shape)


def test_mixed_call_and_the_bucket_cap(emu_lib):
    vm.check_mixed_call(emu_lib)


def test_refusals_leave_the_context_usable(emu_lib):
    vm.check_refusals(emu_lib)


def test_sharded_context_is_refused(emu_lib):
    vm.check_sharded_context_refused(emu_lib)


def test_batch_library_outside_any_batch():
    from test_batch_emu import _build
    vm.check_batch_library(_build())


def test_python_entry_points(emu_lib):
    vm.check_python_entry_points(emu_lib)


def test_fuzzed_proofs_get_the_host_verifiers_verdict(emu_lib):
    vm.check_fuzz(emu_lib)
