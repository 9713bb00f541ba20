"""The close of the FRI transcript on the device (`lmn_col_fri_close`, and `lmn_prove` from LMN_POW_DEVICE_MIN_BITS on) through
the TEST-ONLY emulation build (tests/emu: the same HIP sources compiled for the CPU, one fiber per GPU thread): the checks of
tests/fri_close_checks.py against the oracle, the library's host grind loop and the host close.  The same checks on the
MI355X: tests/test_gpu_fri_close.py."""
import os
import subprocess

import pytest

import fri_close_checks as fc
from luminair_amd import backend


def _built(root, so, *build_args):
    csrc = os.path.join(root, "luminair_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".cpp", ".h"))]
    srcs += [os.path.join(root, "tests", "emu", f) for f in ("emu_runtime.cpp", "build_emu.sh")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        r = subprocess.run([os.path.join(root, "tests", "emu", "build_emu.sh"), *build_args], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return so


@pytest.fixture(scope="module")
def emu_lib(root):
    return backend.Library(_built(root, os.path.join(root, "tests", "emu", "libluminair_emu.so")))


@pytest.fixture(scope="module")
def ctxs(emu_lib):
    c = fc.Contexts(emu_lib)
    yield c
    c.close()


def test_line_evaluate_round_trip():
    fc.check_line_evaluate_round_trip()


@pytest.mark.parametrize("cls", fc.CLASSES)
@pytest.mark.parametrize("shape", fc.SHAPES, ids=lambda s: "ll%d-lb%d" % s)
def test_shape_and_value_class(ctxs, shape, cls):
    fc.check_shape_and_class(ctxs, shape, cls)


@pytest.mark.parametrize("pow_bits", [0, 1, 5, 12, 16])
@pytest.mark.parametrize("variant", fc.FORMS, ids=["kat", "hashed", "prefixed"])
def test_grind(ctxs, emu_lib, variant, pow_bits):
    """every proof-of-work form; at 16 bits one nonce inside the queued windows and one beyond them (the fallback)"""
    fc.check_grind(ctxs, emu_lib, variant, pow_bits)


@pytest.mark.parametrize("u32_counter", [False, True], ids=["ctr-u64", "ctr-u32"])
@pytest.mark.parametrize("n_queries", fc.N_QUERIES)
def test_draws(ctxs, n_queries, u32_counter):
    fc.check_draws(ctxs, n_queries, u32_counter)


def test_refusals_leave_context_and_handles_usable(ctxs):
    fc.check_refusals(ctxs)


def test_sharded_context_is_refused(ctxs):
    fc.check_sharded_context_refused(ctxs)


def test_batch_library_outside_any_batch(root):
    fc.check_batch_library(_built(root, os.path.join(root, "tests", "emu", "libluminair_emu_batch.so"), "batch"))


@pytest.mark.parametrize("case", fc.PROOF_CASES, ids=lambda c: c.id)
def test_proof_bytes_equal_host_close(emu_lib, case):
    fc.check_proof_case(emu_lib, case)


def test_proofs_with_and_without_fallback(emu_lib):
    fc.check_fallback_occurs_and_not(emu_lib)


def test_default_path_untouched(emu_lib):
    fc.check_default_path_untouched(emu_lib)


def test_error_precedence(emu_lib):
    fc.check_error_precedence(emu_lib)
