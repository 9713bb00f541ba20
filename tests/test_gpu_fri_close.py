"""The close of the FRI transcript on the device (`lmn_col_fri_close`: k_fri_close, the queued grind windows, k_fri_queries;
and `lmn_prove` from LMN_POW_DEVICE_MIN_BITS on) on a real MI355X: the checks of tests/fri_close_checks.py, and two 2^16-row
proofs against the host close."""
import pytest

import fri_close_checks as fc
from luminair_amd import backend, synthetic as syn
from luminair_amd.batch import BATCH_LIB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip_lib_path):
    return backend.default_library()


@pytest.fixture(scope="module")
def ctxs(lib):
    c = fc.Contexts(lib)
    yield c
    c.close()


@pytest.mark.parametrize("cls", fc.CLASSES)
@pytest.mark.parametrize("shape", fc.SHAPES, ids=lambda s: "ll%d-lb%d" % s)
def test_gpu_shape_and_value_class(ctxs, shape, cls):
    fc.check_shape_and_class(ctxs, shape, cls)


@pytest.mark.parametrize("pow_bits", [0, 1, 5, 12, 16])
@pytest.mark.parametrize("variant", fc.FORMS, ids=["kat", "hashed", "prefixed"])
def test_gpu_grind(ctxs, lib, variant, pow_bits):
    fc.check_grind(ctxs, lib, variant, pow_bits)


@pytest.mark.parametrize("u32_counter", [False, True], ids=["ctr-u64", "ctr-u32"])
@pytest.mark.parametrize("n_queries", fc.N_QUERIES)
def test_gpu_draws(ctxs, n_queries, u32_counter):
    fc.check_draws(ctxs, n_queries, u32_counter)


def test_gpu_refusals_leave_context_and_handles_usable(ctxs):
    fc.check_refusals(ctxs)


def test_gpu_sharded_context_is_refused(ctxs):
    fc.check_sharded_context_refused(ctxs)


def test_gpu_batch_library_outside_any_batch(hip_lib_path):
    fc.check_batch_library(BATCH_LIB)


@pytest.mark.parametrize("case", fc.PROOF_CASES, ids=lambda c: c.id)
def test_gpu_proof_bytes_equal_host_close(lib, case):
    fc.check_proof_case(lib, case)


def test_gpu_proofs_with_and_without_fallback(lib):
    fc.check_fallback_occurs_and_not(lib)


def test_gpu_default_path_untouched(lib):
    fc.check_default_path_untouched(lib)


def test_gpu_error_precedence(lib):
    fc.check_error_precedence(lib)


@pytest.mark.parametrize("pow_bits,n_queries", [(16, 3), (20, 70)], ids=["pow16", "pow20-q70"])
def test_gpu_2_16_row_add_proof(lib, pow_bits, n_queries):
    """default windows: byte-equal to the host close, accepted, one device close"""
    case = fc.ProofCase("2^16 rows", fc.KAT, pow_bits, 0, 1, n_queries)
    tables = [(k, r, len(r)) for k, r in syn.config2_add_only(1 << 16, 5)]
    dev, dc, host, hc = fc.prove_both(lib, case, tables)
    assert dev == host
    lib.verify(dev, case.variant, fc.proof_config(lib, case))
    assert dc[9] == 1 and hc[9] == 0 and hc[8] >= 1, (dc, hc)
