"""Openings planned on the device (`lmn_positions_*`, `lmn_open_queries`: k_open_plan, k_open_offsets, k_open_fetch; and
`lmn_col_fri_close_keep`) on a real MI355X: the checks of tests/open_queries_checks.py, in process."""
import pytest

import fri_close_checks as fc
import open_queries_checks as oq
from luminair_amd import backend
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


@pytest.mark.parametrize("extra_log", [0, 2], ids=["domain=top", "domain=top+2"])
@pytest.mark.parametrize("si", range(len(oq.SHAPES)), ids=[name for name, _ in oq.SHAPES])
def test_gpu_openings_equal_host_walk_and_oracle(lib, si, extra_log):
    oq.check_opening(lib, si, extra_log)


def test_gpu_many_items_one_plan_one_fetch_one_wait(lib):
    oq.check_many_items(lib)


@pytest.mark.parametrize("u32_counter", [False, True], ids=["ctr-u64", "ctr-u32"])
@pytest.mark.parametrize("n_queries", fc.N_QUERIES)
def test_gpu_fri_close_keep_equals_fri_close(ctxs, n_queries, u32_counter):
    oq.check_keep_draws(ctxs, n_queries, u32_counter)


def test_gpu_fri_close_keep_beyond_the_queued_windows(ctxs):
    oq.check_keep_fallback(ctxs)


def test_gpu_refusals_name_the_argument_and_leave_context_and_handles_usable(lib):
    oq.check_refusals(lib)


def test_gpu_fri_close_keep_refusals(ctxs):
    oq.check_keep_refusals(ctxs)


def test_gpu_sharded_context_is_refused(lib):
    oq.check_sharded_context_refused(lib)


def test_gpu_batch_library_outside_any_batch(hip_lib_path):
    oq.check_batch_library(BATCH_LIB)


# ---- whole proofs under LMN_DEVICE_FRI_CLOSE=1 LMN_DEVICE_DECOMMIT=1
@pytest.mark.parametrize("case", fc.PROOF_CASES, ids=lambda c: c.id)
def test_gpu_proof_bytes_equal_default_path(lib, case):
    oq.check_proof_case(lib, case)


def test_gpu_proofs_with_and_without_fallback(lib):
    oq.check_fallback_seeds(lib)


def test_gpu_prepared_sin_circuit(lib):
    oq.check_prepared_sin(lib)


def test_gpu_switch_is_inert_where_the_close_is(lib):
    oq.check_inert_at_pow_bits_5(lib)


def test_gpu_error_precedence_under_both_switches(lib):
    oq.check_error_precedence(lib)


def test_gpu_batch_library_proof_plans_on_the_host(hip_lib_path):
    oq.check_batch_library_proof(BATCH_LIB)


def test_gpu_2_16_row_add_proof_70_queries(lib):
    oq.check_2_16_rows(lib)


@pytest.mark.parametrize("name", list(oq.MIXED))
def test_gpu_recompute_jobs_come_from_the_device_planner(lib, name, capfd):
    """k_open_recompute on hardware: LMN_MERKLE_SUB=3 makes trees of 2^11 leaves and more drop their register levels"""
    oq.check_recompute_jobs(lib, name, capfd)
