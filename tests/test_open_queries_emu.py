"""Openings planned on the device (`lmn_positions_*`, `lmn_open_queries`, `lmn_col_fri_close_keep`) on the TEST-ONLY
emulation build: k_open_plan's walk, the offset step and the fetch with lanes run as fibres, the host code around them, and
every refusal.  The checks are in tests/open_queries_checks.py; tests/test_gpu_open_queries.py runs them on the MI355X."""
import os
import subprocess

import pytest

import fri_close_checks as fc
import open_queries_checks as oq
from luminair_amd import backend


@pytest.fixture(scope="module")
def emu_lib(root):
    so = os.path.join(root, "tests", "emu", "libluminair_emu.so")
    srcs = [os.path.join(root, "luminair_amd", "csrc", f) for f in os.listdir(os.path.join(root, "luminair_amd", "csrc"))
            if f.endswith((".hip", ".cpp", ".h"))] + [os.path.join(root, "tests", "emu", "emu_runtime.cpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run([os.path.join(root, "tests", "emu", "build_emu.sh")], check=True, capture_output=True)
    return backend.Library(so)


@pytest.fixture(scope="module")
def ctxs(emu_lib):
    c = fc.Contexts(emu_lib)
    yield c
    c.close()


def test_open_queries_symbols_are_exported_and_bound(emu_lib):
    for name in ("lmn_positions_from_cpu", "lmn_positions_to_cpu", "lmn_positions_log_domain", "lmn_positions_free",
                 "lmn_col_fri_close_keep", "lmn_open_queries"):
        assert name in backend.EXPORTS
        getattr(emu_lib.lib, name)
    assert backend.API_VERSION == 6 and emu_lib.lib.lmn_abi_version() == 6


@pytest.mark.parametrize("extra_log", [0, 2], ids=["domain=top", "domain=top+2"])
@pytest.mark.parametrize("si", range(len(oq.SHAPES)), ids=[name for name, _ in oq.SHAPES])
def test_openings_equal_host_walk_and_oracle(emu_lib, si, extra_log):
    oq.check_opening(emu_lib, si, extra_log)


def test_many_items_one_plan_one_fetch_one_wait(emu_lib):
    oq.check_many_items(emu_lib)


@pytest.mark.parametrize("u32_counter", [False, True], ids=["ctr-u64", "ctr-u32"])
@pytest.mark.parametrize("n_queries", fc.N_QUERIES)
def test_fri_close_keep_equals_fri_close(ctxs, n_queries, u32_counter):
    oq.check_keep_draws(ctxs, n_queries, u32_counter)


def test_fri_close_keep_beyond_the_queued_windows(ctxs):
    oq.check_keep_fallback(ctxs)


def test_refusals_name_the_argument_and_leave_context_and_handles_usable(emu_lib):
    oq.check_refusals(emu_lib)


def test_fri_close_keep_refusals(ctxs):
    oq.check_keep_refusals(ctxs)


def test_sharded_context_is_refused(emu_lib):
    oq.check_sharded_context_refused(emu_lib)


def test_batch_library_outside_any_batch():
    from test_batch_emu import _build
    oq.check_batch_library(_build())


# ---- whole proofs under LMN_DEVICE_FRI_CLOSE=1 LMN_DEVICE_DECOMMIT=1
@pytest.mark.parametrize("case", fc.PROOF_CASES, ids=lambda c: c.id)
def test_proof_bytes_equal_default_path(emu_lib, case):
    oq.check_proof_case(emu_lib, case)


def test_proofs_with_and_without_fallback(emu_lib):
    oq.check_fallback_seeds(emu_lib)


@pytest.mark.parametrize("name", list(oq.MIXED))
def test_recompute_jobs_come_from_the_device_planner(emu_lib, name, capfd):
    oq.check_recompute_jobs(emu_lib, name, capfd)


def test_prepared_sin_circuit(emu_lib):
    oq.check_prepared_sin(emu_lib)


def test_switch_is_inert_where_the_close_is(emu_lib):
    oq.check_inert_at_pow_bits_5(emu_lib)


def test_error_precedence_under_both_switches(emu_lib):
    oq.check_error_precedence(emu_lib)


def test_batch_library_proof_plans_on_the_host():
    from test_batch_emu import _build
    oq.check_batch_library_proof(_build())
