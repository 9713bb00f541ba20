"""`lmn_trace_check` on the MI355X (-m gpu): the checks of tests/trace_doctor_checks.py against the product library, plus
BASELINE config 2a and config 3 at full size.  Every check runs in a child process of its own with its own time limit (as
tests/test_gpu_level2_decommit.py does): a check that hangs ends there, and nothing is tried twice."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

CHECKS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "trace_doctor_checks.py")


def _run(hip_lib_path, check, seconds, *more):
    r = subprocess.run([sys.executable, CHECKS, hip_lib_path, check, *more], capture_output=True, text=True, timeout=seconds)
    assert r.returncode == 0 and ("ok " + check) in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_gpu_trace_check_symbol(hip_lib_path):
    from luminair_amd import backend
    getattr(backend.Library(hip_lib_path).lib, "lmn_trace_check")


def test_gpu_clean_synthetic_pies_report_ok_prove_and_verify(hip_lib_path):
    _run(hip_lib_path, "clean_synthetic", 300)


def test_gpu_producer_scenarios_report_ok_prove_and_verify(hip_lib_path):
    _run(hip_lib_path, "clean_producers", 300)


def test_gpu_every_slot_both_ways(hip_lib_path):
    _run(hip_lib_path, "slots", 300)


def test_gpu_report_ok_iff_the_proof_is_made_and_accepted(hip_lib_path):
    _run(hip_lib_path, "prover_agreement", 180)


def test_gpu_imbalances_equal_the_dict(hip_lib_path):
    _run(hip_lib_path, "imbalances", 120)


def test_gpu_noncanonical_words(hip_lib_path):
    _run(hip_lib_path, "noncanonical", 120)


def test_gpu_host_rows_device_rows_and_a_finished_sink_agree(hip_lib_path):
    _run(hip_lib_path, "table_forms", 120)


def test_gpu_refusals_use_lmn_proves_codes_and_name_the_table(hip_lib_path):
    _run(hip_lib_path, "refusals", 120)


def test_gpu_hot_keys_of_the_range_check(hip_lib_path):
    _run(hip_lib_path, "hot_keys", 180)


def test_gpu_batch_librarys_solo_path_reports_the_same(hip_lib_path):
    batch = os.path.join(os.path.dirname(hip_lib_path), "libluminair_hip_batch.so")
    assert os.path.exists(batch), "libluminair_hip_batch.so is built by __graft_entry__.build()"
    _run(hip_lib_path, "batch_solo", 180, batch)


def test_gpu_config2a_resident_and_config3_at_full_size(hip_lib_path):
    _run(hip_lib_path, "full_size", 300)
