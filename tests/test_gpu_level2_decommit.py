"""Decommitment on device handles on the MI355X (-m gpu): the checks of tests/level2_decommit_checks.py against the
product library, plus a tree of BASELINE config 2a's trace-tree size with a second column size in it and a gather from
a 2^22-row secure column.  Every check runs in a child process of its own with its own time limit (as
tests/test_gpu_row_stream.py does): a check that hangs ends there, and nothing is tried twice."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

CHECKS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "level2_decommit_checks.py")


def _run(hip_lib_path, check, seconds):
    r = subprocess.run([sys.executable, CHECKS, hip_lib_path, check], capture_output=True, text=True, timeout=seconds)
    assert r.returncode == 0 and ("ok " + check) in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_gpu_decommit_symbols(hip_lib_path):
    from luminair_amd import backend
    lib = backend.Library(hip_lib_path)
    for name in ("lmn_tree_decommit", "lmn_col_gather"):
        getattr(lib.lib, name)


def test_gpu_openings_equal_the_oracle_and_verify(hip_lib_path):
    _run(hip_lib_path, "oracle", 300)


def test_gpu_gather_equals_numpy_indexing(hip_lib_path):
    _run(hip_lib_path, "gather", 120)


def test_gpu_refusals_name_the_argument_and_leave_context_and_tree_usable(hip_lib_path):
    _run(hip_lib_path, "refusals", 120)


def test_gpu_whole_proofs_without_whole_column_downloads(hip_lib_path):
    _run(hip_lib_path, "whole_proof", 300)


def test_gpu_config2a_trace_tree_with_a_second_size(hip_lib_path):
    _run(hip_lib_path, "full_size", 300)


def test_gpu_gather_from_a_2_22_row_secure_column(hip_lib_path):
    _run(hip_lib_path, "big_gather", 180)
