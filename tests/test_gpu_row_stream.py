"""Row sinks on the MI355X (-m gpu): the checks of tests/row_stream_checks.py against the product library - the chunk
kernel reading page-locked host memory over the link, the sink's stream next to the proof stream - plus BASELINE config
2a at full size, a 2^22-row table, and a sink filled while the previous one is being proved on the same context.  Every
check runs in a child process of its own with its own time limit (as the twiddle-lifetime test of tests/test_gpu_parity.py
does): a check that hangs ends there, and nothing is tried twice."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

CHECKS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "row_stream_checks.py")


def _run(hip_lib_path, check, seconds):
    r = subprocess.run([sys.executable, CHECKS, hip_lib_path, check], capture_output=True, text=True, timeout=seconds)
    assert r.returncode == 0 and ("ok " + check) in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_gpu_sink_symbols(hip_lib_path):
    from luminair_amd import backend
    lib = backend.Library(hip_lib_path)
    for name in ("lmn_rows_open", "lmn_rows_push", "lmn_rows_push_pinned", "lmn_rows_sync", "lmn_rows_finish",
                 "lmn_rows_count", "lmn_rows_reset", "lmn_rows_close"):
        getattr(lib.lib, name)


def test_gpu_proofs_from_sinks_equal_proofs_from_host_rows(hip_lib_path):
    _run(hip_lib_path, "byte_identity", 300)


def test_gpu_finished_columns_are_the_padded_transpose(hip_lib_path):
    _run(hip_lib_path, "columns_as_data", 180)


def test_gpu_capacity_larger_than_needed_is_compacted(hip_lib_path):
    _run(hip_lib_path, "compaction", 120)


def test_gpu_errors_leave_sink_and_context_usable(hip_lib_path):
    _run(hip_lib_path, "errors", 120)


def test_gpu_config2a_full_size(hip_lib_path):
    _run(hip_lib_path, "config2a", 300)


def test_gpu_table_of_2_22_rows(hip_lib_path):
    _run(hip_lib_path, "big_table", 300)


def test_gpu_fill_next_sink_while_the_previous_one_is_proved(hip_lib_path):
    _run(hip_lib_path, "overlap", 180)
