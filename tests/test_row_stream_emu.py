"""Row sinks (`lmn_rows_*`: host trace rows streamed to the device while they are produced) on the TEST-ONLY emulation
build: the chunk kernel's indexing for every chunk border, the sink's host logic, and the proof's path for
LMN_TABLE_COLS_ON_DEVICE tables - byte for byte against `lmn_prove` on the same rows as plain host tables.  The checks
themselves are in tests/row_stream_checks.py; tests/test_gpu_row_stream.py runs them on the MI355X."""
import os
import subprocess

import pytest

import row_stream_checks as rs
from luminair_amd import backend


@pytest.fixture(scope="module")
def emu_lib(root):
    so = os.path.join(root, "tests", "emu", "libluminair_emu.so")
    srcs = [os.path.join(root, "luminair_amd", "csrc", f) for f in os.listdir(os.path.join(root, "luminair_amd", "csrc"))
            if f.endswith((".hip", ".cpp", ".h"))] + [os.path.join(root, "tests", "emu", "emu_runtime.cpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run([os.path.join(root, "tests", "emu", "build_emu.sh")], check=True, capture_output=True)
    return backend.Library(so)


def test_sink_symbols_are_exported_and_bound(emu_lib):
    for name in ("lmn_rows_open", "lmn_rows_push", "lmn_rows_push_pinned", "lmn_rows_sync", "lmn_rows_finish",
                 "lmn_rows_count", "lmn_rows_reset", "lmn_rows_close"):
        assert name in backend.EXPORTS
        getattr(emu_lib.lib, name)
    assert backend.TABLE_COLS_ON_DEVICE == 2 and backend.API_VERSION == 6


def test_proofs_from_sinks_equal_proofs_from_host_rows(emu_lib):
    rs.check_byte_identity(emu_lib)


def test_finished_columns_are_the_padded_transpose(emu_lib):
    rs.check_columns_as_data(emu_lib)


def test_capacity_larger_than_needed_is_compacted(emu_lib):
    rs.check_compaction(emu_lib)


def test_sink_host_and_device_tables_in_one_pie(emu_lib):
    rs.check_mixed_pie(emu_lib)


def test_errors_leave_sink_and_context_usable(emu_lib):
    rs.check_errors(emu_lib)


def test_finished_sink_proved_twice_and_two_pies_in_flight(emu_lib):
    rs.check_reuse_and_pool(emu_lib)


def test_batch_library_refuses_sinks_and_says_so():
    """libluminair_hip_batch.so exports the symbols (one header) and refuses them: no sink opens, and a
    LMN_TABLE_COLS_ON_DEVICE table is turned away by its solo lmn_prove as by lmn_batch_*"""
    import ctypes as C

    import numpy as np

    from test_batch_emu import _build
    lib = backend.Library(_build())
    ctx = backend.Context(0, None, lib)
    h = C.c_void_p()
    assert lib.lib.lmn_rows_open(ctx.handle, 0, 100, C.byref(h)) == backend.ERR_INVALID_ARGUMENT and not h.value
    assert b"batch" in lib.lib.lmn_last_error(None)
    rows = np.zeros((16, 15), dtype=np.uint32)
    arr = (backend.LmnTable * 1)()
    arr[0].kind, arr[0].flags, arr[0].n_rows, arr[0].rows = 0, backend.TABLE_COLS_ON_DEVICE, 16, rows.ctypes.data
    out, out_len = C.POINTER(C.c_uint8)(), C.c_size_t()
    assert lib.lib.lmn_prove(ctx.handle, arr, 1, None, C.byref(out), C.byref(out_len)) == backend.ERR_INVALID_ARGUMENT
    assert b"batch" in lib.lib.lmn_last_error(ctx.handle)
    ctx.close()
