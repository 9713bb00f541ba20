"""The device producers that fill a row sink (`lmn_rows_append_*`, `DeviceGraph.gen_trace(columns=True)`) on the emulation
build (tests/emu: the same HIP sources compiled for the CPU), against the plain Python-integer references of
tests/trace_checks.py and the row forms of the same producers.  The GPU counterpart is tests/test_gpu_trace_sink.py."""
import os
import subprocess

import pytest

import trace_sink_checks as ts
from luminair_amd import backend


def _srcs(root):
    csrc = os.path.join(root, "luminair_amd", "csrc")
    return [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".cpp", ".h"))] + \
        [os.path.join(root, "tests", "emu", "emu_runtime.cpp")]


def _emu(root, name, *args):
    so = os.path.join(root, "tests", "emu", name)
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in _srcs(root)):
        subprocess.run([os.path.join(root, "tests", "emu", "build_emu.sh"), *args], check=True, capture_output=True)
    return so


@pytest.fixture(scope="module")
def emu_lib(root):
    return backend.Library(_emu(root, "libluminair_emu.so"))


@pytest.fixture(scope="module")
def emu_ctx(emu_lib):
    ctx = backend.Context(0, None, emu_lib)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("kind", ts.KINDS)
def test_every_kind_at_every_size_and_sink_count(emu_ctx, kind):
    ts.check_kind(emu_ctx, kind)


def test_views(emu_ctx):
    ts.check_views(emu_ctx)


def test_two_nodes_and_a_host_chunk_in_one_sink(emu_ctx):
    ts.check_mixed_with_host_push(emu_ctx)


def test_reduce_groups_across_blocks_and_strided(emu_ctx):
    ts.check_reduce(emu_ctx)


def test_contiguous_buffer_rule(emu_ctx):
    ts.check_contiguous(emu_ctx)


def test_lut_ranges_and_an_input_outside_them(emu_ctx):
    ts.check_lut(emu_ctx)


@pytest.mark.parametrize("kind", ts.KINDS)
def test_refused_elements_fail_the_finish_and_a_reset_clears_them(emu_ctx, kind):
    ts.check_refused(emu_ctx, kind)


def test_refused_reduce_rows(emu_ctx):
    ts.check_refused_reduce(emu_ctx)


def test_refusals_touch_nothing(emu_ctx):
    ts.check_refusals(emu_ctx, other_device=1)       # the emulation has as many devices as one asks for


def test_batch_library_exports_and_refuses(root):
    ts.check_batch_library_refuses(backend.Library(_emu(root, "libluminair_emu_batch.so", "batch")))


def test_compaction(emu_lib):
    ts.check_compaction(emu_lib)


def test_end_to_end_equals_the_row_form(emu_lib):
    ts.check_end_to_end(emu_lib)


def test_graph_with_a_refused_element(emu_lib):
    ts.check_graph_refuses(emu_lib)
