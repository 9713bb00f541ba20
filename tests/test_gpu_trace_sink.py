"""The device producers that fill a row sink (`lmn_rows_append_*`, `DeviceGraph.gen_trace(columns=True)`) on a real MI355X:
the column-form kernels against the plain Python-integer references of tests/trace_checks.py and the row forms of the same
producers, the stream ordering between a context and a sink (a failed table, a reset, a clean table), and the proofs of
sink tables against those of row tables, byte for byte."""
import os

import pytest

import trace_sink_checks as ts
from luminair_amd import backend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip_lib_path):
    return backend.Library(hip_lib_path)


@pytest.fixture(scope="module")
def ctx(lib):
    c = backend.Context(0, None, lib)
    yield c
    c.close()


@pytest.mark.parametrize("kind", ts.KINDS)
def test_gpu_every_kind_at_every_size_and_sink_count(ctx, kind):
    ts.check_kind(ctx, kind)


def test_gpu_views(ctx):
    ts.check_views(ctx)


def test_gpu_two_nodes_and_a_host_chunk_in_one_sink(ctx):
    ts.check_mixed_with_host_push(ctx)


def test_gpu_reduce_groups_across_blocks_and_strided(ctx):
    ts.check_reduce(ctx)


def test_gpu_contiguous_buffer_rule(ctx):
    ts.check_contiguous(ctx)


def test_gpu_lut_ranges_and_an_input_outside_them(ctx):
    ts.check_lut(ctx)


@pytest.mark.parametrize("kind", ts.KINDS)
def test_gpu_refused_elements_fail_the_finish_and_a_reset_clears_them(ctx, kind):
    ts.check_refused(ctx, kind)


def test_gpu_refused_reduce_rows(ctx):
    ts.check_refused_reduce(ctx)


def test_gpu_refusals_touch_nothing(ctx):
    import torch
    ts.check_refusals(ctx, other_device=1 if torch.cuda.device_count() > 1 else None)


def test_gpu_batch_library_exports_and_refuses(hip_lib_path):
    ts.check_batch_library_refuses(backend.Library(os.path.join(os.path.dirname(hip_lib_path), "libluminair_hip_batch.so")))


def test_gpu_compaction(lib):
    ts.check_compaction(lib)


def test_gpu_end_to_end_equals_the_row_form(lib):
    ts.check_end_to_end(lib)


def test_gpu_graph_with_a_refused_element(lib):
    ts.check_graph_refuses(lib)
