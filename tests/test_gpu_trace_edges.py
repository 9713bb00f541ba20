"""Value and shape edges of the device trace producers on a real MI355X, against the plain Python-integer reference of
tests/trace_checks.py; the value edges once more through the batch library's own compile of the kernels."""
import os

import pytest

import trace_checks as tc
from luminair_amd import backend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(hip_lib_path):
    c = backend.Context(0, None, backend.Library(hip_lib_path))
    yield c
    c.close()


@pytest.mark.parametrize("name", sorted(tc.NAMED_CASES))
def test_gpu_named_value_case(ctx, name):
    tc.check_named_case(ctx, name)


def test_gpu_value_edges(ctx):
    tc.check_value_edges(ctx)


def test_gpu_shapes_around_block_boundaries(ctx):
    tc.check_shapes(ctx)


def test_gpu_less_than_multiplicities(ctx):
    tc.check_less_than_multiplicities(ctx)


def test_gpu_reduce_shapes_and_wrapping_sums(ctx):
    tc.check_reduce_shapes(ctx)


def test_gpu_views(ctx):
    tc.check_views(ctx)


def test_gpu_contiguous_buffer_rule(ctx):
    tc.check_contiguous(ctx)


def test_gpu_lut_range_edges(ctx):
    tc.check_lut_edges(ctx)


def test_gpu_row_offset_appends(ctx):
    tc.check_row_offset_appends(ctx)


def test_gpu_marked_rows_are_refused_by_prove(hip_lib_path):
    tc.check_marked_rows_refused(backend.Library(hip_lib_path))


def test_gpu_edge_graph_end_to_end(hip_lib_path):
    tc.check_edge_graph_end_to_end(backend.Library(hip_lib_path))


def test_gpu_batch_library_value_edges(hip_lib_path):
    """libluminair_hip_batch.so compiles kernels_trace.hip a second time and exports the whole C ABI"""
    lib = backend.Library(os.path.join(os.path.dirname(hip_lib_path), "libluminair_hip_batch.so"))
    c = backend.Context(0, None, lib)
    try:
        tc.check_value_edges(c)
        for name in sorted(tc.NAMED_CASES):
            tc.check_named_case(c, name)
    finally:
        c.close()
