"""Float tensors in and out on a real MI355X, against the references of tests/float_io_checks.py: the value and shape
edges, the graph end to end - once more fed from torch device tensors produced on torch's stream just before the call -
read_float(device=True), and the value edges through the batch library's own compile of the kernels."""
import os

import pytest

import float_io_checks as fc
from luminair_amd import backend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(hip_lib_path):
    c = backend.Context(0, None, backend.Library(hip_lib_path))
    yield c
    c.close()


@pytest.mark.parametrize("code", fc.CODES, ids=[fc.NAME[c] for c in fc.CODES])
def test_gpu_float_to_fixed_values(ctx, code):
    fc.check_to_fixed_values(ctx, code)


@pytest.mark.parametrize("code", fc.CODES, ids=[fc.NAME[c] for c in fc.CODES])
def test_gpu_fixed_to_float_values(ctx, code):
    fc.check_from_fixed_values(ctx, code)


@pytest.mark.parametrize("code", fc.CODES, ids=[fc.NAME[c] for c in fc.CODES])
def test_gpu_shapes_around_block_boundaries(ctx, code):
    fc.check_shapes(ctx, code)


@pytest.mark.parametrize("code", fc.CODES, ids=[fc.NAME[c] for c in fc.CODES])
def test_gpu_many_members_and_shared_sources(ctx, code):
    fc.check_many(ctx, code)


def test_gpu_argument_errors(ctx):
    fc.check_argument_errors(ctx)


def test_gpu_graph_end_to_end(hip_lib_path):
    fc.check_end_to_end(backend.Library(hip_lib_path))


def test_gpu_gen_trace_many_float_feeds(hip_lib_path):
    fc.check_many_end_to_end(backend.Library(hip_lib_path))


def _produced_on_device(t):
    """the tensor as the result of work enqueued on torch's current stream (x * 2 * 0.5 is exact for every finite value of
    the graphs' moderate magnitudes, and keeps a NaN a NaN)"""
    return (t.to("cuda:0") * 2.0) * 0.5


def test_gpu_graph_from_torch_device_tensors(hip_lib_path):
    fc.check_end_to_end(backend.Library(hip_lib_path), to_device=_produced_on_device)


def test_gpu_gen_trace_many_from_torch_device_tensors(hip_lib_path):
    fc.check_many_end_to_end(backend.Library(hip_lib_path), to_device=_produced_on_device)


def test_gpu_read_float_into_a_torch_tensor(hip_lib_path):
    fc.check_read_float_device(backend.Library(hip_lib_path))


def test_gpu_batch_library_value_edges(hip_lib_path):
    """libluminair_hip_batch.so compiles kernels_trace.hip a second time and exports all five entry points"""
    lib = backend.Library(os.path.join(os.path.dirname(hip_lib_path), "libluminair_hip_batch.so"))
    c = backend.Context(0, None, lib)
    try:
        for code in fc.CODES:
            fc.check_to_fixed_values(c, code, with_sink=False)
            fc.check_from_fixed_values(c, code)
        fc.check_argument_errors(c, with_sink=False)
        fc.check_batch_library_sink_refuses(c)
    finally:
        c.close()
