"""The many-member trace producers (`lmn_trace_many_*`, `DeviceGraph.gen_trace_many`) on a real MI355X, against the plain
Python-integer reference of tests/trace_checks.py and the single-member producers; once more through the batch library's own
compile of the kernels (behind its trampoline), and end to end through `BatchProver.prove_batch` on device-resident tables."""
import os

import pytest

import trace_many_checks as tm
from luminair_amd import backend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(hip_lib_path):
    c = backend.Context(0, None, backend.Library(hip_lib_path))
    yield c
    c.close()


@pytest.fixture(scope="module")
def batch_lib_path(hip_lib_path):
    return os.path.join(os.path.dirname(hip_lib_path), "libluminair_hip_batch.so")


@pytest.mark.parametrize("kind", tm.KINDS)
def test_gpu_every_kind_at_every_member_count_and_size(ctx, kind):
    tm.check_kind(ctx, kind)


def test_gpu_shared_operands_and_shared_outputs(ctx):
    tm.check_shared(ctx)


def test_gpu_views_with_a_member_stride_larger_than_the_buffer(ctx):
    tm.check_views(ctx)


def test_gpu_row_offsets_in_a_strided_table(ctx):
    tm.check_row_offsets(ctx)


def test_gpu_reduce_carry_in_reads_the_members_own_input(ctx):
    tm.check_reduce(ctx)


def test_gpu_lut_ranges_and_inputs_outside_them(ctx):
    tm.check_lut(ctx)


def test_gpu_contiguous_buffer_rule(ctx):
    tm.check_contiguous(ctx)


def test_gpu_argument_errors_touch_nothing(ctx):
    tm.check_argument_errors(ctx)


def test_gpu_whole_graph_equals_gen_trace_per_member(ctx):
    tm.check_graph(ctx)


def test_gpu_batch_library_produces_the_same_rows(batch_lib_path):
    """libluminair_hip_batch.so compiles kernels_trace.hip a second time, as device functions behind its trampoline"""
    c = backend.Context(0, None, backend.Library(batch_lib_path))
    try:
        for kind in tm.KINDS:
            tm.check_kind(c, kind, members=(3, 65), sizes=(257,))
        tm.check_shared(c)
        tm.check_reduce(c)
        tm.check_lut(c)
        tm.check_contiguous(c)
        tm.check_argument_errors(c)
        tm.check_graph(c)
    finally:
        c.close()


def test_gpu_end_to_end_through_the_batch_prover(batch_lib_path):
    tm.check_batch_end_to_end(batch_lib_path)
