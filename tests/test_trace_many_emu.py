"""The many-member trace producers (`lmn_trace_many_*`, `DeviceGraph.gen_trace_many`) on the emulation build (tests/emu:
the same HIP sources compiled for the CPU), against the plain Python-integer reference of tests/trace_checks.py and the
single-member producers; the end-to-end case goes through the emulated lock-step batch library.  The GPU counterpart is
tests/test_gpu_trace_many.py."""
import os
import subprocess

import pytest

import trace_many_checks as tm
from luminair_amd import backend


def _srcs(root):
    csrc = os.path.join(root, "luminair_amd", "csrc")
    return [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".cpp", ".h"))] + \
        [os.path.join(root, "tests", "emu", "emu_runtime.cpp")]


@pytest.fixture(scope="module")
def emu_so(root):
    so = os.path.join(root, "tests", "emu", "libluminair_emu.so")
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in _srcs(root)):
        subprocess.run([os.path.join(root, "tests", "emu", "build_emu.sh")], check=True, capture_output=True)
    return so


@pytest.fixture(scope="module")
def emu_batch_so(root):
    so = os.path.join(root, "tests", "emu", "libluminair_emu_batch.so")
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in _srcs(root)):
        subprocess.run([os.path.join(root, "tests", "emu", "build_emu.sh"), "batch"], check=True, capture_output=True)
    return so


@pytest.fixture(scope="module")
def emu_ctx(emu_so):
    ctx = backend.Context(0, None, backend.Library(emu_so))
    yield ctx
    ctx.close()


@pytest.mark.parametrize("kind", tm.KINDS)
def test_every_kind_at_every_member_count_and_size(emu_ctx, kind):
    tm.check_kind(emu_ctx, kind)


def test_shared_operands_and_shared_outputs(emu_ctx):
    tm.check_shared(emu_ctx)


def test_views_with_a_member_stride_larger_than_the_buffer(emu_ctx):
    tm.check_views(emu_ctx)


def test_row_offsets_in_a_strided_table(emu_ctx):
    tm.check_row_offsets(emu_ctx)


def test_reduce_carry_in_reads_the_members_own_input(emu_ctx):
    tm.check_reduce(emu_ctx)


def test_lut_ranges_and_inputs_outside_them(emu_ctx):
    tm.check_lut(emu_ctx)


def test_contiguous_buffer_rule(emu_ctx):
    tm.check_contiguous(emu_ctx)


def test_argument_errors_touch_nothing(emu_ctx):
    tm.check_argument_errors(emu_ctx)


def test_whole_graph_equals_gen_trace_per_member(emu_ctx):
    tm.check_graph(emu_ctx)


def test_feeds_are_checked(emu_ctx):
    tm.check_graph_feeds_are_checked(emu_ctx)


def test_batch_library_produces_the_same_rows(emu_batch_so):
    """the batch library compiles the kernels behind its trampoline: blockIdx.y reaches them through it"""
    ctx = backend.Context(0, None, backend.Library(emu_batch_so))
    try:
        tm.check_kind(ctx, tm.LT, members=(3,), sizes=(257,))
        tm.check_reduce(ctx, shapes=((2, 300, 3),), members=(3,))
        tm.check_lut(ctx, members=(3,), sizes=(257,))
    finally:
        ctx.close()


def test_end_to_end_through_the_batch_prover(emu_batch_so):
    """one emulated library produces and proves.  The emulation runs every lane as a fiber, so the shape is the smallest with
    every part of the path in it: 3 members, one hidden layer (2-4-1) and an Exp2 LUT of 2^13 rows (the first layer's
    arguments stay inside +-3300); the GPU test runs 5 members of 2-8-8-1 over +-8 * 4096."""
    tm.check_batch_end_to_end(emu_batch_so, n_members=3, widths=(2, 4, 1), lut_half_range=3500)
