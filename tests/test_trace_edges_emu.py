"""Value and shape edges of the device trace producers on the emulation build (tests/emu: the same HIP sources
compiled for the CPU), against the plain Python-integer reference of tests/trace_checks.py.  The GPU counterpart is
tests/test_gpu_trace_edges.py."""
import os
import subprocess
import sys

import pytest

import trace_checks as tc
from luminair_amd import backend


@pytest.fixture(scope="module")
def emu_so(root):
    so = os.path.join(root, "tests", "emu", "libluminair_emu.so")
    srcs = [os.path.join(root, "luminair_amd", "csrc", f) for f in os.listdir(os.path.join(root, "luminair_amd", "csrc"))
            if f.endswith((".hip", ".cpp", ".h"))] + [os.path.join(root, "tests", "emu", "emu_runtime.cpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run([os.path.join(root, "tests", "emu", "build_emu.sh")], check=True, capture_output=True)
    return so


@pytest.fixture(scope="module")
def emu_ctx(emu_so):
    ctx = backend.Context(0, None, backend.Library(emu_so))
    yield ctx
    ctx.close()


# a kernel that divides by zero (SIGFPE) or runs its isqrt correction loop ~10^9 times must fail the case, not the suite
_IN_CHILD = ("recip_0", "sqrt_-1")


@pytest.mark.parametrize("name", sorted(tc.NAMED_CASES))
def test_named_value_case(emu_so, emu_ctx, root, name):
    """the inputs on which the producers disagreed with an exact reduction mod P, or did value-dependent work"""
    if name not in _IN_CHILD:
        tc.check_named_case(emu_ctx, name)
        return
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import trace_checks as tc\nfrom luminair_amd import backend\n"
            "tc.check_named_case(backend.Context(0, None, backend.Library(%r)), %r)\nprint('ok')\n"
            % (root, os.path.join(root, "tests"), emu_so, name))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stderr[-3000:])


def test_value_edges(emu_ctx):
    tc.check_value_edges(emu_ctx)


def test_shapes_around_block_boundaries(emu_ctx):
    tc.check_shapes(emu_ctx)


def test_less_than_multiplicities(emu_ctx):
    tc.check_less_than_multiplicities(emu_ctx)


def test_reduce_shapes_and_wrapping_sums(emu_ctx):
    tc.check_reduce_shapes(emu_ctx)


def test_views(emu_ctx):
    tc.check_views(emu_ctx)


def test_contiguous_buffer_rule(emu_ctx):
    tc.check_contiguous(emu_ctx)


def test_lut_range_edges(emu_ctx):
    tc.check_lut_edges(emu_ctx)


def test_row_offset_appends(emu_ctx):
    tc.check_row_offset_appends(emu_ctx)


def test_marked_rows_are_refused_by_prove(emu_so):
    tc.check_marked_rows_refused(backend.Library(emu_so))


def test_edge_graph_end_to_end(emu_so):
    tc.check_edge_graph_end_to_end(backend.Library(emu_so))


def test_host_mirror_refuses_what_the_device_marks(emu_ctx):
    tc.check_host_mirror_refuses(emu_ctx)


def test_synthetic_agrees_with_the_reference():
    tc.check_synthetic_agrees()
