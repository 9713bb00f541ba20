"""Float tensors in and out on the emulation build (tests/emu: the same HIP sources compiled for the CPU), against the
references of tests/float_io_checks.py.  The GPU counterpart is tests/test_gpu_float_io.py."""
import os
import subprocess

import pytest

import float_io_checks as fc
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


@pytest.mark.parametrize("code", fc.CODES, ids=[fc.NAME[c] for c in fc.CODES])
def test_float_to_fixed_values(emu_ctx, code):
    fc.check_to_fixed_values(emu_ctx, code)


@pytest.mark.parametrize("code", fc.CODES, ids=[fc.NAME[c] for c in fc.CODES])
def test_fixed_to_float_values(emu_ctx, code):
    fc.check_from_fixed_values(emu_ctx, code)


@pytest.mark.parametrize("code", fc.CODES, ids=[fc.NAME[c] for c in fc.CODES])
def test_shapes_around_block_boundaries(emu_ctx, code):
    fc.check_shapes(emu_ctx, code)


@pytest.mark.parametrize("code", fc.CODES, ids=[fc.NAME[c] for c in fc.CODES])
def test_many_members_and_shared_sources(emu_ctx, code):
    fc.check_many(emu_ctx, code)


def test_argument_errors(emu_ctx):
    fc.check_argument_errors(emu_ctx)


def test_host_mirrors():
    fc.check_host_mirrors()


def test_graph_end_to_end(emu_so):
    fc.check_end_to_end(backend.Library(emu_so))


def test_gen_trace_many_float_feeds(emu_so):
    fc.check_many_end_to_end(backend.Library(emu_so))
