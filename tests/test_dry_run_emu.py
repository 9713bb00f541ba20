"""The device dry run (`lmn_eval_*`, `lmn_tensor_range`, `DeviceGraph.gen_circuit_settings(device=True)`) on the emulation
build (tests/emu: the same HIP sources compiled for the CPU); cases and references in tests/dry_run_checks.py.  The GPU
counterpart is tests/test_gpu_dry_run.py."""
import os
import subprocess

import pytest

import dry_run_checks as dr
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
def emu_lib(emu_so):
    return backend.Library(emu_so)


@pytest.fixture(scope="module")
def emu_ctx(emu_lib):
    ctx = backend.Context(0, None, emu_lib)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("kind", dr.ELEMENTWISE)
def test_element_counts_and_extreme_positions(emu_ctx, kind):
    dr.check_counts(emu_ctx, kind)


def test_range_cases(emu_ctx):
    dr.check_range_cases(emu_ctx)


def test_tensor_range(emu_ctx):
    dr.check_tensor_range_counts(emu_ctx)


@pytest.mark.parametrize("kind", dr.ELEMENTWISE)
def test_views(emu_ctx, kind):
    dr.check_views(emu_ctx, kind)


@pytest.mark.parametrize("kind", sorted(dr.REFUSED_OPERANDS))
def test_refusals(emu_ctx, kind):
    dr.check_refusals(emu_ctx, kind)


def test_counter_accumulates(emu_ctx):
    dr.check_counter_accumulates(emu_ctx)


def test_lut(emu_ctx):
    dr.check_lut_counts(emu_ctx)


def test_reduce_split(emu_lib):
    dr.check_reduce_split(emu_lib)


@pytest.mark.parametrize("maximum", (False, True), ids=("sum", "max"))
@pytest.mark.parametrize("shape", dr.REDUCE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_reduce(emu_ctx, shape, maximum):
    dr.check_reduce_shape(emu_ctx, shape, maximum)


def test_argument_refusals(emu_ctx):
    dr.check_argument_refusals(emu_ctx)


def test_scenario_graphs(emu_lib):
    dr.check_scenario_graphs(emu_lib)


def test_lut_range_comes_from_the_buffer_not_the_view(emu_ctx):
    dr.check_view_not_buffer(emu_ctx)


def test_tie_input_follows_the_lut_columns(emu_ctx):
    dr.check_tie_graph(emu_ctx)


def test_full_mirror(emu_lib):
    dr.check_full_mirror(emu_lib)


def test_refused_graph(emu_ctx):
    dr.check_refused_graph(emu_ctx)


def test_exports_and_rust_bindings(emu_lib, root):
    dr.check_exports(emu_lib)
    rust = open(os.path.join(root, "bindings", "rust", "luminair-hip-sys", "src", "lib.rs")).read()
    header = open(os.path.join(root, "include", "luminair_hip.h")).read()
    for name in dr.NEW_EXPORTS:
        assert "pub fn %s(" % name in rust and "%s(" % name in header, name
