"""The device dry run (`lmn_eval_*`, `lmn_tensor_range`, `DeviceGraph.gen_circuit_settings(device=True)`) on a real MI355X;
cases and references in tests/dry_run_checks.py, the emulation counterpart is tests/test_dry_run_emu.py."""
import os

import pytest

import dry_run_checks as dr
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


@pytest.mark.parametrize("kind", dr.ELEMENTWISE)
def test_gpu_element_counts_and_extreme_positions(ctx, kind):
    dr.check_counts(ctx, kind)


def test_gpu_range_cases(ctx):
    dr.check_range_cases(ctx)


def test_gpu_tensor_range(ctx):
    dr.check_tensor_range_counts(ctx)


@pytest.mark.parametrize("kind", dr.ELEMENTWISE)
def test_gpu_views(ctx, kind):
    dr.check_views(ctx, kind)


@pytest.mark.parametrize("kind", sorted(dr.REFUSED_OPERANDS))
def test_gpu_refusals(ctx, kind):
    dr.check_refusals(ctx, kind)


def test_gpu_counter_accumulates(ctx):
    dr.check_counter_accumulates(ctx)


def test_gpu_lut(ctx):
    dr.check_lut_counts(ctx)


def test_gpu_reduce_split(lib):
    dr.check_reduce_split(lib)


@pytest.mark.parametrize("maximum", (False, True), ids=("sum", "max"))
@pytest.mark.parametrize("shape", dr.REDUCE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_gpu_reduce(ctx, shape, maximum):
    dr.check_reduce_shape(ctx, shape, maximum)


def test_gpu_argument_refusals(ctx):
    dr.check_argument_refusals(ctx)


def test_gpu_scenario_graphs(lib):
    dr.check_scenario_graphs(lib)


def test_gpu_lut_range_comes_from_the_buffer_not_the_view(ctx):
    dr.check_view_not_buffer(ctx)


def test_gpu_tie_input_follows_the_lut_columns(ctx):
    dr.check_tie_graph(ctx)


def test_gpu_full_mirror(lib):
    dr.check_full_mirror(lib)


def test_gpu_refused_graph(ctx):
    dr.check_refused_graph(ctx)


def test_gpu_batch_library(hip_lib_path):
    """libluminair_hip_batch.so compiles the eval kernels behind the trampoline and exports the solo entry points"""
    blib = backend.Library(os.path.join(os.path.dirname(hip_lib_path), "libluminair_hip_batch.so"))
    dr.check_exports(blib)
    dr.check_exports(backend.Library(hip_lib_path))
    c = backend.Context(0, None, blib)
    try:
        dr.check_refusals(c, dr.RECIP)
        dr.check_views(c, dr.MUL)
        dr.check_reduce_shape(c, (5, 64, 7), False)
        dr.check_reduce_shape(c, (1, 1, 300), True)
        dr.check_view_not_buffer(c)
    finally:
        c.close()
