"""Trace reuse on a real MI355X: the sequences of the CPU suite (tests/test_trace_reuse_emu.py) at 2^13 rows and at 2^18 rows,
the first size with a fixed-shape strided pass; the checks are in tests/trace_reuse_checks.py."""
import os

import pytest

import trace_reuse_checks as tr
from luminair_amd import backend

pytestmark = pytest.mark.gpu
SHAPES = tr.SMALL + tr.LARGE
BELOW = [tr.SMALL[0], tr.LARGE[0]]


@pytest.fixture(scope="module")
def env(hip_lib_path):
    from oracle.cbackend import CKernels
    return tr.Env(backend.Library(hip_lib_path), CKernels())


@pytest.fixture(autouse=True)
def _switch_unset(monkeypatch):
    monkeypatch.delenv(tr.SWITCH, raising=False)


@pytest.mark.parametrize("shape", SHAPES, ids=tr.shape_id)
def test_gpu_same_pie_then_new_values(env, shape):
    tr.check_same_pie_then_new_values(env, shape)


@pytest.mark.parametrize("shape", SHAPES, ids=tr.shape_id)
def test_gpu_single_graph_words(env, shape):
    # multiplicities in the first row, the last real row (padding-adjacent where the table is padded) and the row before
    # it; next_idx in the last real row and in the middle (a broken transition: the parent's error)
    n = shape[1]
    tr.check_single_graph_words(env, shape, [(0, 12), (-1, 13), (-2, 14), (-1, 8), (n // 2, 8)])


@pytest.mark.parametrize("shape", SHAPES, ids=tr.shape_id)
def test_gpu_other_shapes_skip_nothing(env, shape):
    tr.check_other_shapes_skip_nothing(env, shape)


@pytest.mark.parametrize("shape", BELOW, ids=tr.shape_id)
def test_gpu_other_arena_users(env, shape):
    tr.check_other_arena_users(env, shape)


@pytest.mark.parametrize("shape", BELOW, ids=tr.shape_id)
def test_gpu_rejected_pies(env, shape):
    tr.check_rejected_pies(env, shape)


@pytest.mark.parametrize("shape", BELOW, ids=tr.shape_id)
def test_gpu_host_rows(env, shape):
    tr.check_host_rows(env, shape)


@pytest.mark.parametrize("log_add", [13, 17])
def test_gpu_two_tables(env, log_add):
    tr.check_two_tables(env, log_add)


def test_gpu_sharded_leaves_counters_at_zero(env):
    tr.check_sharded_leaves_counters_at_zero(env, tr.SMALL[0])


def test_gpu_batch_library_leaves_counters_at_zero(env, hip_lib_path):
    batch = backend.Library(os.path.join(os.path.dirname(hip_lib_path), "libluminair_hip_batch.so"))
    tr.check_batch_library_leaves_counters_at_zero(env, batch, tr.SMALL[0])


@pytest.mark.parametrize("shape", [tr.SMALL[1], tr.LARGE[0]], ids=tr.shape_id)
def test_gpu_back_off(env, shape):
    tr.check_back_off(env, shape)


def test_gpu_back_off_retries(env):
    tr.check_back_off(env, tr.SMALL[1], retry=True)


def test_gpu_switch_off(env):
    tr.check_switch_off(env, tr.SMALL[0])
