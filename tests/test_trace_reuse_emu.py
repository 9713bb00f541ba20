"""Trace reuse on the emulation build (tests/emu: the same HIP sources compiled for the CPU) at 2^13 rows, the smallest table
with the three-launch transform; the checks are in tests/trace_reuse_checks.py, the 2^18-row shapes (the fixed-shape strided
pass) and the batch library in tests/test_gpu_trace_reuse.py."""
import os
import subprocess

import pytest

import trace_reuse_checks as tr
from luminair_amd import backend

BELOW, FULL = tr.SMALL


@pytest.fixture(scope="module")
def env(root):
    so = os.path.join(root, "tests", "emu", "libluminair_emu.so")
    srcs = [os.path.join(root, "luminair_amd", "csrc", f) for f in os.listdir(os.path.join(root, "luminair_amd", "csrc"))
            if f.endswith((".hip", ".cpp", ".h"))] + [os.path.join(root, "tests", "emu", "emu_runtime.cpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run([os.path.join(root, "tests", "emu", "build_emu.sh")], check=True, capture_output=True)
    from oracle.cbackend import CKernels
    return tr.Env(backend.Library(so), CKernels())


@pytest.fixture(autouse=True)
def _switch_unset(monkeypatch):
    monkeypatch.delenv(tr.SWITCH, raising=False)


@pytest.mark.parametrize("shape", tr.SMALL, ids=tr.shape_id)
def test_emu_same_pie_then_new_values(env, shape):
    tr.check_same_pie_then_new_values(env, shape)


def test_emu_single_graph_words_padded(env):
    # a multiplicity in the first row, next_idx in the last real row (padding-adjacent)
    tr.check_single_graph_words(env, BELOW, [(0, 12), (-1, 8)])


def test_emu_back_off(env):
    tr.check_back_off(env, FULL)


def test_emu_other_shapes_skip_nothing(env):
    tr.check_other_shapes_skip_nothing(env, BELOW, and_back=False)


def test_emu_other_arena_users(env):
    tr.check_other_arena_users(env, BELOW)


def test_emu_rejected_pies(env):
    tr.check_rejected_pies(env, BELOW)


def test_emu_host_rows(env):
    tr.check_host_rows(env, BELOW)


def test_emu_two_tables(env):
    tr.check_two_tables(env, brief=True)


def test_emu_sharded_leaves_counters_at_zero(env):
    tr.check_sharded_leaves_counters_at_zero(env, BELOW)


def test_emu_switch_off(env):
    tr.check_switch_off(env, BELOW)
