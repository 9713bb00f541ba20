"""Every layer and launch form of the standalone Merkle commit on a real MI355X, against the references of
tests/merkle_checks.py: the CPU suite's matrix (tests/test_merkle_edges_emu.py) plus what only size reaches - sub = 1, 2, 3
chosen by the planner itself (2^18 .. 2^22 leaves), interior layers of those trees in full, fused runs of 11 and of sub + 8
levels, and the quad-cooperative DPP parents of the LDS climb, which the emulation build replaces.  Modes 3 and 4 of
k_merkle_fused (FRI fold, leaf level under the start level) are reached through the FRI commit loop:
tests/test_gpu_fri_commit.py."""
import numpy as np
import pytest

import merkle_checks as mc
from luminair_amd import backend

pytestmark = pytest.mark.gpu

SMALL_LOG, FUSED_LOG, SUB3_LOG = 7, 11, 20


@pytest.fixture(scope="module")
def ctx(hip_lib_path):
    c = backend.Context(0, None, backend.Library(hip_lib_path))
    yield c
    c.close()


@pytest.mark.parametrize("ncols", mc.LEAF_COUNTS)
def test_gpu_leaf_column_count_small(ctx, ncols):
    """k_merkle_small<1> up to 16 columns, k_merkle_small<0> above"""
    mc.check_leaf_count(ctx, ncols, SMALL_LOG)


@pytest.mark.parametrize("ncols", mc.LEAF_COUNTS)
def test_gpu_leaf_column_count_fused_every_value_class(ctx, ncols):
    """k_merkle_fused<1, 4 | 8 | 12 | 15 | 16> on either side of every NZ threshold, k_merkle_fused<0> with one run above 16
    columns; sub = 0"""
    mc.check_leaf_count(ctx, ncols, FUSED_LOG, mc.VALUE_CLASSES, expect_sub=0)


@pytest.mark.parametrize("ncols", mc.LEAF_COUNTS)
def test_gpu_leaf_column_count_fused_sub3(ctx, ncols):
    """the same leaf forms at 2^20 leaves: sub = 3 by size, every interior layer compared"""
    mc.check_leaf_count(ctx, ncols, SUB3_LOG, ("random", "zero") if ncols <= 17 else ("random",), expect_sub=3)


@pytest.mark.parametrize("nown", mc.OWN_COUNTS)
def test_gpu_children_plus_columns(ctx, nown):
    """k_merkle_small<0> (7 and 6 under 8, 9 under a fused 13), k_merkle_fused<0> with one run (12 and 11 under 13; 18 under
    19 with sub = 1, 20 under 21 with sub = 3)"""
    for top, own in ((8, 7), (8, 6), (13, 12), (13, 11), (13, 9), (19, 18)) + (((21, 20),) if nown <= 17 else ()):
        mc.check_children_plus_columns(ctx, top, own, nown)


@pytest.mark.parametrize("with_children", (False, True))
@pytest.mark.parametrize("log", (6, 11, 18))
def test_gpu_runs(ctx, log, with_children):
    """k_merkle_small<0> / k_merkle_fused<0> with 1, 2, 3, 4 runs, k_merkle_layer for 5 and 9, merged and gapped views; at
    2^18 with sub = 1"""
    mc.check_runs(ctx, log, with_children)


def test_gpu_root_form_layouts(ctx):
    mc.check_root_form_layouts(ctx)


@pytest.mark.parametrize("log", (0, 1, 2, 5, 10, 11, 12, 17, 18, 19, 20, 21, 22))
def test_gpu_single_size(ctx, log):
    """sub = 0 up to 2^17, then 1, 2, 3 by size; 4 columns at 2^22 (a 256 MiB tree over 64 MiB of columns)"""
    expect = ("small<2>", "sub=%d" % max(0, min(3, log - 17))) if log > 10 else ()
    mc.check_single_size(ctx, log, 4 if log == 22 else 1 + log % 5, expect=expect)


@pytest.mark.parametrize("sub", (0, 1, 2))
def test_gpu_single_size_sub_override(ctx, sub, monkeypatch):
    """LMN_MERKLE_SUB at 2^20 (3 by size): the other depths on a tree wide enough for many blocks"""
    monkeypatch.setenv("LMN_MERKLE_SUB", str(sub))
    mc.check_single_size(ctx, 20, 3, sub_env=sub, expect=("sub=%d" % sub,))


@pytest.mark.parametrize("k", (12, 18, 21))
def test_gpu_mixed_sizes_against_the_planner(ctx, k):
    for name, shape, forms in mc.mixed_shapes(k):
        mc.check_mixed(ctx, name, shape, forms)


def test_gpu_pure_inner_fused_level(ctx):
    """k_merkle_fused<2> behind a pointer-table level, with sub = 3 (five handles at 2^21)"""
    for log, sub in ((13, 0), (21, 3)):
        H = mc.Handles()
        try:
            rng = np.random.default_rng(log)
            mc.build_level(ctx, H, mc.random_cols(rng, 5, log), "5 handles", rng)
            mc.check_tree(ctx, H, "five handles at 2^%d" % log, ["layer", "fused<2>", "small<2>", "sub=%d" % sub], root_form=False)
        finally:
            H.free()


@pytest.mark.parametrize("top,cap,sub", [(14, 4, None), (21, 11, None), (22, 11, None), (19, 8, 0)])
def test_gpu_columns_where_a_fused_run_ends(ctx, top, cap, sub, monkeypatch):
    """a run of level - 10 levels from 2^14, of MERKLE_MAX_FUSED = 11 from 2^21 and 2^22, of sub + 8 = 8 from 2^19 with
    LMN_MERKLE_SUB=0: columns at the level where it ends, and at the one after"""
    if sub is not None:
        monkeypatch.setenv("LMN_MERKLE_SUB", str(sub))
    mc.check_fused_run_end(ctx, top, cap, sub_env=sub)


def test_gpu_refusals_leave_the_context_usable(ctx):
    mc.check_refusals_leave_context_usable(ctx)
