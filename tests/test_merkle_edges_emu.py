"""Every layer and launch form of the standalone Merkle commit on the emulation build (tests/emu: the same HIP sources
compiled for the CPU), against the hashlib and oracle references of tests/merkle_checks.py.  The emulation build follows the
GPU's planner, so a tree of less than 2^18 leaves takes sub = 0 unless LMN_MERKLE_SUB says otherwise: sub = 1, 2, 3 are
reached here through that switch at 2^11..2^14, and by size alone (with the 2^17..2^22 trees, the 11-level and the sub + 8
fused runs) in tests/test_gpu_merkle_edges.py.  Modes 3 and 4 of k_merkle_fused (FRI fold, leaf level under the start
level) are reached through the FRI commit loop: tests/test_fri_commit_emu.py."""
import os
import subprocess

import numpy as np
import pytest

import merkle_checks as mc
from luminair_amd import backend

SMALL_LOG, FUSED_LOG = 7, 11


@pytest.fixture(scope="module")
def emu_so(root):
    so = os.path.join(root, "tests", "emu", "libluminair_emu.so")
    srcs = [os.path.join(root, "luminair_amd", "csrc", f) for f in os.listdir(os.path.join(root, "luminair_amd", "csrc"))
            if f.endswith((".hip", ".cpp", ".h"))] + [os.path.join(root, "tests", "emu", "emu_runtime.cpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run([os.path.join(root, "tests", "emu", "build_emu.sh")], check=True, capture_output=True)
    return so


@pytest.fixture(scope="module")
def ctx(emu_so):
    c = backend.Context(0, None, backend.Library(emu_so))
    yield c
    c.close()


@pytest.mark.parametrize("ncols", mc.LEAF_COUNTS)
def test_leaf_column_count_small(ctx, ncols):
    """k_merkle_small<1> up to 16 columns, k_merkle_small<0> (multi-block leaf) above"""
    mc.check_leaf_count(ctx, ncols, SMALL_LOG)


@pytest.mark.parametrize("ncols", mc.LEAF_COUNTS)
def test_leaf_column_count_fused_every_value_class(ctx, ncols):
    """k_merkle_fused<1, 4 | 8 | 12 | 15 | 16> on either side of every NZ threshold, k_merkle_fused<0> with one run from 17
    columns on (leaf blocks of 16, 17, 31, 32, 33, 48, 49 words); sub = 0.  All-zero leaves must hash with their length."""
    mc.check_leaf_count(ctx, ncols, FUSED_LOG, mc.VALUE_CLASSES, expect_sub=0)


@pytest.mark.parametrize("ncols", (4, 5, 16, 17, 33))
def test_leaf_column_count_fused_sub3(ctx, ncols, monkeypatch):
    """the same leaf forms with a register subtree of 2^3 leaves per lane (sub = 3: the merge loop of k_merkle_fused)"""
    monkeypatch.setenv("LMN_MERKLE_SUB", "3")
    mc.check_leaf_count(ctx, ncols, 14, ("random", "zero"), sub_env=3, expect_sub=3)


@pytest.mark.parametrize("nown", mc.OWN_COUNTS)
def test_children_plus_columns(ctx, nown):
    """children plus 1, 2, 15, 16, 17, 32 own columns: the byte counter and the final flag of merkle_hash_from.
    k_merkle_small<0> (levels 7, 6 under 8; level 9 under a fused 13) and k_merkle_fused<0> with one run (levels 11 and 12
    under 13: directly below, and with one empty level between)"""
    for top, own in ((8, 7), (8, 6), (13, 12), (13, 11), (13, 9)):
        mc.check_children_plus_columns(ctx, top, own, nown)


@pytest.mark.parametrize("with_children", (False, True))
@pytest.mark.parametrize("log", (6, 11))
def test_runs(ctx, log, with_children):
    """one level as 1, 2, 3, 4 runs (k_merkle_small<0> / k_merkle_fused<0> x1..x4; <1> for a single run without children),
    as 5 and 9 runs (k_merkle_layer), as adjacent views (merged into one run), views with a gap (two runs) and a handle
    between two views (three runs)"""
    mc.check_runs(ctx, log, with_children)


def test_root_form_layouts(ctx):
    """lmn_op_merkle_root: k_merkle_layer for five columns shorter than 256 bytes, two runs for unsorted input"""
    mc.check_root_form_layouts(ctx)


@pytest.mark.parametrize("log", range(0, 15))
def test_single_size_every_log(ctx, log):
    """k_merkle_small<1> + nothing else up to 2^10; k_merkle_fused<1, NZ> + k_merkle_small<2> above (sub = 0)"""
    mc.check_single_size(ctx, log, 4 if log == 14 else 1 + log % 5, expect=("small<2>", "sub=0") if log > 10 else ())


@pytest.mark.parametrize("sub", (1, 2, 3))
@pytest.mark.parametrize("log", (11, 12, 13, 14))
def test_single_size_with_register_subtrees(ctx, log, sub, monkeypatch):
    """LMN_MERKLE_SUB = 1, 2, 3: sub is also capped by the levels the launch fuses (level - 10)"""
    monkeypatch.setenv("LMN_MERKLE_SUB", str(sub))
    mc.check_single_size(ctx, log, 2 + sub, sub_env=sub, expect=("sub=%d" % min(sub, log - 10),))


@pytest.mark.parametrize("k", (12, 13))
def test_mixed_sizes_against_the_planner(ctx, k):
    """columns at (k, k-1), (k, k-2), (k, 10), (k, 11), (k, 0), at 3, 2, 1, 0; k_merkle_fused<2> is in none of these by
    itself - see test_pure_inner_fused_level"""
    for name, shape, forms in mc.mixed_shapes(k):
        mc.check_mixed(ctx, name, shape, forms)


def test_mixed_sizes_with_register_subtrees(ctx, monkeypatch):
    monkeypatch.setenv("LMN_MERKLE_SUB", "2")
    for name, shape, forms in mc.mixed_shapes(13):
        mc.check_mixed(ctx, name, shape, forms, sub_env=2)


def test_pure_inner_fused_level(ctx):
    """k_merkle_fused<2>: a pointer-table level (five handles at 2^13) leaves the children-only levels below it to a fused
    launch of their own"""
    H = mc.Handles()
    try:
        rng = np.random.default_rng(8)
        mc.build_level(ctx, H, mc.random_cols(rng, 5, 13), "5 handles", rng)
        mc.check_tree(ctx, H, "five handles at 2^13", ["layer", "fused<2>", "small<2>"], root_form=False)
    finally:
        H.free()


@pytest.mark.parametrize("sub", (None, 3))
def test_columns_where_a_fused_run_ends(ctx, sub, monkeypatch):
    """from 2^14 a launch fuses level - 10 = 4 levels: columns at level 10 stop it after 3, columns at level 9 leave it whole"""
    if sub is not None:
        monkeypatch.setenv("LMN_MERKLE_SUB", str(sub))
    mc.check_fused_run_end(ctx, 14, 4, sub_env=sub)


def test_refusals_leave_the_context_usable(ctx):
    mc.check_refusals_leave_context_usable(ctx)
