"""The FRI commit loop layer by layer (`lmn_col_fri_commit`) on a real MI355X, against the references of tests/fri_checks.py:
the CPU suite's matrix (tests/test_fri_commit_emu.py) plus what only size reaches - first columns of 2^18 .. 2^22, where
commit.cpp itself chooses register subtrees of depth 1, 2, 3 for the fold launch and splits a layer's tree over several
fused launches, and the first tree's `below` form at its default threshold of 2^19."""
import pytest

import fri_checks as fc
from luminair_amd import backend

pytestmark = pytest.mark.gpu

BIG_CASES = [fc.Case("first column 2^%d" % k, (k,), u32=bool(k & 1)) for k in (18, 19, 20, 21, 22)] + [
    fc.Case("below at the default threshold", (19, 18)),
    fc.Case("not below under the default threshold", (18, 17, 12)),
]


@pytest.fixture(scope="module")
def ctxs(hip_lib_path):
    c = fc.Contexts(backend.Library(hip_lib_path))
    yield c
    c.close()


def test_gpu_matrix_reaches_every_form():
    fc.check_matrix_reaches_every_form(fc.CASES)
    forms = set()
    for c in BIG_CASES:
        forms |= c.plan().forms()
        assert all(len(a) <= 3 for a in c.plan().absent)
    assert fc.FIRST_TREE_BELOW in forms
    # register subtrees by size alone: some tree of every depth 1, 2, 3
    assert {len(a) for c in BIG_CASES for a in c.plan().absent} >= {0, 1, 2, 3}


def test_gpu_redraw_cases_reach_every_draw():
    """which draw implementation each redraw reaches, from plan(): k_merkle_small's step for the first tree and for an inner
    tree, k_fri_tail's first (with and without the front fold), middle and last layer, in both draw encodings per kernel; the
    single-lane k_chan_mix_root_draw cannot be reached by an unsharded context (fri_checks.check_redraw_cases_reach_every_draw
    states commit.cpp's condition)"""
    fc.check_redraw_cases_reach_every_draw(fc.REDRAW_CASES)


@pytest.mark.parametrize("case", fc.REDRAW_CASES, ids=lambda c: c.id)
def test_gpu_redraw(ctxs, case):
    fc.check_case(ctxs, case)


@pytest.mark.parametrize("case", fc.SHAPE_CASES, ids=lambda c: c.id)
def test_gpu_shape(ctxs, case):
    fc.check_case(ctxs, case)


@pytest.mark.parametrize("case", fc.CLASS_CASES, ids=lambda c: c.id)
def test_gpu_value_class(ctxs, case):
    fc.check_case(ctxs, case)


@pytest.mark.parametrize("case", BIG_CASES, ids=lambda c: c.id)
def test_gpu_size(ctxs, case):
    """every layer and every written level of every tree in full, in the default form and under LMN_NO_FOLD_FUSION=1 and
    LMN_NO_JOIN_FUSION=1; the reference from 2^17 is the C oracle, computed once per case"""
    fc.check_case(ctxs, case)


def test_gpu_refusals_leave_context_and_handles_usable(ctxs):
    fc.check_refusals(ctxs)


def test_gpu_sharded_context_is_refused(ctxs):
    fc.check_sharded_context_refused(ctxs)
