"""The FRI commit loop layer by layer (`lmn_col_fri_commit`) on the emulation build (tests/emu: the same HIP sources compiled
for the CPU), against the plain-integer / hashlib / oracle references of tests/fri_checks.py.  Everything stays at or below
2^14: the fused forms are reached from 2^11 on, the register subtrees through LMN_MERKLE_SUB and the first tree's `below`
form through LMN_MERKLE_BELOW_MIN_LOG at its floor of 12; tests/test_gpu_fri_commit.py crosses the same thresholds by size."""
import os
import subprocess

import pytest

import fri_checks as fc
import transcript_seeds as ts
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
def ctxs(emu_so):
    c = fc.Contexts(backend.Library(emu_so))
    yield c
    c.close()


def test_matrix_reaches_every_form():
    """every form code without a switch, and tails of 0, 1, 2 and 9 layers: a condition on plan() alone"""
    fc.check_matrix_reaches_every_form(fc.CASES)


def test_plan_tail_lengths():
    fc.check_plan_tail_lengths()


@pytest.mark.parametrize("case", fc.SHAPE_CASES, ids=lambda c: c.id)
def test_shape(ctxs, case):
    """roots, alphas, every layer, every written tree level, the absent levels and the form codes; the same under
    LMN_NO_FOLD_FUSION=1 and LMN_NO_JOIN_FUSION=1"""
    fc.check_case(ctxs, case)


@pytest.mark.parametrize("case", fc.CLASS_CASES, ids=lambda c: c.id)
def test_value_class(ctxs, case):
    """all 0, all P-1, alternating, EDGE_WORDS, random, pairs with a + b = 0 and with a == b in every input column; all 0 in
    cols[0] alone and in the joining columns alone"""
    fc.check_case(ctxs, case)


def test_redraw_cases_reach_every_draw():
    fc.check_redraw_cases_reach_every_draw(fc.REDRAW_CASES)


@pytest.mark.parametrize("case", fc.REDRAW_CASES, ids=lambda c: c.id)
def test_redraw(ctxs, case):
    """the transcript's value edges (tests/golden/transcript_redraw_seeds.json): a redraw, the accepted word 0xFFFFFFFD and a
    word P at a chosen tree; the reference must have met the event there, and only there, before the loop is asked.  A loop
    that never leaves its redraw fails the case at the limit"""
    ts.bounded(ts.LIMIT, fc.check_case, ctxs, case)


def test_refusals_leave_context_and_handles_usable(ctxs):
    fc.check_refusals(ctxs)


def test_sharded_context_is_refused(ctxs):
    fc.check_sharded_context_refused(ctxs)
