"""Value and shape edges of the level-2 field ops on the emulation build (tests/emu: the same HIP sources compiled for
the CPU), against the plain-integer and oracle references of tests/numeric_checks.py.  The GPU counterpart, with the
sizes above 2^20, is tests/test_gpu_numeric_edges.py."""
import os
import subprocess

import numpy as np
import pytest

import numeric_checks as nc
from luminair_amd import backend

CLASSES = nc.CLASSES
NCOLS = (1, 2, 3, 5)


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


@pytest.mark.parametrize("lc,ld", nc.SMALL_DOMAIN_CASES)
def test_evaluate_onto_16_points_or_fewer_zero_extends(ctx, lc, ld):
    """regression: the single-stage transform (2^4 points or fewer) read its whole first group with vector loads when
    only the first word was inside the coefficients"""
    nc.check_small_domain_evaluate(ctx, lc, ld)


@pytest.mark.parametrize("log", [1, 2, 3, 4, 5])
def test_fft_small_every_blowup_ncols_class(ctx, log):
    for blowup in range(4):
        for ncols in NCOLS:
            for cls in CLASSES:
                nc.check_fft_case(ctx, log, blowup, ncols, cls)


@pytest.mark.parametrize("log", [8, 11, 12, 13])
def test_fft_every_class(ctx, log):
    for i, cls in enumerate(CLASSES):
        for blowup in range(4):
            nc.check_fft_case(ctx, log, blowup, NCOLS[(i + blowup) % 4], cls, col_form=blowup == i % 4)


@pytest.mark.parametrize("log", [16, 17, 18])
def test_fft_large_every_class(ctx, log):
    for i, cls in enumerate(CLASSES):
        blowup = i % 4 if log < 18 else i % 2
        nc.check_fft_case(ctx, log, blowup, 1 if log == 18 else NCOLS[i % 3], cls, col_form=i == 0)


@pytest.mark.parametrize("log", [1, 4, 8, 12])
def test_constant_columns(ctx, log):
    nc.check_constant_columns(ctx, log)


@pytest.mark.parametrize("cls", CLASSES)
def test_evaluate_block(ctx, cls):
    for lc, ld in ((4, 5), (11, 12), (12, 13), (13, 14), (16, 17)):
        for g in (1, 2, 3):
            nc.check_evaluate_block_case(ctx, lc, ld, g, cls, col_form=g == 2)


@pytest.mark.parametrize("cls", CLASSES)
def test_eval_at_point(ctx, cls):
    for log in (1, 2, 9, 10, 11, 14, 19):
        nc.check_eval_at_point_case(ctx, log, cls)


@pytest.mark.parametrize("npts", [1, 2, 3, 4])
def test_quotients_every_batch_count(ctx, npts):
    for i, cls in enumerate(CLASSES):
        for log in (2, 3, 4, 8, 12):
            for k in range(1, 8):           # 1-7 entries per batch: the 6-wide loop and every tail
                if log == 12 and k not in (1, 6, 7):
                    continue
                per = [1 + (k + b) % 7 for b in range(npts)]
                per[0] = k
                nc.check_quotients_case(ctx, cls, log, npts, per, col_form=k % 3 == i % 3)


def test_quotients_near_the_entry_limit(ctx):
    for cls in ("random", "pm1", "zero_out"):
        nc.check_quotients_case(ctx, cls, 3, 4, [126, 125, 124, 125])     # 500 samples


def test_quotient_limits_are_caller_errors(ctx):
    nc.check_quotient_limits(ctx)


@pytest.mark.parametrize("cls", CLASSES)
def test_folds(ctx, cls):
    for log_src in (1, 2, 8, 9, 10, 20):
        nc.check_folds_case(ctx, log_src, cls, col_form=log_src != 20)


@pytest.mark.parametrize("cls", CLASSES)
def test_decompose_accumulate_bit_reverse(ctx, cls):
    for log in (1, 2, 9, 10, 17) + ((19,) if cls in ("pm1", "zero_out") else ()):    # 2^19 for all classes: GPU suite
        nc.check_decompose_accumulate_bitrev_case(ctx, log, cls)


@pytest.mark.parametrize("log", [4, 12])
def test_logup_every_kind(ctx, log):
    from oracle import air
    for kind in sorted(air.COMPONENTS):
        for cls in (("random", "pm1", "edge") if log == 4 else ("random",)):
            nc.check_logup_kind(ctx, kind, log, cls)


@pytest.mark.parametrize("log", [4, 12])
def test_composition_every_kind(ctx, log):
    from oracle import air
    for kind in sorted(air.COMPONENTS):
        for cls in ("pm1", "random"):
            for coeff_cls in ("pm1", "random"):
                nc.check_composition_kind(ctx, kind, log, cls, coeff_cls)


# ---- logup at every scan shape.  Fractions: a partly filled 256-lane block (logs 4 to 7), exactly one block (8).  Scan:
# one partly filled block (4), two blocks and the first block's total as the second's offset (11: the only such size, the
# coalesced scan takes over at 12), one workgroup of the coalesced scan (12), two workgroups with paired regions (13).
LOGUP_SMALL_CLASSES = ("random", "pm1", "edge", "alt")
LOGUP_DIRTY_LOGS = (11, 13, 19)         # block totals land in arena words that held other data


@pytest.mark.parametrize("log", [4, 5, 7, 8])
def test_logup_small_every_kind_and_class_against_plain_integers(ctx, log):
    from oracle import air
    assert log <= nc.PY_MAX_LOG
    for kind in sorted(air.COMPONENTS):
        for cls in LOGUP_SMALL_CLASSES:
            nc.check_logup_kind(ctx, kind, log, cls)


@pytest.mark.parametrize("log", [9, 10, 11, 12, 13])
def test_logup_scan_shapes(ctx, log):
    """kinds 4, 0 and 13: 1, 3 and 7 relations; kind 14 (a width-1 lookup) where the scan changes form"""
    if log in LOGUP_DIRTY_LOGS:
        nc.dirty_context(ctx, np.random.default_rng(log))
    for kind in (4, 0, 13) + ((14,) if log in (11, 13) else ()):
        nc.check_logup_kind(ctx, kind, log, "random")


def test_logup_refusals(ctx):
    nc.check_logup_refusals(ctx)


# ---- composition
@pytest.mark.parametrize("log", [4, 5, 7])
def test_composition_relations_against_plain_integers(ctx, log):
    from oracle import air
    for kind in sorted(air.COMPONENTS):
        for cls in ("random", "pm1", "edge", "alt"):
            for coeff_cls in ("random", "pm1"):
                nc.check_composition_relations(ctx, kind, log, cls, coeff_cls)


@pytest.mark.parametrize("log", [4, 5, 7, 8, 12, 13])
def test_composition_shapes_and_classes(ctx, log):
    """2^5 points: a partly filled block; 2^8: exactly one block"""
    from oracle import air
    for kind in sorted(air.COMPONENTS):
        for cls, coeff_cls in nc.composition_class_pairs(kind, log):
            nc.check_composition_kind(ctx, kind, log, cls, coeff_cls)


@pytest.mark.parametrize("log", [5, 12])
def test_composition_accumulator_zero_and_cancelling(ctx, log):
    from oracle import air
    for kind in sorted(air.COMPONENTS) if log == 5 else nc.COMPOSITION_LARGE_KINDS:
        for acc in ("zero", "cancel"):
            nc.check_composition_kind(ctx, kind, log, "random", "random", acc=acc)


@pytest.mark.parametrize("k", [4, 6])
def test_composition_of_a_valid_witness_is_low_degree(ctx, k):
    from oracle import air
    for kind in sorted(air.COMPONENTS):
        nc.check_low_degree(ctx, kind, k)
