"""Value and shape edges of the level-2 field ops on a real MI355X, against the references of tests/numeric_checks.py:
the CPU suite's matrix (tests/test_numeric_edges_emu.py) plus the sizes above 2^20 - the two-pass FFT up to 2^22, the
three-pass sizes 2^23 and 2^25 (the C oracle is the reference there), cpb remainders once tiles reach 512 / 2048, logup
at the lane and batch counts of its block-total scan (2^15 to 2^21 rows) and composition on 2^19 points."""
import numpy as np
import pytest

import numeric_checks as nc
from luminair_amd import backend

pytestmark = pytest.mark.gpu

CLASSES = nc.CLASSES
NCOLS = (1, 2, 3, 5)


@pytest.fixture(scope="module")
def ctx(hip_lib_path):
    c = backend.Context(0, None, backend.Library(hip_lib_path))
    yield c
    c.close()


@pytest.mark.parametrize("lc,ld", nc.SMALL_DOMAIN_CASES)
def test_gpu_evaluate_onto_16_points_or_fewer_zero_extends(ctx, lc, ld):
    nc.check_small_domain_evaluate(ctx, lc, ld)


@pytest.mark.parametrize("log", [1, 2, 3, 4, 5])
def test_gpu_fft_small_every_blowup_ncols_class(ctx, log):
    for blowup in range(4):
        for ncols in NCOLS:
            for cls in CLASSES:
                nc.check_fft_case(ctx, log, blowup, ncols, cls)


@pytest.mark.parametrize("log", [8, 11, 12, 13, 16, 17, 18])
def test_gpu_fft_every_class(ctx, log):
    for i, cls in enumerate(CLASSES):
        for blowup in range(4):
            nc.check_fft_case(ctx, log, blowup, NCOLS[(i + blowup) % 4], cls, col_form=blowup == i % 4)


@pytest.mark.parametrize("log", [21, 22])
def test_gpu_fft_two_pass_large(ctx, log):
    for i, cls in enumerate(CLASSES):
        blowup = i % 4 if log == 21 else i % 2
        nc.check_fft_case(ctx, log, blowup, (3, 5, 2)[i % 3], cls, col_form=i == 0)


@pytest.mark.parametrize("log,cases", [(23, ((0, 5, "random"), (1, 3, "pm1"), (2, 2, "zero_out"), (0, 3, "alt"))),
                                       (25, ((0, 2, "random"), (1, 1, "edge")))])
def test_gpu_fft_three_pass(ctx, log, cases):
    for blowup, ncols, cls in cases:
        nc.check_fft_case(ctx, log, blowup, ncols, cls, col_form=False)


@pytest.mark.parametrize("log", [1, 4, 8, 12, 22])
def test_gpu_constant_columns(ctx, log):
    nc.check_constant_columns(ctx, log)


@pytest.mark.parametrize("cls", CLASSES)
def test_gpu_evaluate_block(ctx, cls):
    for lc, ld in ((4, 5), (11, 12), (12, 13), (13, 14), (16, 17), (20, 21), (22, 23)):
        for g in (1, 2, 3):
            nc.check_evaluate_block_case(ctx, lc, ld, g, cls, ncols=3 if ld < 21 else 1, col_form=g == 2)


@pytest.mark.parametrize("cls", CLASSES)
def test_gpu_eval_at_point(ctx, cls):
    for log in (1, 2, 9, 10, 11, 14, 19):
        nc.check_eval_at_point_case(ctx, log, cls)


@pytest.mark.parametrize("npts", [1, 2, 3, 4])
def test_gpu_quotients_every_batch_count(ctx, npts):
    for i, cls in enumerate(CLASSES):
        for log in (2, 3, 4, 8, 12):
            for k in range(1, 8):
                if log == 12 and k not in (1, 6, 7):
                    continue
                per = [1 + (k + b) % 7 for b in range(npts)]
                per[0] = k
                nc.check_quotients_case(ctx, cls, log, npts, per, col_form=k % 3 == i % 3)


def test_gpu_quotients_near_the_entry_limit(ctx):
    for cls in ("random", "pm1", "zero_out"):
        nc.check_quotients_case(ctx, cls, 3, 4, [126, 125, 124, 125])


def test_gpu_quotient_limits_are_caller_errors(ctx):
    nc.check_quotient_limits(ctx)


@pytest.mark.parametrize("cls", CLASSES)
def test_gpu_folds(ctx, cls):
    for log_src in (1, 2, 8, 9, 10, 20):
        nc.check_folds_case(ctx, log_src, cls)


@pytest.mark.parametrize("cls", CLASSES)
def test_gpu_decompose_accumulate_bit_reverse(ctx, cls):
    for log in (1, 2, 9, 10, 17, 19):
        nc.check_decompose_accumulate_bitrev_case(ctx, log, cls)


@pytest.mark.parametrize("log", [4, 12])
def test_gpu_logup_every_kind(ctx, log):
    from oracle import air
    for kind in sorted(air.COMPONENTS):
        for cls in ("random", "pm1", "edge"):
            nc.check_logup_kind(ctx, kind, log, cls)


@pytest.mark.parametrize("log", [4, 12])
def test_gpu_composition_every_kind(ctx, log):
    from oracle import air
    for kind in sorted(air.COMPONENTS):
        for cls in ("pm1", "random"):
            for coeff_cls in ("pm1", "random"):
                nc.check_composition_kind(ctx, kind, log, cls, coeff_cls)


# ---- logup at every scan shape: the CPU suite's sizes with all 17 kinds, plus the lane and batch counts of the
# block-total scan: 2^8 totals on 256 lanes, every lane loaded (15), two totals per lane (16), eight per lane on the last
# 256-lane size (18), 1024 lanes in 16 waves (19), sixteen per lane, so a second batch of eight (21)
LOGUP_SMALL_CLASSES = ("random", "pm1", "edge", "alt")
LOGUP_DIRTY_LOGS = (11, 13, 19)


@pytest.mark.parametrize("log", [4, 5, 7, 8])
def test_gpu_logup_small_every_kind_and_class_against_plain_integers(ctx, log):
    from oracle import air
    assert log <= nc.PY_MAX_LOG
    for kind in sorted(air.COMPONENTS):
        for cls in LOGUP_SMALL_CLASSES:
            nc.check_logup_kind(ctx, kind, log, cls)


@pytest.mark.parametrize("log", [9, 10, 11, 12, 13])
def test_gpu_logup_scan_shapes(ctx, log):
    from oracle import air
    if log in LOGUP_DIRTY_LOGS:
        nc.dirty_context(ctx, np.random.default_rng(log))
    for kind in sorted(air.COMPONENTS):
        nc.check_logup_kind(ctx, kind, log, "random")


@pytest.mark.parametrize("log,kind,cls", [(log, kind, cls) for log in (15, 16, 18, 19)
                                          for kind, cls in ((4, "random"), (4, "pm1"), (13, "random"))] + [(21, 4, "random")])
def test_gpu_logup_block_total_scan_shapes(ctx, log, kind, cls):
    """one case per test: the numpy oracle takes seconds at these sizes (kind 13 stops at 2^19, 2^21 is kind 4 alone)"""
    if log in LOGUP_DIRTY_LOGS and (kind, cls) == (4, "random"):
        nc.dirty_context(ctx, np.random.default_rng(log))
    nc.check_logup_kind(ctx, kind, log, cls)


def test_gpu_logup_refusals(ctx):
    nc.check_logup_refusals(ctx)


# ---- composition
@pytest.mark.parametrize("log", [4, 5, 7])
def test_gpu_composition_relations_against_plain_integers(ctx, log):
    from oracle import air
    for kind in sorted(air.COMPONENTS):
        for cls in ("random", "pm1", "edge", "alt"):
            for coeff_cls in ("random", "pm1"):
                nc.check_composition_relations(ctx, kind, log, cls, coeff_cls)


@pytest.mark.parametrize("log", [4, 5, 7, 8, 12, 13])
def test_gpu_composition_shapes_and_classes(ctx, log):
    from oracle import air
    for kind in sorted(air.COMPONENTS):
        for cls, coeff_cls in nc.composition_class_pairs(kind, log):
            nc.check_composition_kind(ctx, kind, log, cls, coeff_cls)


@pytest.mark.parametrize("kind", nc.COMPOSITION_LARGE_KINDS)
def test_gpu_composition_2_19_points(ctx, kind):
    for cls, coeff_cls in nc.composition_class_pairs(kind, 18):
        nc.check_composition_kind(ctx, kind, 18, cls, coeff_cls)


@pytest.mark.parametrize("log", [5, 12])
def test_gpu_composition_accumulator_zero_and_cancelling(ctx, log):
    from oracle import air
    for kind in sorted(air.COMPONENTS) if log == 5 else nc.COMPOSITION_LARGE_KINDS:
        for acc in ("zero", "cancel"):
            nc.check_composition_kind(ctx, kind, log, "random", "random", acc=acc)


@pytest.mark.parametrize("k", [4, 6])
def test_gpu_composition_of_a_valid_witness_is_low_degree(ctx, k):
    from oracle import air
    for kind in sorted(air.COMPONENTS):
        nc.check_low_degree(ctx, kind, k)
