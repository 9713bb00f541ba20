"""`Col.batch_inverse` / `Col.batch_inverse_secure` (lmn_col_batch_inverse*, k_batch_inverse_m / _q) on a real MI355X: the
checks of tests/field_ops_checks.py at every log size from 0 to 13, and the defining identity at 2^20 and 2^22 rows."""
import pytest

import field_ops_checks as checks
from luminair_amd import backend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(hip_lib_path):
    c = backend.Context(0, None, backend.Library(hip_lib_path))
    yield c
    c.close()


@pytest.mark.parametrize("log", checks.LOGS)
def test_gpu_batch_inverse_every_class_and_column_count(ctx, log):
    checks.check_m31_classes(ctx, log)


@pytest.mark.parametrize("log", checks.LOGS)
def test_gpu_batch_inverse_one_zero_and_all_zero_but_one(ctx, log):
    checks.check_m31_one_zero(ctx, log)


@pytest.mark.parametrize("log", checks.LOGS)
def test_gpu_batch_inverse_secure_every_class(ctx, log):
    checks.check_qm31_classes(ctx, log)


@pytest.mark.parametrize("log", checks.LOGS)
def test_gpu_batch_inverse_secure_every_coordinate_support(ctx, log):
    checks.check_qm31_subsets(ctx, log)


@pytest.mark.parametrize("log", checks.LOGS)
def test_gpu_batch_inverse_secure_one_zero_and_all_zero_but_one(ctx, log):
    checks.check_qm31_one_zero(ctx, log)


@pytest.mark.parametrize("secure", [False, True])
@pytest.mark.parametrize("log", checks.VIEW_LOGS)
def test_gpu_batch_inverse_on_views(ctx, log, secure):
    checks.check_views(ctx, log, secure)


def test_gpu_batch_inverse_refusals(ctx):
    checks.check_refusals(ctx)


@pytest.mark.parametrize("log,secure,cls", [(20, False, "random"), (22, False, "zero_out"),
                                            (20, True, "zero_out"), (22, True, "random")])
def test_gpu_batch_inverse_large(ctx, log, secure, cls):
    checks.check_large(ctx, log, secure, cls)


def test_gpu_batch_inverse_in_the_batch_library(hip_lib_path):
    """the lock-step batch library exports the same entry points and runs the same kernels behind its trampoline"""
    import os
    lib = backend.Library(os.path.join(os.path.dirname(hip_lib_path), "libluminair_hip_batch.so"))
    c = backend.Context(0, None, lib)
    try:
        checks.check_m31_classes(c, 12, ncols_list=(3,), classes=("zero_out",))
        checks.check_qm31_classes(c, 12, classes=("zero_out",))
    finally:
        c.close()
