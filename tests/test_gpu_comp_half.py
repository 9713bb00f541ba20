"""The composition polynomial from half of its evaluation domain on a real MI355X: the shapes of the CPU suite
(tests/test_comp_half_emu.py) plus the two sizes around the lower boundary of the fixed-shape strided kernels; the checks are
in tests/comp_half_checks.py."""
import pytest

import comp_half_checks as ch
from luminair_amd import backend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def provers(hip_lib_path):
    p = ch.Provers(backend.Library(hip_lib_path))
    yield p
    p.close()


@pytest.fixture(scope="module")
def c_oracle():
    from oracle.cbackend import CKernels
    return CKernels()


@pytest.mark.parametrize("case", ch.shared_cases(), ids=lambda c: c[0])
def test_gpu_proofs_are_byte_identical(provers, case, monkeypatch):
    ch.check_case(provers, case, monkeypatch)


@pytest.mark.parametrize("case", ch.gpu_size_cases(), ids=lambda c: c[0])
def test_gpu_sizes_around_the_fixed_kernels_boundary(provers, c_oracle, case, monkeypatch):
    ch.check_case(provers, case, monkeypatch, kernels=c_oracle)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("log_rows", [12, 13])
def test_gpu_invalid_traces_are_rejected_on_both_paths(provers, monkeypatch, log_rows, which):
    """a broken constraint still ends in LMN_ERR_CONSTRAINTS with and without the switch: at 2^12 rows (the whole domain on
    both paths) and at 2^13 (the smallest table that takes the half-domain path), for two corruptions at different rows"""
    ch.check_invalid_trace(provers.ctx(ch.KAT), monkeypatch, log_rows, which)
