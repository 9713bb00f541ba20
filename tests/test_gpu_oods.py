"""The sampled values and the quotient tables at their shape edges (tests/oods_checks.py) on a real MI355X: the matrix of
the CPU suite (tests/test_oods_emu.py) and the 2^17-row case (16 chunks next to a sub-table job), in process, one context
per configuration for the whole module."""
import pytest

import oods_checks as oc
from luminair_amd import backend
from luminair_amd.batch import BATCH_LIB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def provers(hip_lib_path):
    p = oc.Provers(backend.Library(hip_lib_path))
    yield p
    p.close()


@pytest.fixture(scope="module")
def c_oracle():
    from oracle.cbackend import CKernels
    return CKernels()


def test_gpu_sampled_values_equal_plain_integers(provers, monkeypatch):
    oc.check_pin_pie_on_library(provers, monkeypatch)


@pytest.mark.parametrize("case", oc.CASES, ids=lambda c: c.name.replace(" ", "_"))
def test_gpu_proof_equals_oracle_on_the_expected_path(provers, c_oracle, case, monkeypatch):
    """default, LMN_HOST_QUOT=1, LMN_HOST_FS=1: the oracle's bytes; counter 22 on the device path, 23 on the host's wait"""
    oc.check_case(provers, case, monkeypatch, kernels=c_oracle if case.max_log >= oc.C_ORACLE_MIN_LOG else None)


@pytest.mark.parametrize("case", oc.GPU_ONLY_CASES, ids=lambda c: c.name.replace(" ", "_"))
def test_gpu_sixteen_chunks_next_to_a_sub_table_job(provers, c_oracle, case, monkeypatch):
    oc.check_case(provers, case, monkeypatch, kernels=c_oracle)


def test_gpu_batch_members_equal_solo_proofs(hip_lib_path, monkeypatch):
    oc.check_batch_library(backend.Library(hip_lib_path), BATCH_LIB, monkeypatch)


def test_gpu_eight_nine_eight_sizes_on_one_context(hip_lib_path, monkeypatch):
    oc.check_back_to_back(backend.Library(hip_lib_path), monkeypatch)
