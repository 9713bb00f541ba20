"""The sampled values and the quotient tables at their shape edges (tests/oods_checks.py) on the oracle alone and on the
emulation build (tests/emu: the same HIP sources compiled for the CPU) with its lock-step batch library;
tests/test_gpu_oods.py runs the same on the device, with the 2^17-row case."""
import os
import subprocess

import pytest

import oods_checks as oc
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
def provers(emu_so):
    p = oc.Provers(backend.Library(emu_so))
    yield p
    p.close()


@pytest.fixture(scope="module")
def emu_batch_so(emu_so):
    import test_batch_emu
    return test_batch_emu._build()


def test_matrix_reaches_every_edge():
    """no library: all four Blake2s residues on the device path (a full last block at two block counts), both paths, 8 and 9
    sizes, 2 and 10 sample points, both multiplicity forms - from the oracle's proofs alone"""
    oc.check_matrix_reaches_every_edge()


def test_a_mismatch_is_named_by_its_first_field():
    """no library: the message of a failing case says "evaluation" or "quotient tables / quotient kernel", not "bytes differ\""""
    oc.check_first_difference_names_the_field()


def test_sampled_values_equal_plain_integers(provers, monkeypatch):
    """the oracle's sampled values of a five-size pie against Python integers; the same pie through the library"""
    oc.check_pin_pie_on_library(provers, monkeypatch)


@pytest.mark.parametrize("case", oc.CASES, ids=lambda c: c.name.replace(" ", "_"))
def test_emu_proof_equals_oracle_on_the_expected_path(provers, case, monkeypatch):
    """default, LMN_HOST_QUOT=1, LMN_HOST_FS=1: the oracle's bytes; counter 22 on the device path, 23 on the host's wait"""
    oc.check_case(provers, case, monkeypatch)


def test_emu_batch_members_equal_solo_proofs(emu_so, emu_batch_so, monkeypatch):
    oc.check_batch_library(backend.Library(emu_so), emu_batch_so, monkeypatch)


def test_emu_eight_nine_eight_sizes_on_one_context(emu_so, monkeypatch):
    oc.check_back_to_back(backend.Library(emu_so), monkeypatch)
