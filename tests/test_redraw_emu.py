"""A whole proof whose relation draws redraw (tests/redraw_checks.py) on the emulation build (tests/emu: the same HIP
sources compiled for the CPU) and its lock-step batch library; tests/test_gpu_redraw.py runs the same on the device."""
import os
import subprocess

import pytest

import redraw_checks as rc
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
def emu_batch_so(emu_so):
    import test_batch_emu
    return test_batch_emu._build()


@pytest.mark.parametrize("name", sorted(rc.VARIANTS), ids=lambda n: n.replace(" ", "_"))
def test_reference_redraws_in_the_recorded_set(name):
    """no library: the oracle redrew in the recorded set and nowhere else, and its verifier accepts the proof"""
    rc.reference(name)


@pytest.mark.parametrize("name", sorted(rc.VARIANTS), ids=lambda n: n.replace(" ", "_"))
def test_reference_proof_depends_on_the_drawn_elements(name):
    """no library: the comparison with the oracle's bytes is not blind to the draws under test"""
    rc.check_reference_depends_on_the_draws(name)


@pytest.mark.parametrize("name", sorted(rc.VARIANTS), ids=lambda n: n.replace(" ", "_"))
def test_prove_equals_oracle(emu_so, name):
    """by default, under LMN_CHAN_STEP_SEPARATE=1, LMN_HOST_FS=1 and LMN_HOST_QUOT=1; lmn_verify accepts.  A draw loop that
    never leaves its redraw fails the case at the limit"""
    ts.bounded(ts.LIMIT, rc.check_prove, backend.Library(emu_so), name)


@pytest.mark.parametrize("name", sorted(rc.VARIANTS), ids=lambda n: n.replace(" ", "_"))
def test_middle_member_of_a_batch(emu_so, emu_batch_so, name):
    ts.bounded(ts.LIMIT, rc.check_batch, backend.Library(emu_so), emu_batch_so, name)
