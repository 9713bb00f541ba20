"""A whole proof whose relation draws redraw (tests/redraw_checks.py) on a real MI355X: `lmn_prove` in its four transcript
forms and the lock-step batch library.  The pie has no lookup table, so `lmn_prove_prepared` has nothing to prepare."""
import pytest

import redraw_checks as rc
from luminair_amd import backend
from luminair_amd.batch import BATCH_LIB

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(rc.VARIANTS), ids=lambda n: n.replace(" ", "_"))
def test_gpu_prove_equals_oracle(hip_lib_path, name):
    rc.check_prove(backend.Library(hip_lib_path), name)


@pytest.mark.parametrize("name", sorted(rc.VARIANTS), ids=lambda n: n.replace(" ", "_"))
def test_gpu_middle_member_of_a_batch(hip_lib_path, name):
    rc.check_batch(backend.Library(hip_lib_path), BATCH_LIB, name)
