"""`Context.grind_many` (lmn_ctx_grind_many, k_grind_many) on the MI355X: the checks of tests/grind_many_checks.py at
pow_bits up to 20, and a pair of digests whose nonce lies above 2^32 (64-bit window bases)."""
import os
import sys

import pytest

from luminair_amd import backend

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grind_many_checks as checks        # noqa: E402
from test_gpu_pow import PINNED_BITS, PINNED_DIGEST, PINNED_NONCE, PINNED_VARIANT     # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip_lib_path):
    return backend.default_library()


@pytest.fixture(scope="module")
def ctx(lib):
    c = backend.Context(0)
    yield c
    c.close()


@pytest.fixture
def small_window_ctx(lib, monkeypatch):
    c = checks.small_window_context(lib, monkeypatch)
    yield c
    c.close()


@pytest.mark.parametrize("variant", checks.FORMS)
@pytest.mark.parametrize("pow_bits", [0, 8, 16, 20])
@pytest.mark.parametrize("n", [64, 5, 2, 1])       # (the smaller calls reuse the host answers of the first)
def test_gpu_grind_many_equals_host_loop(lib, ctx, variant, pow_bits, n):
    checks.check_equals_host_loop(lib, ctx, variant, n, pow_bits)


@pytest.mark.parametrize("variant", checks.FORMS)
def test_gpu_grind_many_spread_nonces_in_either_order(lib, small_window_ctx, variant):
    checks.check_spread(lib, small_window_ctx, variant)


@pytest.mark.parametrize("variant", checks.FORMS)
def test_gpu_grind_many_duplicate_digests(lib, small_window_ctx, variant):
    checks.check_duplicates(lib, small_window_ctx, variant)


def test_gpu_grind_many_nonce_above_2_32(ctx):
    """about 3 * 10^10 nonces (two digests x 1.6 * 10^10)"""
    assert PINNED_NONCE > 1 << 32
    assert ctx.grind_many([PINNED_DIGEST, PINNED_DIGEST], PINNED_BITS, PINNED_VARIANT) == [PINNED_NONCE, PINNED_NONCE]


def test_gpu_grind_many_refusals_and_empty_call(lib, ctx):
    checks.check_refusals(lib, ctx)


def test_gpu_grind_many_of_one_agrees_with_grind(lib, small_window_ctx):
    checks.check_agrees_with_single_grind(lib, small_window_ctx)


def test_gpu_grind_many_largest_call(lib, ctx):
    checks.check_largest_call(lib, ctx)
