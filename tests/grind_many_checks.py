"""Checks of `Context.grind_many` (lmn_ctx_grind_many, k_grind_many) shared by tests/test_grind_many_emu.py (the
emulation build, no GPU) and tests/test_gpu_grind_many.py (the MI355X): every nonce equals the host loop's
(`Library.grind` = lmn_op_grind; the oracle's `Blake2sChannel.grind` confirms the host loop on the cheap cases), for the
three proof-of-work forms, for digests that finish in different rounds, in either order, and for repeated digests; the
refusals name their argument.

A context made under LMN_POW_WINDOW_LOG=11 grinds in rounds of 8 launches x 2^11 nonces per digest (up to 8 pending
digests), so that pow_bits 16 needs several rounds and a pending table that shrinks; the default window finishes these
cases in the first round."""
import ctypes as C
import functools
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from luminair_amd import backend                                   # noqa: E402
from oracle.channel import Blake2sChannel, ProtocolVariant        # noqa: E402

# the three forms: bare compression (KAT), blake2s(digest || nonce), blake2s(prefixed digest || nonce)
FORMS = [backend.VARIANT_KAT, 0x4, 0x10]
WINDOW_LOG = 11                      # LMN_POW_WINDOW_LOG of the several-round contexts: the smallest window, one block
WINDOWS_PER_WAIT = 8                 # launches per round (phase_decommit.cpp POW_WINDOWS_PER_WAIT)
ROUND_ONE = WINDOWS_PER_WAIT << WINDOW_LOG    # nonces per digest examined before the first wait, up to 8 digests pending
GRIND_MANY_MAX = 1024                # LMN_GRIND_MANY_MAX


def digest(i):
    return hashlib.sha256(b"pow grind digest %d" % i).digest()


_host_cache = {}


def host_nonce(lib, d, pow_bits, variant):
    """the host loop's nonce, computed once per (digest, pow_bits, form) and shared by the cases"""
    key = (d, pow_bits, variant)
    if key not in _host_cache:
        _host_cache[key] = lib.grind(d, pow_bits, variant)
    return _host_cache[key]


def oracle_nonce(d, pow_bits, variant):
    ch = Blake2sChannel(ProtocolVariant(variant))
    ch.digest = d
    return ch.grind(pow_bits)


def small_window_context(lib, monkeypatch):
    monkeypatch.setenv("LMN_POW_WINDOW_LOG", str(WINDOW_LOG))     # read when the context is created
    return backend.Context(0, lib.default_config(), lib)


def check_equals_host_loop(lib, ctx, variant, n, pow_bits):
    ds = [digest(5000 + 97 * pow_bits + i) for i in range(n)]     # the cases of one pow_bits share their digests
    want = [host_nonce(lib, d, pow_bits, variant) for d in ds]
    if pow_bits <= 8:                                              # (the oracle hashes in Python: cheap cases only)
        assert want[0] == oracle_nonce(ds[0], pow_bits, variant)
    assert ctx.grind_many(ds, pow_bits, variant) == want


@functools.lru_cache(maxsize=None)
def _spread_pick(lib_path, variant):
    """5 digests at pow_bits 16 whose host nonces are spread: one inside the first block, one beyond round one of a
    2^11-window context (so a second wait and a compacted pending table occur), three in between"""
    lib = backend.Library(lib_path)
    pool = [(host_nonce(lib, digest(i), 16, variant), digest(i)) for i in range(160)]
    near = min(pool)
    # beyond the first round however it is read: 8 launches x 2^11 nonces, and 8 times that for good measure
    far = min(p for p in pool if p[0] >= WINDOWS_PER_WAIT * ROUND_ONE)
    mid = sorted(p for p in pool if (1 << WINDOW_LOG) <= p[0] < far[0])[:3]
    assert len(mid) == 3
    return [mid[0], far, near, mid[1], mid[2]]


def check_spread(lib, ctx, variant):
    picked = _spread_pick(lib.path, variant)
    nonces = [p[0] for p in picked]
    assert min(nonces) < 1 << WINDOW_LOG, nonces                   # done in the first block of the first launch
    assert max(nonces) >= ROUND_ONE * WINDOWS_PER_WAIT, nonces     # needs a later round, alone in the pending table
    ds = [p[1] for p in picked]
    assert ctx.grind_many(ds, 16, variant) == nonces
    assert ctx.grind_many(ds[::-1], 16, variant) == nonces[::-1]


def check_duplicates(lib, ctx, variant, pow_bits=12):
    a, b = digest(31), digest(32)
    ds = [a, b, a, a, b, a]
    assert ctx.grind_many(ds, pow_bits, variant) == [host_nonce(lib, d, pow_bits, variant) for d in ds]


def check_agrees_with_single_grind(lib, ctx, pow_bits=12):
    for variant in FORMS:
        d = digest(77)
        assert ctx.grind_many([d], pow_bits, variant) == [ctx.grind(d, pow_bits, variant)]
        assert ctx.grind(d, pow_bits, variant) == host_nonce(lib, d, pow_bits, variant)


def check_refusals(lib, ctx):
    fn = lib.lib.lmn_ctx_grind_many
    h = ctx.handle
    two = digest(1) + digest(2)
    out = (C.c_uint64 * 2)(7, 7)

    def refused(word, *args):
        assert fn(*args) == backend.ERR_INVALID_ARGUMENT, word
        msg = lib.lib.lmn_last_error(args[0]).decode()
        assert "lmn_ctx_grind_many" in msg and word in msg, (word, msg)

    refused("ctx", None, two, 2, 5, 0, out)
    refused("digests", h, None, 2, 5, 0, out)
    refused("nonces_out", h, two, 2, 5, 0, None)
    big = digest(3) * (GRIND_MANY_MAX + 1)
    big_out = (C.c_uint64 * (GRIND_MANY_MAX + 1))()
    refused("LMN_GRIND_MANY_MAX", h, big, GRIND_MANY_MAX + 1, 5, 0, big_out)
    refused("pow_bits", h, two, 2, 41, 0, out)
    refused("protocol_variant", h, two, 2, 5, 1 << 30, out)
    assert list(out) == [7, 7]                                     # a refused call writes nothing
    # n == 0: fine, and nothing is touched (not even null pointers)
    assert fn(h, None, 0, 5, 0, None) == 0
    assert fn(h, two, 0, 5, 0, out) == 0 and list(out) == [7, 7]
    assert ctx.grind_many([], 5) == []
    try:
        ctx.grind_many([digest(1)[:31]], 5)
        raise AssertionError("a 31-byte digest was accepted")
    except ValueError:
        pass


def check_largest_call(lib, ctx, pow_bits=4):
    """LMN_GRIND_MANY_MAX digests in one call: one block per digest and launch"""
    ds = [digest(9000 + i) for i in range(GRIND_MANY_MAX)]
    assert ctx.grind_many(ds, pow_bits, 0x4) == [host_nonce(lib, d, pow_bits, 0x4) for d in ds]
