"""The device proof-of-work grind (k_pow_grind, `Context.grind` / lmn_ctx_grind, and the prover's grind from
LMN_POW_DEVICE_MIN_BITS on) through the TEST-ONLY emulation build (tests/emu, one fiber per GPU thread): the nonce equals
the host loop's (`Library.grind` = lmn_op_grind) and the oracle's for all three proof-of-work forms, with windows small
enough (LMN_POW_WINDOW_LOG) that several windows, skipped blocks, later waits and hits in later windows all occur, and whole
proofs are byte-equal whichever path ground.  The same checks on the MI355X: tests/test_gpu_pow.py."""
import hashlib
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from luminair_amd import backend, synthetic as syn                # noqa: E402
from oracle.channel import Blake2sChannel, ProtocolVariant        # noqa: E402

EMU = os.path.join(ROOT, "tests", "emu", "libluminair_emu.so")
# the three forms: bare compression (KAT), blake2s(digest || nonce), blake2s(prefixed digest || nonce)
FORMS = [backend.VARIANT_KAT, 0x4, 0x10]
WINDOW_LOG = 11                  # the smallest window: one block of 2048 nonces per launch, 8 launches per wait


def _emu_library():
    csrc = os.path.join(ROOT, "luminair_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".cpp", ".h"))]
    srcs += [os.path.join(ROOT, "tests", "emu", f) for f in ("emu_runtime.cpp", "build_emu.sh")]
    if not os.path.exists(EMU) or any(os.path.getmtime(s) > os.path.getmtime(EMU) for s in srcs):
        r = subprocess.run([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return backend.Library(EMU)


@pytest.fixture(scope="module")
def emu_lib():
    return _emu_library()


@pytest.fixture
def small_window_ctx(emu_lib, monkeypatch):
    monkeypatch.setenv("LMN_POW_WINDOW_LOG", str(WINDOW_LOG))   # read when the context is created
    ctx = backend.Context(0, emu_lib.default_config(), emu_lib)
    yield ctx
    ctx.close()


def _digest(i):
    return hashlib.sha256(b"pow grind digest %d" % i).digest()


def _oracle_grind(digest, pow_bits, variant):
    ch = Blake2sChannel(ProtocolVariant(variant))
    ch.digest = digest
    return ch.grind(pow_bits)


@pytest.mark.parametrize("variant", FORMS)
@pytest.mark.parametrize("pow_bits", [0, 1, 5, 10, 12])
def test_device_grind_equals_host_and_oracle(emu_lib, small_window_ctx, variant, pow_bits):
    for i in range(3):
        d = _digest(100 * pow_bits + i)
        got = small_window_ctx.grind(d, pow_bits, variant)
        assert got == emu_lib.grind(d, pow_bits, variant)
        assert got == _oracle_grind(d, pow_bits, variant)


@pytest.mark.parametrize("variant", FORMS)
def test_device_grind_over_several_waits(emu_lib, small_window_ctx, variant):
    """pow_bits 16 with 2^11-nonce windows: the minimum lies beyond the first wait's 8 windows for some digests"""
    got = []
    for i in range(6):
        d = _digest(1000 + i)
        n = small_window_ctx.grind(d, 16, variant)
        assert n == emu_lib.grind(d, 16, variant)
        got.append(n)
    assert max(got) >= 8 << WINDOW_LOG, got


def test_default_window_and_argument_checks(emu_lib):
    ctx = backend.Context(0, emu_lib.default_config(), emu_lib)
    try:
        d = _digest(7)
        assert ctx.grind(d, 12, backend.VARIANT_PINNED) == emu_lib.grind(d, 12, backend.VARIANT_PINNED)
        with pytest.raises(backend.LuminairBackendError):
            ctx.grind(d, 41, backend.VARIANT_KAT)
        with pytest.raises(backend.LuminairBackendError):
            ctx.grind(d, 5, 1 << 30)
        with pytest.raises(ValueError):
            ctx.grind(d[:31], 5, backend.VARIANT_KAT)
        rc = emu_lib.lib.lmn_ctx_grind(None, d, 5, 0, None)
        assert rc == backend.ERR_INVALID_ARGUMENT
    finally:
        ctx.close()


@pytest.mark.parametrize("variant", [backend.VARIANT_KAT, 0x4, backend.VARIANT_PINNED])
def test_whole_proof_same_bytes_on_either_grind_path(emu_lib, monkeypatch, variant):
    monkeypatch.setenv("LMN_POW_WINDOW_LOG", str(WINDOW_LOG))
    tabs = syn.config2_add_only(64, 11) if variant != backend.VARIANT_PINNED else syn.config2_graph_faithful(64, 11)
    proofs = []
    for min_bits in ("0", "41"):                    # device grind at every pow_bits / never
        monkeypatch.setenv("LMN_POW_DEVICE_MIN_BITS", min_bits)
        cfg = emu_lib.default_config()
        cfg.protocol_variant = variant
        cfg.pow_bits = 12
        ctx = backend.Context(0, cfg, emu_lib)
        try:
            proofs.append(ctx.prove_tables([(k, r, len(r)) for k, r in tabs]))
        finally:
            ctx.close()
    assert proofs[0] == proofs[1]
    emu_lib.verify(proofs[0], variant, config=cfg)
