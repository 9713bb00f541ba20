"""The proof-of-work grind on the MI355X (k_pow_grind): `Context.grind` (lmn_ctx_grind) returns the host loop's nonce for
all three proof-of-work forms, including a nonce above 2^32; proofs ground on the device are byte-equal to host-ground ones
and accepted by the verifier; and a proof at pow_bits 26 - about 9 s of host grinding - finishes in well under a second."""
import hashlib
import os
import time

import pytest

import luminair_amd
from luminair_amd import backend, synthetic as syn

pytestmark = pytest.mark.gpu

FORMS = [backend.VARIANT_KAT, 0x4, 0x10]      # bare compression, blake2s(digest || nonce), prefixed double hash

# Minimal nonce above 2^32 at pow_bits 33, KAT form, digest = sha256(b"luminair pow vector 0").  Found, and shown minimal
# (every smaller nonce examined: 282 s on 16 threads), on the CPU with tools/pow_exhaustive.cpp:
#   pow_exhaustive 9a0631261ec4602bf4aaa19a02ef645376e660b496870667c10cccdb891f23f7 33 0 16
PINNED_DIGEST = hashlib.sha256(b"luminair pow vector 0").digest()
PINNED_BITS, PINNED_VARIANT, PINNED_NONCE = 33, backend.VARIANT_KAT, 15906534353


def _digest(i):
    return hashlib.sha256(b"pow grind digest %d" % i).digest()


@pytest.fixture(scope="module")
def ctx(hip_lib_path):
    c = backend.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("variant", FORMS)
@pytest.mark.parametrize("pow_bits", [0, 8, 16, 20])
def test_gpu_grind_equals_host_grind(ctx, variant, pow_bits):
    lib = backend.default_library()
    for i in range(3 if pow_bits < 20 else 2):
        d = _digest(1000 * pow_bits + i)
        assert ctx.grind(d, pow_bits, variant) == lib.grind(d, pow_bits, variant)


def test_gpu_grind_nonce_above_2_32(ctx):
    assert PINNED_NONCE > 1 << 32
    assert ctx.grind(PINNED_DIGEST, PINNED_BITS, PINNED_VARIANT) == PINNED_NONCE


def _prove(tabs, variant, pow_bits, device_min_bits=None, n_queries=3):
    old = os.environ.get("LMN_POW_DEVICE_MIN_BITS")
    if device_min_bits is not None:
        os.environ["LMN_POW_DEVICE_MIN_BITS"] = str(device_min_bits)   # read when the context is created
    try:
        p = luminair_amd.Prover(0, protocol_variant=variant, pow_bits=pow_bits, n_queries=n_queries)
    finally:
        if old is None:
            os.environ.pop("LMN_POW_DEVICE_MIN_BITS", None)
        else:
            os.environ["LMN_POW_DEVICE_MIN_BITS"] = old
    try:
        t = time.perf_counter()
        proof = p.ctx.prove_tables([(k, r, len(r)) for k, r in tabs])
        return proof, time.perf_counter() - t, p.ctx.config
    finally:
        p.ctx.close()


@pytest.mark.parametrize("pow_bits", [20, 24])
@pytest.mark.parametrize("variant", [backend.VARIANT_KAT, 0x4, backend.VARIANT_PINNED])
def test_gpu_proof_device_grind_equals_host_grind(hip_lib_path, pow_bits, variant):
    tabs = syn.config2_add_only(1 << 12, 3) if variant != backend.VARIANT_PINNED else syn.config2_graph_faithful(1 << 12, 3)
    dev, _, cfg = _prove(tabs, variant, pow_bits, device_min_bits=0)
    host, _, _ = _prove(tabs, variant, pow_bits, device_min_bits=41)
    assert dev == host
    backend.default_library().verify(dev, variant, config=cfg)


def test_gpu_prover_pool_device_grind_equals_lmn_prove(hip_lib_path):
    pies = [luminair_amd.LuminairPie.from_tables(syn.config2_add_only(1 << 12, 20 + i)) for i in range(6)]
    pool = luminair_amd.ProverPool(0, 3, pow_bits=20)
    try:
        got = [p.to_bincode() for p in pool.prove_many(pies)]
    finally:
        pool.close()
    solo = luminair_amd.Prover(0, pow_bits=20)
    try:
        assert got == [solo.prove(p).to_bincode() for p in pies]
    finally:
        solo.ctx.close()


def test_gpu_proof_pow_26_under_a_second(hip_lib_path):
    """BASELINE config 2a size (one Add table of 2^20 rows), 70 queries, pow_bits 26: ~2^26 nonces, ~9 s on the host loop"""
    tabs = syn.config2_add_only(1 << 20, 5)
    _prove(tabs, backend.VARIANT_KAT, 26, n_queries=70)          # warm-up: twiddles, code objects, arena
    proof, secs, cfg = _prove(tabs, backend.VARIANT_KAT, 26, n_queries=70)
    backend.default_library().verify(proof, backend.VARIANT_KAT, config=cfg)
    assert secs < 1.0, secs
