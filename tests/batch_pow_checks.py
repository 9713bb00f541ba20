"""Checks of the lock-step batch library's proof of work on the device, shared by tests/test_batch_pow_emu.py (the emulated
batch library, no GPU) and tests/test_gpu_batch_pow.py (the MI355X).  From LMN_POW_DEVICE_MIN_BITS on the members of a
batch grind in one collective rendezvous (csrc/batch.h): whoever arrives last grinds everybody's digest with
`Context::grind_many` and hands each member its nonce.  Checked: batched proofs are byte-equal to the solo context's and
verify; one grind per batch whatever the nonces, with the lock-step launch and wait counts of the host-grinding batch;
the rounds the leader needs follow from the largest nonce; a member that fails earlier does not disturb the others'
grind; two groups at once; and the batch library's own lmn_ctx_grind / lmn_ctx_grind_many.

Shapes are those of tests/test_batch_emu.py: 64-row Add pies and the KAT pie."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from luminair_amd import backend, synthetic as syn          # noqa: E402
from luminair_amd.batch import BatchPool, BatchProver        # noqa: E402
from luminair_amd.pie import LuminairProof                   # noqa: E402
import grind_many_checks as gm                               # noqa: E402
from test_batch_emu import _pie, _raw_batch                  # noqa: E402

ROUND = gm.ROUND_ONE       # nonces per digest and round under LMN_POW_WINDOW_LOG=11 with at most 8 members


class Env:
    """environment switches that the libraries read when a context / batch is created"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update({k: str(v) for k, v in self.kv.items()})

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _solo(solo_lib, variant, pow_bits):
    cfg = solo_lib.default_config()
    cfg.protocol_variant = variant
    cfg.pow_bits = pow_bits
    return backend.Context(0, cfg, solo_lib), cfg


def _pies(variant, n, seed0=50):
    mk = syn.config2_graph_faithful if variant == backend.VARIANT_PINNED else syn.config2_add_only
    return [_pie(mk(64, seed0 + i)) for i in range(n)]


def _nonce(proof):
    return LuminairProof(proof).to_dict()["proof"]["proof_of_work"]


def _delta(bp, before):
    now = bp.counters()
    return {k: now[k] - before[k] for k in ("launches", "host_waits", "grinds", "grind_rounds")}


def scenario_byte_equal(batch_so, solo_lib, variant, pow_bits):
    """4 members, then 2 in the same object, then 5 members on two worker threads, and the KAT pie: byte-equal to the solo
    context's proofs, which verify under that config"""
    solo, cfg = _solo(solo_lib, variant, pow_bits)
    try:
        pies = _pies(variant, 5) + [_pie(syn.simple_example())]
        want = [solo.prove_tables(p) for p in pies]
    finally:
        solo.close()
    for w in want:
        solo_lib.verify(w, variant, config=cfg)
    bp = BatchProver(0, 4, protocol_variant=variant, library_path=batch_so, pow_bits=pow_bits)
    try:
        c0 = bp.counters()
        assert bp.prove_batch(pies[:4]) == want[:4]
        assert bp.prove_batch(pies[2:4]) == want[2:4]
        assert bp.prove_batch([pies[5]] * 3) == [want[5]] * 3
        assert _delta(bp, c0)["grinds"] == 3                   # one collective per batch
    finally:
        bp.close()
    with Env(LMN_BATCH_THREADS=2):                             # five members on two worker threads: three fibers on one
        bp = BatchProver(0, 5, protocol_variant=variant, library_path=batch_so, pow_bits=pow_bits)
    try:
        assert bp.prove_batch(pies[:5]) == want[:5]
    finally:
        bp.close()


def scenario_rounds_and_lockstep_counts(batch_so, solo_lib, pow_bits, seed0):
    """2^11-nonce windows: the members need different numbers of rounds, and nothing of that shows in the lock-step
    counters - they equal those of the same batch ground on the host (LMN_POW_DEVICE_MIN_BITS=41)"""
    variant = backend.VARIANT_KAT
    pies = _pies(variant, 4, seed0)
    runs = {}
    for min_bits in (0, 41):
        with Env(LMN_POW_WINDOW_LOG=gm.WINDOW_LOG, LMN_POW_DEVICE_MIN_BITS=min_bits):
            bp = BatchProver(0, 4, protocol_variant=variant, library_path=batch_so, pow_bits=pow_bits)
        try:
            c0 = bp.counters()
            proofs = bp.prove_batch(pies)
            runs[min_bits] = (proofs, _delta(bp, c0))
        finally:
            bp.close()
    (dev, cd), (host, ch) = runs[0], runs[41]
    assert dev == host
    nonces = [_nonce(p) for p in dev]
    rounds = [n // ROUND + 1 for n in nonces]
    assert len(set(rounds)) > 1 and max(rounds) >= 2, nonces   # the shapes were chosen for this: see the callers
    assert ch["grinds"] == 0 and ch["grind_rounds"] == 0, ch
    assert cd["grinds"] == 1 and cd["grind_rounds"] >= 2, cd
    # every round examines ROUND nonces of every pending digest: the leader waits until the largest nonce is covered
    assert cd["grind_rounds"] == max(rounds), (cd, nonces)
    assert (cd["launches"], cd["host_waits"]) == (ch["launches"], ch["host_waits"]), (cd, ch)
    solo, cfg = _solo(solo_lib, variant, pow_bits)
    try:
        assert dev == [solo.prove_tables(p) for p in pies]
    finally:
        solo.close()


def scenario_bad_member_fails_alone(batch_so, solo_lib, pow_bits):
    variant = backend.VARIANT_PINNED
    solo, _ = _solo(solo_lib, variant, pow_bits)
    try:
        good = _pies(variant, 4, 7)
        want = [solo.prove_tables(p) for p in good]
    finally:
        solo.close()
    bp = BatchProver(0, 4, protocol_variant=variant, library_path=batch_so, pow_bits=pow_bits)
    try:
        bad = [(k, r.copy(), n) for k, r, n in good[2]]
        bad[0][1][5, 11] = (int(bad[0][1][5, 11]) + 1) % ((1 << 31) - 1)     # pie 2 violates its constraints
        c0 = bp.counters()
        rc, rcs, out = _raw_batch(bp, good[:2] + [bad] + good[3:])
        assert rc == backend.ERR_CONSTRAINTS and rcs == [0, 0, backend.ERR_CONSTRAINTS, 0], (rc, rcs)
        assert [out[i] for i in (0, 1, 3)] == [want[i] for i in (0, 1, 3)] and out[2] is None
        assert _delta(bp, c0)["grinds"] == 1                   # the three others ground together, once
        assert bp.prove_batch(good) == want                    # the slot proves correctly in the next batch
        assert _delta(bp, c0)["grinds"] == 2
    finally:
        bp.close()


def scenario_two_groups(batch_so, solo_lib, pow_bits, slots=3, n_pies=8):
    variant = backend.VARIANT_PINNED
    solo, _ = _solo(solo_lib, variant, pow_bits)
    try:
        pies = _pies(variant, n_pies, 70)
        want = [solo.prove_tables(p) for p in pies]
    finally:
        solo.close()
    pool = BatchPool(0, groups=2, slots=slots, protocol_variant=variant, library_path=batch_so, pow_bits=pow_bits)
    try:
        assert pool.prove_many(pies) == want
    finally:
        pool.close()


def scenario_context_entry_points(batch_so, solo_lib, pow_bits):
    """lmn_ctx_grind, lmn_ctx_grind_many and a solo lmn_prove of the batch library itself: a thread outside any batch is a
    group of one and grinds through the same collective"""
    lib = backend.Library(batch_so)
    with Env(LMN_POW_WINDOW_LOG=gm.WINDOW_LOG):
        cfg = lib.default_config()
        cfg.pow_bits = pow_bits
        ctx = backend.Context(0, cfg, lib)
    try:
        for variant in gm.FORMS:
            ds = [gm.digest(300 + i) for i in range(5)]
            want = [gm.host_nonce(solo_lib, d, pow_bits, variant) for d in ds]
            assert ctx.grind_many(ds, pow_bits, variant) == want
            assert ctx.grind(ds[0], pow_bits, variant) == want[0]
        gm.check_refusals(lib, ctx)
        pie = _pies(backend.VARIANT_KAT, 1, 90)[0]
        got = ctx.prove_tables(pie)
    finally:
        ctx.close()
    solo, _ = _solo(solo_lib, backend.VARIANT_KAT, pow_bits)
    try:
        assert got == solo.prove_tables(pie)
    finally:
        solo.close()
