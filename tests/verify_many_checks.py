"""Checks of proofs verified in batches (`lmn_verify_many`; luminair_amd.backend.Library.verify_many), shared by the
emulation suite (tests/test_verify_many_emu.py) and the GPU suite (tests/test_gpu_verify_many.py), both in process.
Every comparison is exact.  The reference of every return code is `lmn_verify_with_config` on the same bytes, the reference
of the three device bits (TREE_DECOMMIT, FRI_DECOMMIT, FRI_FOLDS) is `lmn_verify_diagnose`; both are the host verifier.
Proofs come from the oracle prover and the known-answer proof; fields are edited through oracle.proof."""
import copy
import ctypes as C
import os
import random
from dataclasses import dataclass
from typing import Optional

import numpy as np

from luminair_amd import backend, synthetic as syn
from oracle.channel import ProtocolVariant
from oracle.field import P, QM31
from oracle.proof import from_bincode, to_bincode
from oracle.prover import PcsConfig, prove

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, VERIFICATION, INV = backend.LMN_OK, backend.ERR_VERIFICATION, backend.ERR_INVALID_ARGUMENT
TREE, FRI_DEC, FOLDS, SHAPE = (backend.CHECK_TREE_DECOMMIT, backend.CHECK_FRI_DECOMMIT, backend.CHECK_FRI_FOLDS,
                               backend.CHECK_SHAPE)
DEVICE_BITS = TREE | FRI_DEC | FOLDS
C_DEVICE, C_STAGE2, C_LAUNCHES, C_WAITS = (backend.COUNTER_VERIFY_DEVICE, backend.COUNTER_VERIFY_STAGE2,
                                           backend.COUNTER_VERIFY_LAUNCHES, backend.COUNTER_VERIFY_WAITS)
CHUNK_PROOFS = 256   # VM_CHUNK_PROOFS (verifier.cpp)
MAX_BUCKETS = 4      # VM_MAX_BUCKETS


@dataclass(frozen=True)
class Shape:
    name: str
    variant: int = 0
    pow_bits: int = 5
    log_blowup: int = 1
    log_last_layer: int = 0
    n_queries: int = 3

    @property
    def group(self):
        """proofs of one group can share a call: the verifier's config is the call's"""
        return (self.variant, self.pow_bits, self.log_blowup, self.log_last_layer, self.n_queries)


PINNED = int(ProtocolVariant.PINNED)
SHAPES = [Shape("kat"),                                   # domain 2^6, 3 queries, tree 0 without columns
          Shape("chain_70_queries", pow_bits=3, n_queries=70),   # more queries than some layers have nodes
          Shape("config3_mixed"),                         # three sizes with gaps, a tree-1 node of two compression blocks
          Shape("sin", variant=PINNED),                   # tree 0 has columns, of another size than the rest
          Shape("less_than", variant=PINNED),             # 22 columns, 7 relations: two batches per size
          Shape("blowup_2", log_blowup=2),
          Shape("blowup_3", log_blowup=3),
          Shape("last_layer_2", log_last_layer=2),
          Shape("mix_u64_hashed", variant=int(ProtocolVariant.MIX_U64_HASHED))]
# further claims under the default config, for the call that exceeds the bucket cap
EXTRA = [Shape("chain_40"), Shape("chain_300"), Shape("mul_add_20")]
_TABLES = {
    "chain_70_queries": lambda: (syn.chain_graph(40, 2), None),
    "config3_mixed": lambda: (syn.config3_mixed(10, 8, 6, 5), None),
    "sin": lambda: syn.activation_graph(30, 4, names=("sin",), ranges={"sin": (-300, 200)}),
    "less_than": lambda: (syn.less_than_graph(100, 3), None),
    "blowup_2": lambda: (syn.chain_graph(20, 6), None),
    "blowup_3": lambda: (syn.chain_graph(20, 7), None),
    "last_layer_2": lambda: (syn.chain_graph(40, 2), None),
    "mix_u64_hashed": lambda: (syn.chain_graph(20, 8), None),
    "chain_40": lambda: (syn.chain_graph(40, 2), None),
    "chain_300": lambda: (syn.chain_graph(300, 3), None),
    "mul_add_20": lambda: (syn.chain_graph(20, 9, with_recip=False), None),
}
_proofs = {}


def proof_of(shape: Shape) -> bytes:
    """the shape's proof, made once by the oracle and left unchanged"""
    if shape.name not in _proofs:
        if shape.name == "kat":
            with open(os.path.join(ROOT, "tests", "golden", "kat_simple", "proof"), "rb") as f:
                _proofs[shape.name] = f.read()
        else:
            tabs, luts = _TABLES[shape.name]()
            cfg = PcsConfig(shape.pow_bits, shape.log_blowup, shape.log_last_layer, shape.n_queries)
            _proofs[shape.name] = to_bincode(prove([(k, np.asarray(r).astype(np.uint64)) for k, r in tabs], cfg,
                                                   ProtocolVariant(shape.variant), luts=luts))
    return _proofs[shape.name]


def slots_of(shape: Shape) -> int:
    return 17 if shape.variant & backend.PV_CLAIM17 else 8


def config_of(lib, shape: Shape):
    cfg = lib.default_config()
    cfg.pow_bits, cfg.log_blowup, cfg.log_last_layer, cfg.n_queries = (shape.pow_bits, shape.log_blowup, shape.log_last_layer,
                                                                        shape.n_queries)
    cfg.protocol_variant = shape.variant
    return cfg


_ctxs = {}


def ctx_for(lib):
    """one context per library, kept for the session (verify_many takes the verifier's config per call)"""
    if id(lib) not in _ctxs:
        _ctxs[id(lib)] = backend.Context(0, None, lib)
    return _ctxs[id(lib)]


def counters(ctx):
    return [ctx.counter(k) for k in (C_DEVICE, C_STAGE2, C_LAUNCHES, C_WAITS)]


# ---- the references: the host verifier on the same bytes
def ref_rc(lib, proof: bytes, cfg) -> int:
    return int(lib.lib.lmn_verify_with_config(proof, len(proof), None, C.byref(cfg)))


def ref_diagnose(lib, proof: bytes, cfg):
    """(diagnose ran to its end, checks_failed)"""
    rc, rep = lib.diagnose(proof, cfg.protocol_variant, cfg)
    return rc == OK, int(rep.checks_failed)


# ------------------------------------------------------------------------------------------------ accepted proofs
def check_accepted_alone(lib, shape: Shape):
    ctx, cfg, proof = ctx_for(lib), config_of(lib, shape), proof_of(shape)
    assert ref_rc(lib, proof, cfg) == OK, shape.name
    before = counters(ctx)
    (r,) = lib.verify_many([proof], config=cfg, ctx=ctx)
    assert (r.ok, r.code, r.checks_failed, r.stage) == (True, OK, 0, 1), (shape.name, r)
    after = counters(ctx)
    # one proof: one bucket, two launches, one wait
    assert [a - b for a, b in zip(after, before)] == [1, 0, 2, 1], (shape.name, before, after)


def check_accepted_together(lib):
    """the proofs of every config in one call each: several buckets behind one wait"""
    ctx = ctx_for(lib)
    groups = {}
    for s in SHAPES:
        groups.setdefault(s.group, []).append(s)
    assert max(len(g) for g in groups.values()) >= 2
    for shapes in groups.values():
        assert len(shapes) <= MAX_BUCKETS
        cfg = config_of(lib, shapes[0])
        before = counters(ctx)
        res = lib.verify_many([proof_of(s) for s in shapes], config=cfg, ctx=ctx)
        for s, r in zip(shapes, res):
            assert (r.ok, r.code, r.checks_failed, r.stage) == (True, OK, 0, 1), (s.name, r)
        after = counters(ctx)
        assert [a - b for a, b in zip(after, before)] == [len(shapes), 0, 2 * len(shapes), 1], (before, after)


def check_accepted_300_copies(lib):
    """more proofs than a chunk holds: two chunks, a wait each, every copy accepted at its own index"""
    ctx, shape = ctx_for(lib), SHAPES[0]
    n = 300
    assert n > CHUNK_PROOFS
    before = counters(ctx)
    res = lib.verify_many([proof_of(shape)] * n, config=config_of(lib, shape), ctx=ctx)
    assert len(res) == n and all((r.code, r.checks_failed, r.stage) == (OK, 0, 1) for r in res)
    after = counters(ctx)
    assert [a - b for a, b in zip(after, before)] == [n, 0, 4, 2], (before, after)


# ------------------------------------------------------------------------------------------------ the tamper matrix
def _bump_hash(h: bytes) -> bytes:
    return bytes([h[0] ^ 1]) + h[1:]


def _bump_m31(v: int) -> int:
    return (v + 1) % P


def _bump_qm31(q: QM31) -> QM31:
    a, b, c, d = q.v
    return QM31(a, b, (c + 1) % P, d)


def _lists_of(p):
    """(name, getter of the list inside a proof object, the element bump, a fresh element) for every list that no
    transcript step mixes: the queried values, every tree's two witness lists, every FRI layer's witness"""
    sp = p.proof
    out = []
    for t in range(4):
        out.append(("queried_values[%d]" % t, lambda q, t=t: q.proof.queried_values[t], _bump_m31, 5))
        out.append(("decommitments[%d].hash_witness" % t, lambda q, t=t: q.proof.decommitments[t].hash_witness, _bump_hash, bytes(32)))
        out.append(("decommitments[%d].column_witness" % t, lambda q, t=t: q.proof.decommitments[t].column_witness, _bump_m31, 5))
    layers = [("first_layer", lambda q: q.proof.first_layer)]
    for i in range(len(sp.inner_layers)):
        layers.append(("inner_layers[%d]" % i, lambda q, i=i: q.proof.inner_layers[i]))
    for name, layer in layers:
        out.append((name + ".fri_witness", lambda q, layer=layer: layer(q).fri_witness, _bump_qm31, QM31(1, 2, 3, 4)))
        out.append((name + ".decommitment.hash_witness", lambda q, layer=layer: layer(q).decommitment.hash_witness, _bump_hash, bytes(32)))
        out.append((name + ".decommitment.column_witness", lambda q, layer=layer: layer(q).decommitment.column_witness, _bump_m31, 5))
    return out


def _same(a, b):
    return (a.v == b.v) if isinstance(a, QM31) else a == b


def tamper_cases(shape: Shape):
    """[(what, bytes)]: per list - one word changed (first, middle, last element), the last element dropped, one appended,
    two neighbours swapped (the swap of two equal elements is no edit and is left out)"""
    base = from_bincode(proof_of(shape), slots_of(shape))
    cases = []
    for name, get, bump, fresh in _lists_of(base):
        n = len(get(base))
        edits = [("change %d" % i, lambda l, i=i: l.__setitem__(i, bump(l[i]))) for i in sorted({0, n // 2, n - 1}) if n]
        if n:
            edits.append(("drop last", lambda l: l.pop()))
        edits.append(("append", lambda l: l.append(fresh)))
        swap = next((i for i in range(n - 1) if not _same(get(base)[i], get(base)[i + 1])), None)
        if swap is not None:
            edits.append(("swap %d, %d" % (swap, swap + 1), lambda l, i=swap: l.__setitem__(slice(i, i + 2), [l[i + 1], l[i]])))
        for what, edit in edits:
            q = copy.deepcopy(base)
            edit(get(q))
            cases.append(("%s: %s %s" % (shape.name, name, what), to_bincode(q)))
    return cases


_tamper = {}


def tamper_reference(lib, shape: Shape):
    """the matrix with the host verifier's verdicts, computed once per shape: [(what, bytes, rc, diagnose ended, bits)].
    The reference rejects every case with a device bit or SHAPE set - asserted here, before anything runs on a device."""
    if shape.name not in _tamper:
        cfg = config_of(lib, shape)
        rows = []
        for what, b in tamper_cases(shape):
            rc = ref_rc(lib, b, cfg)
            ended, bits = ref_diagnose(lib, b, cfg)
            assert rc == VERIFICATION, (what, rc)
            assert bits & (DEVICE_BITS | SHAPE) and not bits & ~(DEVICE_BITS | SHAPE), (what, hex(bits))
            assert ended == (not bits & SHAPE), (what, ended, hex(bits))
            rows.append((what, b, rc, ended, bits))
        _tamper[shape.name] = rows
    return _tamper[shape.name]


TAMPER_SHAPES = [SHAPES[0], SHAPES[2]]


def check_tamper_reference(lib, shape: Shape):
    rows = tamper_reference(lib, shape)
    base = from_bincode(proof_of(shape), slots_of(shape))
    assert len(rows) >= 2 * len(_lists_of(base))
    seen = 0
    for _, _, _, _, bits in rows:
        seen |= bits
    assert seen & TREE and seen & FRI_DEC and seen & FOLDS and seen & SHAPE, hex(seen)


def check_tamper_matrix(lib, shape: Shape):
    ctx, cfg = ctx_for(lib), config_of(lib, shape)
    rows = tamper_reference(lib, shape)
    before = counters(ctx)
    res = lib.verify_many([b for _, b, _, _, _ in rows], config=cfg, ctx=ctx)
    after = counters(ctx)
    assert all(r.stage == 1 for r in res), [w for (w, *_), r in zip(rows, res) if r.stage != 1]
    assert after[0] - before[0] == len(rows) and after[1] == before[1], (before, after)
    for (what, _, rc, ended, bits), r in zip(rows, res):
        assert r.code == rc and not r.ok, (what, r)
        if ended:
            assert r.checks_failed == bits & DEVICE_BITS, (what, hex(r.checks_failed), hex(bits))
        else:
            assert r.checks_failed & SHAPE, (what, hex(r.checks_failed), hex(bits))
    text = lib.lib.lmn_last_error(ctx.handle).decode()
    assert "StwoVerifierError" in text, text   # the first rejection in index order


# ------------------------------------------------------------------------------------------------ front failures
def front_cases(shape: Shape):
    """one edit per host check: [(what, bytes)]"""
    base = from_bincode(proof_of(shape), slots_of(shape))
    out = []

    def edited(what, f):
        q = copy.deepcopy(base)
        f(q)
        out.append((what, to_bincode(q)))
    k = next(i for i, c in enumerate(base.interaction_claim) if c is not None)
    edited("a claimed sum", lambda q: q.interaction_claim.__setitem__(k, _bump_qm31(q.interaction_claim[k])))
    edited("a sampled value", lambda q: q.proof.sampled_values[1][0].__setitem__(0, _bump_qm31(q.proof.sampled_values[1][0][0])))
    edited("a commitment", lambda q: q.proof.commitments.__setitem__(2, _bump_hash(q.proof.commitments[2])))
    edited("a last-layer coefficient", lambda q: q.proof.last_layer_coeffs.__setitem__(0, _bump_qm31(q.proof.last_layer_coeffs[0])))
    edited("the nonce", lambda q: setattr(q.proof, "proof_of_work", q.proof.proof_of_work + 1))
    edited("a config word", lambda q: setattr(q.proof, "n_queries", q.proof.n_queries + 1))
    out.append(("trailing bytes", proof_of(shape) + b"\0"))
    return out


def check_front_failures(lib, shape: Shape):
    ctx, cfg = ctx_for(lib), config_of(lib, shape)
    cases = front_cases(shape)
    want = [ref_rc(lib, b, cfg) for _, b in cases]
    assert all(rc != OK for rc in want), want
    assert {backend.ERR_INVALID_LOGUP, VERIFICATION, backend.ERR_SERIALIZATION} <= set(want), want
    before = counters(ctx)
    res = lib.verify_many([b for _, b in cases], config=cfg, ctx=ctx)
    assert counters(ctx) == before      # nothing reached the device stage: no launch, no wait
    for (what, b), rc, r in zip(cases, want, res):
        assert (r.code, r.stage) == (rc, 0) and r.checks_failed, (what, r, rc)
        if rc == backend.ERR_SERIALIZATION:
            assert r.checks_failed == backend.CHECK_PARSE, (what, hex(r.checks_failed))
        else:   # the bit of the check that failed first is among those diagnose sees fail
            _, bits = ref_diagnose(lib, b, cfg)
            assert r.checks_failed & bits and not r.checks_failed & (r.checks_failed - 1), (what, hex(r.checks_failed), hex(bits))


# ------------------------------------------------------------------------------------------------ mixed calls
def check_mixed_call(lib):
    """accepted, front-rejected, device-rejected and stage-2 proofs in one call: results at their own indices; stage 2 is
    reached through the bucket cap (the fifth and sixth claim of the call)"""
    ctx = ctx_for(lib)
    default = [SHAPES[0], SHAPES[2]] + EXTRA          # five claims under the default config
    assert len(default) == MAX_BUCKETS + 1 and len({s.group for s in default}) == 1
    cfg = config_of(lib, default[0])
    kat = default[0]
    bad_device = tamper_reference(lib, kat)[0]      # (what, bytes, rc, ended, bits)
    bad_front = front_cases(kat)[4][1]              # the nonce
    stage2_bad = tamper_cases(default[-1])[0][1]    # a rejected proof of the claim beyond the cap
    proofs = [proof_of(default[0]), bad_front, proof_of(default[1]), bad_device[1], proof_of(default[2]), proof_of(default[3]),
              proof_of(default[4]), stage2_bad, proof_of(default[0]), proof_of(default[4])]
    want_stage = [1, 0, 1, 1, 1, 1, 2, 2, 1, 2]
    want_rc = [ref_rc(lib, b, cfg) for b in proofs]
    assert want_rc == [OK, VERIFICATION, OK, VERIFICATION, OK, OK, OK, VERIFICATION, OK, OK], want_rc
    before = counters(ctx)
    res = lib.verify_many(proofs, config=cfg, ctx=ctx)
    after = counters(ctx)
    assert [r.stage for r in res] == want_stage, res
    assert [r.code for r in res] == want_rc, res
    assert res[3].checks_failed == bad_device[4] & DEVICE_BITS and res[1].checks_failed == backend.CHECK_POW, res
    assert res[7].checks_failed and all(r.checks_failed == 0 for r in res if r.ok)
    # six proofs of four buckets on the device: two launches per bucket, one chunk, one wait; three stage-2 proofs
    assert [a - b for a, b in zip(after, before)] == [6, 3, 2 * MAX_BUCKETS, 1], (before, after)
    assert "ProofOfWork" in lib.lib.lmn_last_error(ctx.handle).decode()   # index 1: the first rejection


# ------------------------------------------------------------------------------------------------ refusals
def check_refusals(lib):
    ctx, shape = ctx_for(lib), SHAPES[0]
    cfg, proof = config_of(lib, shape), proof_of(shape)
    L = lib.lib
    ptrs = (C.c_char_p * 1)(proof)
    lens = (C.c_size_t * 1)(len(proof))
    res = (backend.LmnVerifyResult * 1)()

    def usable():
        (r,) = lib.verify_many([proof], config=cfg, ctx=ctx)
        assert (r.code, r.stage) == (OK, 1), r
    before = counters(ctx)
    assert L.lmn_verify_many(None, ptrs, lens, 1, None, C.byref(cfg), res) == INV
    for args, word in (((None, lens, 1, None, C.byref(cfg), res), "proofs"), ((ptrs, None, 1, None, C.byref(cfg), res), "lens"),
                       ((ptrs, lens, 1, None, C.byref(cfg), None), "results")):
        assert L.lmn_verify_many(ctx.handle, *args) == INV
        assert word in L.lmn_last_error(ctx.handle).decode(), word
    # n = 0 touches nothing, whatever else is passed
    res[0].rc, res[0].stage = 77, 9
    assert L.lmn_verify_many(ctx.handle, None, None, 0, None, None, None) == OK
    assert L.lmn_verify_many(ctx.handle, ptrs, lens, 0, None, C.byref(cfg), res) == OK and (res[0].rc, res[0].stage) == (77, 9)
    bad = config_of(lib, shape)
    bad.log_blowup = 9
    assert L.lmn_verify_many(ctx.handle, ptrs, lens, 1, None, C.byref(bad), res) == INV
    assert "PCS config" in L.lmn_last_error(ctx.handle).decode()
    bad = config_of(lib, shape)
    bad.protocol_variant = 1 << 30
    assert L.lmn_verify_many(ctx.handle, ptrs, lens, 1, None, C.byref(bad), res) == INV
    assert counters(ctx) == before
    usable()
    # expected = NULL: PcsConfig::default(), variant 0
    assert L.lmn_verify_many(ctx.handle, ptrs, lens, 1, None, None, res) == OK and (res[0].rc, res[0].stage) == (OK, 1)
    # a null proof among the proofs is that proof's own answer, as lmn_verify_with_config gives it
    two = (C.c_char_p * 2)(None, proof)
    lens2 = (C.c_size_t * 2)(0, len(proof))
    res2 = (backend.LmnVerifyResult * 2)()
    assert L.lmn_verify_many(ctx.handle, two, lens2, 2, None, C.byref(cfg), res2) == OK
    assert (res2[0].rc, res2[0].stage) == (INV, 0) and (res2[1].rc, res2[1].stage) == (OK, 1)


def check_sharded_context_refused(lib):
    ctx, shape = ctx_for(lib), SHAPES[0]
    cfg, proof = config_of(lib, shape), proof_of(shape)
    ctx.set_shard(0, 1, lambda *a: None)
    try:
        try:
            lib.verify_many([proof], config=cfg, ctx=ctx)
        except backend.LuminairBackendError as e:
            assert e.code == INV and "sharded" in str(e) and "verify_many" in str(e), (e.code, str(e))
        else:
            raise AssertionError("a sharded context verified proofs")
    finally:
        ctx.clear_shard()
    (r,) = lib.verify_many([proof], config=cfg, ctx=ctx)
    assert (r.code, r.stage) == (OK, 1), r


def check_batch_library(batch_so):
    """the same entry in the lock-step library, on a thread outside any batch"""
    lib = backend.Library(batch_so)
    ctx = backend.Context(0, None, lib)
    try:
        shape = SHAPES[2]
        bad = tamper_reference(lib, SHAPES[0])[0]
        res = lib.verify_many([proof_of(shape), proof_of(SHAPES[0]), bad[1]], config=config_of(lib, shape), ctx=ctx)
        assert [(r.code, r.stage) for r in res] == [(OK, 1), (OK, 1), (VERIFICATION, 1)], res
        assert res[2].checks_failed == bad[4] & DEVICE_BITS
    finally:
        ctx.close()


def check_python_entry_points(lib):
    """luminair_amd.verify_many next to verify, on proof objects or bytes"""
    import luminair_amd
    shape = SHAPES[0]
    bad = tamper_reference(lib, shape)[0][1]
    res = luminair_amd.verify_many([proof_of(shape), bad], None, library=lib, ctx=ctx_for(lib))
    assert [(r.ok, r.code, r.stage) for r in res] == [(True, OK, 1), (False, VERIFICATION, 1)], res
    assert luminair_amd.verify_many([], None, library=lib, ctx=ctx_for(lib)) == []


# ------------------------------------------------------------------------------------------------ fuzz (emulation only)
def check_fuzz(lib, n_cases=800):
    """random bit flips, truncations, length-field overwrites and insertions of the known-answer proof, as
    test_product_verifier_survives_fuzzed_proofs makes them: verdict parity with lmn_verify, nothing accepted"""
    ctx, shape = ctx_for(lib), SHAPES[0]
    kat = proof_of(shape)
    rnd = random.Random(7)
    by_variant = {0: [], 1: []}
    for it in range(n_cases):
        b = bytearray(kat)
        mode = it % 4
        if mode == 0:
            for _ in range(rnd.randint(1, 4)):
                b[rnd.randrange(len(b))] ^= 1 << rnd.randrange(8)
        elif mode == 1:
            b = b[:rnd.randrange(len(b))]
        elif mode == 2:
            i = rnd.randrange(len(b) - 8)
            b[i:i + 8] = rnd.getrandbits(64).to_bytes(8, "little")
        else:
            i = rnd.randrange(len(b))
            b[i:i] = bytes(rnd.getrandbits(8) for _ in range(rnd.randint(1, 64)))
        by_variant[rnd.choice([0, 0, 0, 1])].append(bytes(b))
    device = 0
    for variant, proofs in by_variant.items():
        cfg = config_of(lib, shape)
        cfg.protocol_variant = variant
        want = [ref_rc(lib, b, cfg) for b in proofs]
        res = lib.verify_many(proofs, config=cfg, ctx=ctx)
        assert [r.code for r in res] == want, [(i, r, w) for i, (r, w) in enumerate(zip(res, want)) if r.code != w][:5]
        assert not any(r.ok for r in res)
        device += sum(r.stage == 1 for r in res)
    assert device > 0    # some cases pass the front and are rejected by the device stage
