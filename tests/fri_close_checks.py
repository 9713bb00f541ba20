"""The close of the FRI transcript on the device (`lmn_col_fri_close` = phase_fri.cpp `enqueue_fri_close` / `finish_fri_close`:
k_fri_close, the queued grind windows, k_fri_queries), shared by tests/test_fri_close_emu.py (the emulation build, no GPU)
and tests/test_gpu_fri_close.py (the MI355X).  Every comparison is exact.  References: the oracle (`oracle.fft.
line_interpolate`, `Blake2sChannel.mix_felts / grind / mix_u64`, `oracle.prover.draw_queries`) and the library's own host
loop (`Library.grind` = lmn_op_grind); whole proofs under LMN_DEVICE_FRI_CLOSE=1 are compared with the host close (the default) byte by byte
and handed to the verifier.

Low-degree layers come from `line_evaluate`, the forward line transform written here and checked by a round trip through the
oracle's `line_interpolate` (check_line_evaluate_round_trip)."""
import functools
import hashlib
import os
import sys
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from luminair_amd import backend, synthetic as syn                      # noqa: E402
from oracle.channel import Blake2sChannel, ProtocolVariant              # noqa: E402
from oracle.circle import Coset, LineDomain                             # noqa: E402
from oracle.field import P, QM31, q_add, q_mul_m, q_sub                 # noqa: E402
from oracle.fft import line_interpolate                                 # noqa: E402
from oracle.prover import draw_queries                                  # noqa: E402

U32 = np.uint32
WINDOW_LOG = 11                  # LMN_POW_WINDOW_LOG of every context here: the smallest window, one block of 2048 nonces
QUEUED = 8 << WINDOW_LOG         # nonces examined behind k_fri_close before the host looks: POW_WINDOWS_PER_WAIT windows
FORMS = [backend.VARIANT_KAT, backend.PV_MIX_U64_HASHED, backend.PV_POW_PREFIXED]   # the three proof-of-work forms
LDS_LOG = 11                     # FRI_CLOSE_LDS_LOG: layers above 2^11 values run their passes in device memory


class Env:
    """environment switches that the library reads when a context is created or a proof starts"""

    def __init__(self, **kv):
        self.kv = {k: str(v) for k, v in kv.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Contexts:
    """one context per configuration, created under LMN_POW_WINDOW_LOG=11 and kept for the module"""

    def __init__(self, lib):
        self.lib, self.ctxs = lib, {}

    def get(self, log_last_layer=0, log_blowup=1, pow_bits=1, n_queries=3, variant=backend.VARIANT_KAT, window_log=WINDOW_LOG):
        key = (log_last_layer, log_blowup, pow_bits, n_queries, variant, window_log)
        if key not in self.ctxs:
            cfg = self.lib.default_config()
            cfg.log_last_layer, cfg.log_blowup, cfg.pow_bits, cfg.n_queries = log_last_layer, log_blowup, pow_bits, n_queries
            cfg.protocol_variant = variant
            with Env(**({"LMN_POW_WINDOW_LOG": window_log} if window_log else {})):
                self.ctxs[key] = backend.Context(0, cfg, self.lib)
        return self.ctxs[key]

    def close(self):
        for c in self.ctxs.values():
            c.close()
        self.ctxs = {}


# ----------------------------------------------------------------------------- the forward line transform
def line_domain(log_n):
    return LineDomain(Coset.half_odds(log_n))


def line_evaluate(coeffs, domain=None):
    """ordered line-poly coefficients ((n, 4) words; coefficient j multiplies x^(j & 1) pi(x)^(j >> 1 & 1) ...) -> the
    evaluations, bit-reversed over LineDomain(half_odds(log n)): f(x) = f0(pi(x)) + x f1(pi(x)), even coefficients to f0"""
    c = np.asarray(coeffs, dtype=np.uint64)
    n = len(c)
    domain = domain or line_domain(n.bit_length() - 1)
    if n == 1:
        return c.copy()
    e0, e1 = line_evaluate(c[0::2], domain.double()), line_evaluate(c[1::2], domain.double())
    t = q_mul_m(e1, np.asarray(domain.xs_bitrev()[0::2], dtype=np.uint64))
    out = np.empty((n, 4), dtype=np.uint64)
    out[0::2], out[1::2] = q_add(e0, t), q_sub(e0, t)
    return out


def oracle_coeffs(values):
    """all n coefficients of the layer `values` ((n, 4) words) by the oracle"""
    n = len(values)
    got = line_interpolate([QM31(*(int(w) for w in v)) for v in values], line_domain(n.bit_length() - 1))
    return np.array([list(c.v) for c in got], dtype=np.uint64).reshape(n, 4)


def check_line_evaluate_round_trip():
    rng = np.random.default_rng(7)
    for log_n in (0, 1, 2, 5, 8):
        c = rng.integers(0, P, size=(1 << log_n, 4), dtype=np.uint64)
        assert np.array_equal(oracle_coeffs(line_evaluate(c)), c), log_n


# ----------------------------------------------------------------------------- layers
SHAPES = [(ll, lb) for ll in (0, 1, 3, 10) for lb in (1, 2, 3)]        # 2 .. 2^13 values, both sides of 2^LDS_LOG
assert {ll + lb > LDS_LOG for ll, lb in SHAPES} == {False, True} and (10, 1) in SHAPES   # 2^11 itself: the last LDS size
CLASSES = ["zero", "p-1", "random", "last-ok", "first-bad", "last", "full"]


@functools.lru_cache(maxsize=None)
def layer(cls, log_last_layer, log_blowup):
    """-> (values (n, 4) uint32, all n expected coefficients (n, 4) uint64): by construction from coefficients where the
    class names them, by the oracle's interpolation where it names the values"""
    log_n = log_last_layer + log_blowup
    n, bound = 1 << log_n, 1 << log_last_layer
    rng = np.random.default_rng(1000 * log_n + 10 * log_last_layer + CLASSES.index(cls))
    if cls in ("zero", "p-1", "full"):
        vals = {"zero": np.zeros((n, 4), np.uint64), "p-1": np.full((n, 4), P - 1, np.uint64),
                "full": rng.integers(0, P, size=(n, 4), dtype=np.uint64)}[cls]
        return vals.astype(U32), oracle_coeffs(vals)
    c = np.zeros((n, 4), dtype=np.uint64)
    if cls == "random":                                       # a random polynomial of the degree the layer should have
        c[:bound] = rng.integers(0, P, size=(bound, 4), dtype=np.uint64)
    else:                                                     # one non-zero coefficient
        at = {"last-ok": bound - 1, "first-bad": bound, "last": n - 1}[cls]
        c[at] = rng.integers(1, P, size=4, dtype=np.uint64)
    return line_evaluate(c).astype(U32), c


def first_bad_of(coeffs, bound):
    bad = np.nonzero(coeffs[bound:].any(axis=1))[0]
    return None if len(bad) == 0 else bound + int(bad[0])


def digest_of(seed):
    return hashlib.sha256(b"fri close start digest %d" % seed).digest()


def oracle_close(values_coeffs, bound, start_digest, variant, pow_bits, n_queries, log_query_domain, nonce=None):
    """the oracle's transcript from `start_digest` over the first `bound` coefficients -> (nonce, positions, the three digests,
    n_sent at the end).  nonce: given (the host loop's - checked to pass the oracle's check), or ground by the oracle"""
    ch = Blake2sChannel(ProtocolVariant(variant))
    ch.digest = start_digest
    ch.mix_felts([QM31(*(int(w) for w in c)) for c in values_coeffs[:bound]])
    d_coeffs = ch.digest
    if nonce is None:
        nonce = ch.grind(pow_bits)
    assert ch.verify_pow_nonce(pow_bits, nonce)
    ch.mix_u64(nonce)
    d_nonce = ch.digest
    positions = draw_queries(ch, log_query_domain, n_queries)
    return nonce, positions, d_coeffs, d_nonce, ch.digest, ch.n_sent


def run_close(ctx, values, start_digest, log_query_domain):
    col = ctx.col_from_cpu(np.ascontiguousarray(values.T))           # 4 coordinate columns
    try:
        return ctx.fri_close(col, start_digest, log_query_domain)
    finally:
        col.free()


def compare(got, coeffs, bound, want, what):
    nonce, positions, d_coeffs, d_nonce, d_end, n_sent = want
    assert got.coeffs == [tuple(int(w) for w in c) for c in coeffs[:bound]], what
    assert got.first_bad == first_bad_of(coeffs, bound), what
    assert got.digest_after_coeffs == d_coeffs, what
    assert got.nonce == nonce, what
    assert got.digest_after_nonce == d_nonce and got.digest_end == d_end and got.n_sent_end == n_sent, what
    assert got.positions == positions, what


# ----------------------------------------------------------------------------- the op
def check_shape_and_class(ctxs, shape, cls):
    """interpolation, degree check and the transcript behind them at every shape and value class; the expected first_bad per
    class is asserted here from the reference coefficients"""
    ll, lb = shape
    bound, n = 1 << ll, 1 << (ll + lb)
    values, coeffs = layer(cls, ll, lb)
    expect_bad = {"zero": None, "p-1": None, "random": None, "last-ok": None, "first-bad": bound, "last": n - 1}
    if cls in expect_bad:
        assert first_bad_of(coeffs, bound) == expect_bad[cls], (shape, cls)
    else:
        assert first_bad_of(coeffs, bound) is not None            # a random layer has full degree
    if cls == "p-1":
        assert coeffs[0].tolist() == [P - 1] * 4 and not coeffs[1:].any()
    ctx = ctxs.get(log_last_layer=ll, log_blowup=lb, pow_bits=1)
    start = digest_of(100 * ll + 10 * lb + CLASSES.index(cls))
    got = run_close(ctx, values, start, 12)
    compare(got, coeffs, bound, oracle_close(coeffs, bound, start, backend.VARIANT_KAT, 1, 3, 12), (shape, cls))


# 16-bit seeds per form, picked on the CPU from the oracle's nonces: (one whose nonce lies in the queued windows, one
# beyond them).  The KAT form's bare compression is plain Python in the oracle (0.25 ms per nonce): its second seed was
# chosen for a nonce just past the queue.
GRIND_SEEDS_16 = {backend.VARIANT_KAT: (321, 165), backend.PV_MIX_U64_HASHED: (219, 108), backend.PV_POW_PREFIXED: (120, 138)}
GRIND_SHAPE = (1, 1)


@functools.lru_cache(maxsize=None)
def grind_reference(variant, pow_bits, seed):
    values, coeffs = layer("random", *GRIND_SHAPE)
    return oracle_close(coeffs, 1 << GRIND_SHAPE[0], digest_of(seed), variant, pow_bits, 3, 12)


def check_grind(ctxs, lib, variant, pow_bits):
    ll, lb = GRIND_SHAPE
    values, coeffs = layer("random", ll, lb)
    ctx = ctxs.get(log_last_layer=ll, log_blowup=lb, pow_bits=pow_bits, variant=variant)
    seeds = GRIND_SEEDS_16[variant] if pow_bits == 16 else (1, 2)
    rounds = []
    for seed in seeds:
        want = grind_reference(variant, pow_bits, seed)
        got = run_close(ctx, values, digest_of(seed), 12)
        compare(got, coeffs, 1 << ll, want, (variant, pow_bits, seed))
        assert got.nonce == lib.grind(want[2], pow_bits, variant)       # the library's own host loop
        assert (got.grind_rounds == 0) == (want[0] < QUEUED), (got.grind_rounds, want[0])
        rounds.append(got.grind_rounds)
    if pow_bits == 16:                                                   # both ends of the chain: no fallback, fallback
        below, above = (grind_reference(variant, 16, s)[0] for s in seeds)
        assert below < QUEUED <= above, (below, above)
        assert rounds[0] == 0 and rounds[1] >= 1, rounds


N_QUERIES = [1, 3, 8, 9, 16, 17, 70, 1024]
QUERY_DOMAINS = [0, 1, 4, 12, 27, 31]


def check_draws(ctxs, n_queries, u32_counter):
    variant = backend.PV_DRAW_CTR_U32 if u32_counter else backend.VARIANT_KAT
    ctx = ctxs.get(n_queries=n_queries, variant=variant)
    values, coeffs = layer("random", 0, 1)
    for lqd in QUERY_DOMAINS:
        start = digest_of(7000 + 40 * n_queries + lqd)
        want = oracle_close(coeffs, 1, start, variant, 1, n_queries, lqd)
        got = run_close(ctx, values, start, lqd)
        compare(got, coeffs, 1, want, (n_queries, u32_counter, lqd))
        assert got.positions == sorted(set(got.positions)) and len(got.positions) <= min(n_queries, 1 << lqd)
        if lqd == 0:
            assert got.positions == [0]
        if lqd == 4 and n_queries == 70:
            assert len(got.positions) < 70                               # duplicates were there to remove
        assert got.n_sent_end == (n_queries + 7) // 8


def check_refusals(ctxs):
    """every refusal names its argument, zeroes the result and leaves the context and the handles usable"""
    import ctypes as C
    from luminair_amd.backend import ERR_INVALID_ARGUMENT, LmnFriCloseResult, LuminairBackendError
    ctx = ctxs.get(log_last_layer=1, log_blowup=1)
    values, coeffs = layer("random", 1, 1)
    good = ctx.col_from_cpu(np.ascontiguousarray(values.T))
    three = ctx.col_from_cpu(np.zeros((3, 4), U32))
    small = ctx.col_from_cpu(np.zeros((4, 2), U32))
    big = ctx.col_from_cpu(np.zeros((4, 8), U32))
    start = digest_of(1)
    try:
        for col, lqd, word in ((three, 12, "last_layer"), (small, 12, "last_layer"), (big, 12, "last_layer"),
                               (good, 32, "log_query_domain")):
            try:
                ctx.fri_close(col, start, lqd)
            except LuminairBackendError as e:
                assert e.code == ERR_INVALID_ARGUMENT and "fri_close" in str(e) and word in str(e), (word, e.code, str(e))
            else:
                raise AssertionError("accepted: %s" % word)
        L = ctx.lib.lib
        dig = (C.c_uint8 * 32)(*start)

        def filled():
            r = LmnFriCloseResult()
            r.n_coeffs, r.nonce, r.n_sent_end = 5, 6, 7
            return r
        for args, word in (((ctx.handle, None, dig, 12), "last_layer"), ((ctx.handle, good.handle, None, 12), "start_digest")):
            res = filled()
            assert L.lmn_col_fri_close(*args, C.byref(res)) == ERR_INVALID_ARGUMENT
            assert word in L.lmn_last_error(ctx.handle).decode(), word
            assert res.n_coeffs == 0 and res.nonce == 0 and res.n_sent_end == 0 and not res.coeffs and not res.positions
        assert L.lmn_col_fri_close(ctx.handle, good.handle, dig, 12, None) == ERR_INVALID_ARGUMENT
        res = filled()
        assert L.lmn_col_fri_close(None, good.handle, dig, 12, C.byref(res)) == ERR_INVALID_ARGUMENT and res.n_coeffs == 0
        got = ctx.fri_close(good, start, 12)                             # context and handle still work
        compare(got, coeffs, 2, oracle_close(coeffs, 2, start, backend.VARIANT_KAT, 1, 3, 12), "after the refusals")
        assert np.array_equal(good.to_cpu(), values.T)
    finally:
        for h in (good, three, small, big):
            h.free()


def check_sharded_context_refused(ctxs):
    from luminair_amd.backend import ERR_INVALID_ARGUMENT, LuminairBackendError
    ctx = ctxs.get()
    values, coeffs = layer("random", 0, 1)
    h = ctx.col_from_cpu(np.ascontiguousarray(values.T))
    ctx.set_shard(0, 1, lambda *a: None)
    try:
        try:
            ctx.fri_close(h, digest_of(2), 12)
        except LuminairBackendError as e:
            assert e.code == ERR_INVALID_ARGUMENT and "sharded" in str(e), (e.code, str(e))
        else:
            raise AssertionError("a sharded context closed the transcript")
    finally:
        ctx.clear_shard()
    try:
        got = ctx.fri_close(h, digest_of(2), 12)
        compare(got, coeffs, 1, oracle_close(coeffs, 1, digest_of(2), backend.VARIANT_KAT, 1, 3, 12), "after the shard is cleared")
    finally:
        h.free()


def check_batch_library(batch_so):
    """the same entry in the lock-step library, on a thread outside any batch: both ends of the chain"""
    ctxs = Contexts(backend.Library(batch_so))
    try:
        lib = ctxs.lib
        check_grind(ctxs, lib, backend.PV_MIX_U64_HASHED, 16)
        check_shape_and_class(ctxs, (10, 2), "full")
        ctx = ctxs.get(log_last_layer=GRIND_SHAPE[0], log_blowup=GRIND_SHAPE[1], pow_bits=16, variant=backend.PV_MIX_U64_HASHED)
        assert ctx.counter(backend.COUNTER_GRINDS) >= 2 and ctx.counter(backend.COUNTER_DEVICE_CLOSES) == 0
    finally:
        ctxs.close()


# ----------------------------------------------------------------------------- whole proofs
@dataclass(frozen=True)
class ProofCase:
    name: str
    variant: int
    pow_bits: int
    log_last_layer: int
    log_blowup: int
    n_queries: int
    tables: str = "add"          # add: config2_add_only(64, seed); faithful: config2_graph_faithful(64, seed); mixed
    seed: int = 11

    @property
    def id(self):
        return self.name


KAT, HASHED, PINNED = backend.VARIANT_KAT, backend.PV_MIX_U64_HASHED, backend.VARIANT_PINNED
PROOF_CASES = [
    ProofCase("kat pow12 ll0 lb1 q3", KAT, 12, 0, 1, 3),
    ProofCase("kat pow16 ll2 lb1 q70", KAT, 16, 2, 1, 70),
    ProofCase("kat pow12 ll0 lb2 q70", KAT, 12, 0, 2, 70),
    ProofCase("kat pow12 ll3 lb3 q3", KAT, 12, 3, 3, 3),
    ProofCase("hashed pow12 ll2 lb1 q3", HASHED, 12, 2, 1, 3),
    ProofCase("hashed pow16 ll0 lb2 q3", HASHED, 16, 0, 2, 3),
    ProofCase("hashed pow12 ll3 lb3 q70", HASHED, 12, 3, 3, 70),
    ProofCase("pinned pow12 ll0 lb1 q70", PINNED, 12, 0, 1, 70, "faithful"),
    ProofCase("pinned pow16 ll3 lb3 q3", PINNED, 16, 3, 3, 3, "faithful"),
    ProofCase("pinned pow12 ll2 lb1 q3", PINNED, 12, 2, 1, 3, "faithful"),
    ProofCase("kat pow12 ll2 lb1 q70 mixed sizes", KAT, 12, 2, 1, 70, "mixed"),
]
# pow_bits 16 under 2^11-nonce windows, seeds picked on the CPU: the nonce of the first lies in the queued windows, the
# second's beyond them
FALLBACK_SEEDS = (4, 1)


def tables_of(case, seed=None):
    seed = case.seed if seed is None else seed
    if case.tables == "mixed":
        tabs = syn.config3_mixed(8, 7, 6, seed)                      # Add 2^8, Mul 2^7, Recip 2^6 rows
    elif case.tables == "faithful":
        tabs = syn.config2_graph_faithful(64, seed)
    else:
        tabs = syn.config2_add_only(64, seed)
    return [(k, r, len(r)) for k, r in tabs]


def proof_config(lib, case):
    cfg = lib.default_config()
    cfg.pow_bits, cfg.log_last_layer, cfg.log_blowup, cfg.n_queries = case.pow_bits, case.log_last_layer, case.log_blowup, case.n_queries
    cfg.protocol_variant = case.variant
    return cfg


COUNTERS = (backend.COUNTER_GRINDS, backend.COUNTER_GRIND_WAITS, backend.COUNTER_DEVICE_CLOSES,
            backend.COUNTER_DEVICE_CLOSE_FALLBACKS)


def prove_both(lib, case, tables, window_log=None):
    """-> (device-close proof, its counter deltas, host-close proof, its counter deltas), one context each"""
    out = []
    for host_close in (False, True):
        env = {} if host_close else {"LMN_DEVICE_FRI_CLOSE": 1}
        if window_log:
            env["LMN_POW_WINDOW_LOG"] = window_log
        with Env(**env):
            ctx = backend.Context(0, proof_config(lib, case), lib)
            try:
                before = [ctx.counter(w) for w in COUNTERS]
                proof = ctx.prove_tables(tables)
                out += [proof, dict(zip(COUNTERS, (ctx.counter(w) - b for w, b in zip(COUNTERS, before))))]
            finally:
                ctx.close()
    return out


def check_proof_case(lib, case):
    dev, dc, host, hc = prove_both(lib, case, tables_of(case))
    assert dev == host, case.name
    lib.verify(dev, case.variant, proof_config(lib, case))
    assert dc[9] == 1 and hc[9] == 0 and hc[10] == 0, (dc, hc)
    assert hc[8] >= 1 and hc[7] == 1, hc                               # the host close waits for its grind
    if dc[10] == 0:
        assert dc[8] == 0 and dc[7] == 1, dc                           # the device close did not


def check_fallback_occurs_and_not(lib):
    """2^11-nonce windows at pow_bits 16: one proof whose nonce lies in the queued windows and one that goes on grinding,
    both byte-equal to the host close"""
    case = ProofCase("fallback", KAT, 16, 0, 1, 3)
    fallbacks = []
    for seed in FALLBACK_SEEDS:
        dev, dc, host, hc = prove_both(lib, case, tables_of(case, seed), WINDOW_LOG)
        assert dev == host, seed
        lib.verify(dev, case.variant, proof_config(lib, case))
        assert dc[9] == 1 and (dc[8] >= 1) == (dc[10] == 1), dc
        fallbacks.append(dc[10])
    assert fallbacks == [0, 1], fallbacks


def check_default_path_untouched(lib):
    """pow_bits 5: no device grind and no device close, with default switches and under LMN_DEVICE_FRI_CLOSE=1 alike"""
    cfg = lib.default_config()
    assert cfg.pow_bits == 5
    ctx = backend.Context(0, cfg, lib)
    try:
        tables = [(k, r, len(r)) for k, r in syn.config2_add_only(64, 11)]
        want = ctx.prove_tables(tables)
        with Env(LMN_DEVICE_FRI_CLOSE=1):
            assert ctx.prove_tables(tables) == want
        assert [ctx.counter(w) for w in COUNTERS] == [0, 0, 0, 0]
        assert ctx.counter(0) == 0 and ctx.counter(11) == 0
    finally:
        ctx.close()


def check_error_precedence(lib):
    """a non-canonical word and a broken constraint end as they do under the host close, at pow_bits 12"""
    case = ProofCase("errors", KAT, 12, 0, 1, 3)
    bad_word = syn.config2_add_only(64, 9)[0][1].copy()
    bad_word[5, 9] = 0x7fffffff
    bad_constraint = syn.config2_add_only(64, 9)[0][1].copy()
    bad_constraint[3, 11] ^= 1
    for rows, code in ((bad_word, backend.ERR_INVALID_ARGUMENT), (bad_constraint, backend.ERR_CONSTRAINTS)):
        got = []
        for host_close in (False, True):
            with Env(**({} if host_close else {"LMN_DEVICE_FRI_CLOSE": 1})):
                ctx = backend.Context(0, proof_config(lib, case), lib)
                try:
                    ctx.prove_tables([(0, rows, len(rows))])
                except backend.LuminairBackendError as e:
                    got.append(e.code)
                else:
                    got.append(0)
                finally:
                    ctx.close()
        assert got == [code, code], got
