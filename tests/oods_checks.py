"""The step between the composition tree and the first FRI layer, at its shape edges: `eval_at_points` (csrc/oods.cpp:
k_eval_tables, k_eval_at_point, k_eval_reduce over every (column, point) job of a proof in one launch triple) and
`k_quot_prepare` (kernels_merkle.hip, planned by `enqueue_quotient_tables` in phase_oods.cpp: the sampled values mixed into
the device channel, the quotient randomness drawn, the quotient kernels' tables for every LDE size).  Shared by
tests/test_oods_emu.py (emulation build, CPU suite) and tests/test_gpu_oods.py (MI355X).

Only whole proofs reach this code with mixed job sizes, and `run_oods` chooses between the device path and the host's wait
by what cannot be seen from outside; so every case is a whole proof, proved on one context under the default path, under
LMN_HOST_QUOT=1 and under LMN_HOST_FS=1, and
  * all three results equal the oracle's bytes (oracle.prover, the C oracle from 2^15 rows in a table) - on a mismatch both
    proofs are parsed and the first differing field in transcript order is named (where the library's own replay refuses
    the proof first - the composition identity, the quotient randomness - its text is reported with the step it points to);
  * `lmn_ctx_counter` 22 / 23 say which path was taken, and the path expected is computed from the oracle's own trees
    (distinct column log sizes of its four commitment trees plus log_blowup: at most QUOT_PREP_MAX_SIZES = 8 for the device).

The oracle in turn is tied to plain integers for a mixed-size job table (`check_sampled_values_against_plain_integers`).

The pies (`edge_pie`): kind-ordered tables of the nine kinds that need no LUT, 2^logs[i] rows each.  mults="zero": all
multiplicities 0, so every interaction column is all-zero and sampled to exactly 0 (la = 0, lbb = 0 in k_quot_prepare), as
are the multiplicity columns; mults="chain": the first three tables start with `chain_graph`'s balanced Add / Mul / Recip
rows (non-zero multiplicities, non-zero interaction columns), filled up with rows of multiplicity 0 under other node ids
(every local constraint reads one row alone, so blocks of different nodes may follow each other).

A case's sample count is sum over its tables of (n_cols + 4 n_rel + 4), plus 4 for the composition, plus the preprocessed
columns; `mix_felts` hashes 8 + 4 n_samples words, so n_samples = 2 (mod 4) ends on a Blake2s block boundary (a full last
block, no zero padding, byte counter 4 x words).  `check_matrix_reaches_every_edge` asserts from the oracle's proofs alone
that the device-path cases reach all four residues (2 at two block counts), that both paths, 8 and 9 sizes and both
multiplicity forms are there.  The limit of 496 samples cannot be reached through `lmn_prove` (kernels.h) and is not
tested."""
import functools
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import numpy as np

import numeric_checks as nc
from luminair_amd import backend, synthetic as syn
from oracle.channel import Blake2sChannel, ProtocolVariant
from oracle.field import ONE
from oracle.proof import from_bincode, to_bincode
from oracle.prover import PcsConfig, claim_slots, prove as oracle_prove

KAT, PINNED = ProtocolVariant.KAT, ProtocolVariant.PINNED
KINDS = (0, 1, 2, 5, 6, 7, 8, 15, 16)       # the kinds that need no LUT
MAX_SIZES, MAX_SAMPLES = 8, 496             # QUOT_PREP_MAX_SIZES, QUOT_PREP_MAX_SAMPLES of csrc/kernels.h
C_ORACLE_MIN_LOG = 15                       # the C oracle from 2^15 rows in a table
COUNTER_DEVICE, COUNTER_HOST_WAIT = backend.COUNTER_QUOT_DEVICE, backend.COUNTER_QUOT_HOST_WAIT
SWITCHES = ({}, {"LMN_HOST_QUOT": "1"}, {"LMN_HOST_FS": "1"})
CHAIN_ROWS = 8                              # the balanced rows at the head of a "chain" pie's first three tables


# ----------------------------------------------------------------------------- pies
def _rows(kind, n, rng, node):
    """n rows of `kind` with every multiplicity 0"""
    if kind == 0:
        return syn.add_rows(rng.integers(-2048, 2048, n), rng.integers(-2048, 2048, n), node=node, lhs_id=node + 1, rhs_id=node + 2)
    if kind == 1:
        return syn.mul_rows(rng.integers(0, 2048, n), rng.integers(0, 2048, n), node=node, lhs_id=node + 1, rhs_id=node + 2)
    if kind == 2:
        return syn.recip_rows(rng.integers(4, 2048, n), node=node, input_id=node + 1)
    if kind in (5, 6):
        x = rng.integers(-2048, 2048, (n // 4, 4))
        fn = syn.sum_reduce_rows if kind == 5 else syn.max_reduce_rows
        return fn(x, node=node, input_id=node + 1, input_mult=0, out_mult=0)
    if kind == 7:
        return syn.sqrt_rows(rng.integers(0, 1 << 20, n), node=node, input_id=node + 1)
    if kind == 8:
        return syn.rem_rows(rng.integers(0, 1 << 20, n), rng.integers(1, 4096, n), node=node, lhs_id=node + 1, rhs_id=node + 2)
    if kind == 15:
        return syn.inputs_rows(rng.integers(-2048, 2048, n), node, 0)
    if kind == 16:
        return syn.contiguous_rows(rng.integers(-2048, 2048, n), node=node, input_id=node + 1, input_mult=0, out_mult=0)
    raise ValueError(kind)


def edge_pie(logs, mults="zero", seed=1, kinds=None):
    """kind-ordered tables [(kind, rows)], table i of 2^logs[i] rows; kinds: the first len(logs) of KINDS unless given"""
    kinds = tuple(kinds) if kinds is not None else KINDS[:len(logs)]
    assert len(kinds) == len(logs) and list(kinds) == sorted(set(kinds)) and set(kinds) <= set(KINDS) and min(logs) >= 4
    rng = np.random.default_rng(seed)
    tabs = [(k, _rows(k, 1 << lg, rng, 100 + 10 * i)) for i, (k, lg) in enumerate(zip(kinds, logs))]
    if mults == "chain":
        assert kinds[:3] == (0, 1, 2)
        for i, (k, rows) in enumerate(syn.chain_graph(CHAIN_ROWS, seed)):
            assert k == tabs[i][0]
            tabs[i] = (k, np.concatenate([rows, tabs[i][1][CHAIN_ROWS:]]))
    else:
        assert mults == "zero"
    assert all(len(r) == 1 << lg for (_, r), lg in zip(tabs, logs))
    return tabs


def lut_pie(extra_logs):
    """`activation_graph(40, 3)`: three LUT pairs with LUTs of 2^16, 2^15 and 2^14 rows in tree 0 - sizes that only the
    lookup tables share - next to tables of 2^6 and 2^7 rows, plus Add / Mul / Recip tables of 2^extra_logs[i] rows"""
    tabs, luts = syn.activation_graph(40, 3)
    extra = edge_pie(extra_logs, "zero", 5)
    return sorted(list(tabs) + extra, key=lambda kt: kt[0]), luts


@dataclass(frozen=True)
class Case:
    name: str
    logs: Tuple[int, ...] = ()
    mults: str = "zero"
    kinds: Optional[Tuple[int, ...]] = None
    seed: int = 1
    variant: ProtocolVariant = PINNED
    log_blowup: int = 1
    log_last_layer: int = 0
    dirty: bool = False                 # nc.dirty_context in front of every proof
    build: Optional[Callable] = None    # -> (tables, luts) where the pie is no edge_pie

    def tables(self):
        return self.build() if self.build else (edge_pie(self.logs, self.mults, self.seed, self.kinds), None)

    @property
    def max_log(self):
        return max(int(len(r) - 1).bit_length() for _, r in self.tables()[0])

    def pcs(self):
        return PcsConfig(pow_bits=5, log_blowup=self.log_blowup, log_last_layer=self.log_last_layer, n_queries=3)


_UP7, _UP8, _UP9 = tuple(range(4, 11)), tuple(range(4, 12)), tuple(range(4, 13))
CASES = [
    # size count: 8 sizes (the last case of the device path), 9 (the first fallback), 10 (ten sample points)
    Case("7 tables 2^4..2^10: 8 sizes", _UP7),
    Case("8 tables 2^4..2^11: 9 sizes", _UP8),
    Case("9 tables 2^4..2^12: 10 sizes", _UP9),
    Case("7 tables 2^10..2^4: 8 sizes, descending", _UP7[::-1]),
    Case("8 tables 2^11..2^4: 9 sizes, descending", _UP8[::-1]),
    Case("9 tables 2^12..2^4: 10 sizes, descending", _UP9[::-1]),
    Case("9 tables of 2^4: 2 sizes", (4,) * 9),
    Case("one table of 2^4", (4,)),
    # both multiplicity forms at 8 and 9 sizes
    Case("7 tables 2^4..2^10, chain multiplicities", _UP7, "chain", seed=2),
    Case("8 tables 2^4..2^11, chain multiplicities", _UP8, "chain", seed=2),
    # mixed job sizes (stale words in the arena in front of each)
    Case("8 x 2^4 + 2^14: two chunks next to sub-table jobs", (4,) * 8 + (14,), dirty=True),
    Case("2^4 2^9 2^10 2^11 2^13: the lo-table boundary", (4, 9, 10, 11, 13), "chain", seed=3, dirty=True),
    # config
    Case("8 sizes at log_blowup 2", _UP7, seed=4, log_blowup=2),
    Case("6 sizes at log_blowup 3", (4, 5, 6, 7, 8), "chain", kinds=(0, 1, 2, 15, 16), seed=4, log_blowup=3),
    Case("8 sizes at log_last_layer 2", _UP7, "chain", seed=5, log_last_layer=2),
    Case("variant 0: kinds 0 1 2 5", (4, 6, 5, 7), "chain", kinds=(0, 1, 2, 5), seed=6, variant=KAT),
    # preprocessed columns: LUTs of 2^16, 2^15, 2^14 rows
    Case("LUT pie, 8 sizes", build=functools.partial(lut_pie, (4, 5))),
    Case("LUT pie, 9 sizes", build=functools.partial(lut_pie, (4, 5, 8))),
]
GPU_ONLY_CASES = [
    Case("2^4 2^10 2^17: 16 chunks", (4, 10, 17), "chain", seed=7, dirty=True),
]
PIN_CASE = Case("plain-integer pin: 2^4..2^8, three rows short each", (4, 5, 6, 7, 8), "chain", seed=8)
BY_NAME = {c.name: c for c in CASES + GPU_ONLY_CASES + [PIN_CASE]}
assert len(BY_NAME) == len(CASES) + len(GPU_ONLY_CASES) + 1


# ----------------------------------------------------------------------------- reference
@dataclass
class Reference:
    data: bytes
    proof: object
    n_sizes: int
    n_samples: int
    n_points: int

    @property
    def device(self):
        return self.n_sizes <= MAX_SIZES and self.n_samples <= MAX_SAMPLES

    @property
    def blocks(self):
        return -(-(8 + 4 * self.n_samples) // 16)


_REF = {}


def reference(case, kernels=None, tabs=None):
    """the oracle's proof of the case, once; the path the library must take, from the oracle's own trees"""
    key = (case.name, tabs is not None)
    if key not in _REF:
        own, luts = case.tables()
        tabs = tabs if tabs is not None else own
        if case.max_log >= C_ORACLE_MIN_LOG and kernels is None:
            kernels = nc._c_oracle()
        rows = tabs if kernels is not None else [(k, r.astype(np.uint64)) for k, r in tabs]
        proof, tr = oracle_prove(rows, case.pcs(), variant=case.variant, want_trace=True, kernels=kernels, luts=luts)
        sizes = {ls + case.log_blowup for t in tr.trees for ls in t.log_sizes}
        sv = proof.proof.sampled_values
        _REF[key] = Reference(to_bincode(proof), proof, len(sizes), sum(len(c) for t in sv for c in t),
                              1 + len({ls for ls in proof.claim if ls is not None}))
    return _REF[key]


def first_difference(got: bytes, want: bytes, variant) -> str:
    """the first field, in transcript order, at which two proofs differ - and the code that makes it"""
    n_slots = claim_slots(variant)
    try:
        g = from_bincode(got, n_slots)
    except ValueError as e:
        return "the library's proof does not parse (%s)" % e
    w = from_bincode(want, n_slots)
    gs, ws = g.proof, w.proof
    if g.claim != w.claim:
        return "claim (log sizes): got %s want %s" % (g.claim, w.claim)
    names = ("preprocessed", "main trace", "interaction trace", "composition")
    for t in range(3):
        if gs.commitments[t] != ws.commitments[t]:
            return "commitments[%d] (%s tree)" % (t, names[t])
        if t == 1 and g.interaction_claim != w.interaction_claim:
            return "claimed sums (logup)"
    if gs.commitments[3] != ws.commitments[3]:
        return "commitments[3] (composition tree)"
    shape = lambda sv: [[len(c) for c in t] for t in sv]
    if shape(gs.sampled_values) != shape(ws.sampled_values):
        return "sampled_values: another shape - the sample points planned per column (plan_eval_jobs)"
    for t in range(4):
        for c, (gc, wc) in enumerate(zip(gs.sampled_values[t], ws.sampled_values[t])):
            for p, (gv, wv) in enumerate(zip(gc, wc)):
                if gv != wv:
                    return ("sampled_values[%d][%d][%d] (%s tree): got %s want %s - evaluation (eval_at_points: k_eval_tables, "
                            "k_eval_at_point, k_eval_reduce)" % (t, c, p, names[t], gv.v, wv.v))
    if gs.first_layer.commitment != ws.first_layer.commitment:
        return ("the first FRI layer's commitment, with equal sampled values - quotient tables / quotient kernel (k_quot_prepare "
                "or make_quotient_args: the mix of the sampled values, the quotient randomness, the entries; k_quotients)")
    for i, (gl, wl) in enumerate(zip(gs.inner_layers, ws.inner_layers)):
        if gl.commitment != wl.commitment:
            return "inner FRI layer %d's commitment (the FRI commit loop)" % i
    if len(gs.inner_layers) != len(ws.inner_layers):
        return "the number of inner FRI layers"
    if gs.last_layer_coeffs != ws.last_layer_coeffs:
        return "last_layer_coeffs"
    if gs.proof_of_work != ws.proof_of_work:
        return "proof_of_work"
    if gs.queried_values != ws.queried_values:
        return "queried_values (the openings)"
    if gs.decommitments != ws.decommitments:
        return "decommitments of the trace trees"
    return "the FRI layers' witnesses or decommitments"


def check_first_difference_names_the_field():
    """no library: a proof of the oracle with one field changed is named by that field, in transcript order"""
    import copy
    case = CASES[0]
    ref = reference(case)

    def changed(edit):
        p = copy.deepcopy(ref.proof)
        edit(p.proof)
        return first_difference(to_bincode(p), ref.data, case.variant)

    def sample(s):
        s.sampled_values[2][-1][0] = s.sampled_values[2][-1][0] + ONE

    def first_layer(s):
        s.first_layer.commitment = bytes(32)

    def both(s):
        sample(s)
        first_layer(s)

    assert "sampled_values[2][%d][0]" % (len(ref.proof.proof.sampled_values[2]) - 1) in changed(sample)
    assert "evaluation" in changed(sample) and "evaluation" in changed(both)
    assert "quotient tables / quotient kernel" in changed(first_layer)
    assert first_difference(ref.data[:-1], ref.data, case.variant).startswith("the library's proof does not parse")


def _same(got, want, case, what):
    if got != want:
        raise AssertionError("%s (%s): the proof differs from the oracle's; first differing field: %s"
                             % (case.name, what, first_difference(got, want, case.variant)))


# ----------------------------------------------------------------------------- contexts
class Provers:
    """one context per (variant, log_blowup, log_last_layer) on a given library"""

    def __init__(self, lib):
        self.lib, self.ctxs = lib, {}

    def config(self, case):
        cfg = self.lib.default_config()
        cfg.protocol_variant = backend.VARIANT_PINNED if case.variant == PINNED else backend.VARIANT_KAT
        cfg.pow_bits, cfg.n_queries = 5, 3
        cfg.log_blowup, cfg.log_last_layer = case.log_blowup, case.log_last_layer
        return cfg

    def ctx(self, case):
        key = (int(case.variant), case.log_blowup, case.log_last_layer)
        if key not in self.ctxs:
            self.ctxs[key] = backend.Context(0, self.config(case), self.lib)
        return self.ctxs[key]

    def close(self):
        for c in self.ctxs.values():
            c.close()
        self.ctxs.clear()


def _pie(tabs):
    return [(k, r, len(r)) for k, r in tabs]


def _set(monkeypatch, env):
    for s in SWITCHES:
        for k in s:
            monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def expected_counters(ref, env):
    """(growth of counter 22, growth of counter 23) of one proof"""
    if "LMN_HOST_FS" in env:
        return 0, 0
    if "LMN_HOST_QUOT" in env or not ref.device:
        return 0, 1
    return 1, 0


def prove_counted(ctx, pie, luts, case, what):
    """-> (bytes, growth of counters 22 and 23); a refusal of a pie the oracle proves names what the library said"""
    before = ctx.counter(COUNTER_DEVICE), ctx.counter(COUNTER_HOST_WAIT)
    try:
        got = ctx.prove_tables(pie, luts)
    except backend.LuminairBackendError as e:
        hint = ""
        if e.code == backend.ERR_CONSTRAINTS:
            hint = (" - the composition identity fails at the library's own sampled values of a trace the oracle proves: "
                    "evaluation (eval_at_points) or the sample points")
        elif "quotient randomness" in str(e):
            hint = " - k_quot_prepare's mix of the sampled values (quotient tables) and the host's replay disagree"
        raise AssertionError("%s (%s): the library refuses a pie the oracle proves: %s%s" % (case.name, what, e, hint)) from e
    return got, (ctx.counter(COUNTER_DEVICE) - before[0], ctx.counter(COUNTER_HOST_WAIT) - before[1])


def check_case(provers, case, monkeypatch, kernels=None):
    """the default path, LMN_HOST_QUOT=1 and LMN_HOST_FS=1 on one context: the oracle's bytes, and the counters of the path"""
    ref = reference(case, kernels)
    assert ref.n_samples <= MAX_SAMPLES, "a proof with more samples than k_quot_prepare plans for: kernels.h says there is none"
    tabs, luts = case.tables()
    ctx, pie = provers.ctx(case), _pie(tabs)
    rng = np.random.default_rng(case.seed)
    for env in SWITCHES:
        what = " ".join("%s=%s" % kv for kv in env.items()) or "default"
        _set(monkeypatch, env)
        if case.dirty:
            nc.dirty_context(ctx, rng)
        got, grown = prove_counted(ctx, pie, luts, case, what)
        _same(got, ref.data, case, what)
        assert grown == expected_counters(ref, env), \
            "%s (%s): %d LDE sizes, %d samples: counters 22 / 23 grew by %s, expected %s" % (
                case.name, what, ref.n_sizes, ref.n_samples, grown, expected_counters(ref, env))
    _set(monkeypatch, {})


# ----------------------------------------------------------------------------- the matrix itself
def check_matrix_reaches_every_edge(cases=None):
    """from the oracle's proofs alone: what the module docstring promises of CASES"""
    cases = CASES if cases is None else cases
    refs = [(c, reference(c)) for c in cases]
    dev = [(c, r) for c, r in refs if r.device]
    host = [(c, r) for c, r in refs if not r.device]
    assert dev and host
    assert all(r.n_samples <= MAX_SAMPLES for _, r in refs)
    assert {r.n_samples % 4 for _, r in dev} == {0, 1, 2, 3}, sorted((r.n_samples, c.name) for c, r in dev)
    full = {r.blocks for _, r in dev if r.n_samples % 4 == 2}
    assert len(full) >= 2 and all((8 + 4 * r.n_samples) % 16 == 0 for _, r in dev if r.n_samples % 4 == 2), full
    for n in (MAX_SIZES, MAX_SIZES + 1):
        forms = {c.mults for c, r in refs if r.n_sizes == n and c.build is None}
        assert forms == {"zero", "chain"}, (n, forms)
    assert {r.n_sizes for _, r in dev} >= {1 + 1, MAX_SIZES} and min(r.n_sizes for _, r in host) == MAX_SIZES + 1
    assert max(r.n_points for _, r in refs) >= 10 and min(r.n_points for _, r in refs) == 2
    # all-zero interaction columns are sampled to exactly 0; the chain pies' are not all zero
    for c, r in refs:
        if c.build is not None:
            continue
        inter = [v for col in r.proof.proof.sampled_values[2] for v in col]
        assert all(v.is_zero() for v in inter) == (c.mults == "zero"), c.name
    # sub-table jobs (log < 10) next to jobs of 2 chunks (log 14), and the boundary sizes 2^9, 2^10, 2^11, 2^13
    logs = [set(ls for ls in r.proof.claim if ls is not None) for _, r in refs]
    assert any({4, 14} <= s for s in logs) and any({4, 9, 10, 11, 13} <= s for s in logs)


# ----------------------------------------------------------------------------- plain integers
def oods_point(proof, variant):
    """the OODS point by a replay of the transcript over the proof's commitments and claims (oracle.verifier's steps)"""
    s = proof.proof
    ch = Blake2sChannel(variant)
    ch.mix_root(s.commitments[0])
    for ls in proof.claim:
        if ls is not None:
            ch.mix_u64(ls)
    ch.mix_root(s.commitments[1])
    ch.draw_felts(2)
    for _ in range(4 if int(variant) & ProtocolVariant.LUT_DRAWS4 else 1):
        ch.draw_felts(2)
    for c in proof.interaction_claim:
        if c is not None:
            ch.mix_felts([c])
    ch.mix_root(s.commitments[2])
    ch.draw_felt()
    ch.mix_root(s.commitments[3])
    t = ch.draw_felt()
    t2 = t * t
    inv = (t2 + 1).inverse()
    return (ONE - t2) * inv, t.double() * inv


def padded_columns(lib, kind, rows):
    """the table's columns, padded to a power of two (at least 16 rows) with `lmn_kind_padding_row`"""
    n_cols = lib.kind_columns(kind)
    assert rows.shape[1] == n_cols
    pad = np.zeros(n_cols, dtype=np.uint32)
    assert lib.lib.lmn_kind_padding_row(kind, pad.ctypes.data_as(backend.C.POINTER(backend.C.c_uint32))) == 0
    size = max(16, 1 << int(len(rows) - 1).bit_length())
    out = np.empty((size, n_cols), dtype=np.uint64)
    out[:len(rows)] = rows
    out[len(rows):] = pad
    return np.ascontiguousarray(out.T)


def pin_tables():
    """PIN_CASE's tables, each three rows short of its power of two: the padding row is part of what is pinned"""
    assert max(PIN_CASE.logs) <= nc.PY_MAX_LOG
    return [(k, r[:-3]) for k, r in PIN_CASE.tables()[0]]


def check_sampled_values_against_plain_integers(lib):
    """every tree-1 column of a five-size pie, interpolated and evaluated at the OODS point with Python integers, equals
    `sampled_values[1]` of the oracle's proof: a mixed-size job table tied to plain integers (and, through the bytes, the
    library)"""
    tabs = pin_tables()
    ref = reference(PIN_CASE, tabs=tabs)
    x, y = oods_point(ref.proof, PIN_CASE.variant)
    pt = (tuple(int(v) for v in x.v), tuple(int(v) for v in y.v))
    want = ref.proof.proof.sampled_values[1]
    at = 0
    for kind, rows in tabs:
        cols = padded_columns(lib, kind, rows)
        assert cols.shape[1] == 1 << ref.proof.claim[kind]
        for c, co in enumerate(nc.ref_interpolate(cols)):
            got = nc.ref_eval_at_point(co, pt)
            assert len(want[at]) == 1 and got == tuple(int(v) for v in want[at][0].v), \
                "kind %d column %d (2^%d rows): plain integers %s, the oracle %s" % (kind, c, ref.proof.claim[kind], got, want[at][0].v)
            at += 1
    assert at == len(want)
    return tabs, ref


def check_pin_pie_on_library(provers, monkeypatch):
    """the pie of the plain-integer pin through the library: the same bytes"""
    tabs, ref = check_sampled_values_against_plain_integers(provers.lib)
    _set(monkeypatch, {})
    got, grown = prove_counted(provers.ctx(PIN_CASE), _pie(tabs), None, PIN_CASE, "default")
    _same(got, ref.data, PIN_CASE, "default")
    assert grown == (1, 0) and ref.device


# ----------------------------------------------------------------------------- batch library, back to back
EIGHT, NINE = BY_NAME["7 tables 2^4..2^10, chain multiplicities"], BY_NAME["8 tables 2^4..2^11, chain multiplicities"]


def check_batch_library(solo_lib, batch_so, monkeypatch):
    """three members of the 8-size shape with different seeds, three of the 9-size shape: each member's bytes equal the solo
    library's for the same pie (which check_case ties to the oracle for the seeds of CASES)"""
    from luminair_amd.batch import BatchProver
    _set(monkeypatch, {})
    provers = Provers(solo_lib)
    bp = BatchProver(0, 3, protocol_variant=backend.VARIANT_PINNED, library_path=batch_so)
    try:
        for shape in (EIGHT, NINE):
            pies = [_pie(edge_pie(shape.logs, shape.mults, seed)) for seed in (shape.seed, 31, 32)]
            want = [provers.ctx(shape).prove_tables(p) for p in pies]
            _same(want[0], reference(shape).data, shape, "solo library")
            assert len(set(want)) == 3
            got = bp.prove_batch(pies)
            for i in range(3):
                if got[i] != want[i]:
                    raise AssertionError("%s: member %d of the batch differs from its solo proof; first differing field: %s"
                                         % (shape.name, i, first_difference(got[i], want[i], shape.variant)))
    finally:
        bp.close()
        provers.close()


def check_back_to_back(lib, monkeypatch):
    """8 sizes, 9 sizes, 8 sizes on one context: the bytes of fresh contexts (plan and arena reuse across the path change)"""
    _set(monkeypatch, {})
    provers = Provers(lib)
    try:
        ctx = provers.ctx(EIGHT)
        for case, path in ((EIGHT, (1, 0)), (NINE, (0, 1)), (EIGHT, (1, 0))):
            fresh = backend.Context(0, provers.config(case), lib)
            try:
                want = fresh.prove_tables(_pie(case.tables()[0]))
            finally:
                fresh.close()
            _same(want, reference(case).data, case, "fresh context")
            got, grown = prove_counted(ctx, _pie(case.tables()[0]), None, case, "one context, back to back")
            _same(got, want, case, "one context, back to back")
            assert grown == path, (case.name, grown)
    finally:
        provers.close()
