"""Checks of `lmn_trace_check` (luminair_amd.backend.Context.check_trace), shared by the emulation suite
(tests/test_trace_check_emu.py, in process) and the GPU suite (tests/test_gpu_trace_check.py, one child process per check:
`python tests/trace_doctor_checks.py <library> <check>`).

The reference of every comparison is the oracle: `oracle.air.COMPONENTS[kind].local` on `MV` columns for the local
constraints, the `Rel` entries of the component folded into a Python dict {(set, val, id): (net, first mention)} for the
relation balance, `oracle.air.preprocessed_column` for what the lookup tables read.  Never the library under test."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from luminair_amd import backend, synthetic as syn                                   # noqa: E402
from oracle import air                                                                # noqa: E402
from oracle.air import COMPONENTS, MV, preprocessed_column                            # noqa: E402

P = (1 << 31) - 1
CAP = backend.TRACE_REPORT_MAX
INV = backend.ERR_INVALID_ARGUMENT
KAT, PINNED = backend.VARIANT_KAT, backend.VARIANT_PINNED

_ctx_cache = {}


def ctx_for(lib, variant=PINNED):
    key = (id(lib), variant)
    if key not in _ctx_cache:
        cfg = lib.default_config()
        cfg.protocol_variant = variant
        _ctx_cache[key] = backend.Context(0, cfg, lib)
    return _ctx_cache[key]


def pie(tabs):
    return [(int(k), r, len(r)) for k, r in tabs]


# ------------------------------------------------------------------------------------------------ the oracle's report
class Ref:
    """what the oracle finds in a list of (kind, rows) tables"""

    def __init__(self, tabs, luts=None):
        self.n_noncanonical, self.first_noncanonical = 0, None
        self.constraints = []            # (table, kind, slot, count, first_row), sorted by (table, slot)
        self.slot_rows = {}              # (table, slot) -> (violating rows, examined rows)
        per_set = {}                     # set -> [key, signed multiplicity word, mention] arrays
        for t, (kind, rows) in enumerate(tabs):
            comp = COMPONENTS[int(kind)]
            rows = np.asarray(rows, dtype=np.uint64).reshape(-1, comp.n_cols)
            bad = rows >= P
            if bad.any():
                self.n_noncanonical += int(bad.sum())
                r, c = [int(x) for x in np.argwhere(bad)[0]]             # row-major: the smallest (row, column)
                if self.first_noncanonical is None:
                    self.first_noncanonical = (t, r, c)
            idx = np.nonzero(~bad.any(axis=1))[0]                        # rows holding such a word are left out
            good = rows[idx]
            cols = [MV(good[:, c]) for c in range(comp.n_cols)]
            for slot, v in enumerate(comp.local(cols)):
                nz = np.nonzero(np.broadcast_to(np.asarray(v.a), (len(good),)))[0]
                self.slot_rows[(t, slot)] = (len(nz), len(good))
                if len(nz):
                    self.constraints.append((t, int(kind), slot, len(nz), int(idx[nz[0]])))
            for j, rel in enumerate(comp.relations):
                mult = good[:, rel.mult]
                if rel.pre:
                    pre = [preprocessed_column(cid, luts) for cid in comp.pre_cols]
                    val = pre[rel.val][idx]
                    ident = pre[rel.id][idx] if rel.id is not None else np.zeros(len(idx), dtype=np.uint64)
                else:
                    val = good[:, rel.val]
                    ident = good[:, rel.id] if rel.id is not None else np.zeros(len(idx), dtype=np.uint64)
                on = mult != 0
                w = np.where(rel.neg, (P - mult) % P, mult)[on].astype(np.int64)
                key = (ident[on].astype(np.uint64) << np.uint64(31)) | val[on].astype(np.uint64)
                mention = (np.uint64(t) << np.uint64(40)) | (np.uint64(comp.n_local + j) << np.uint64(32)) | idx[on].astype(np.uint64)
                per_set.setdefault(rel.elems, []).append((key, w, mention))
        # the fold: net multiplicity and smallest mention per (set, val, id)
        self.tuples = {}
        for s, parts in per_set.items():
            key = np.concatenate([p[0] for p in parts])
            w = np.concatenate([p[1] for p in parts])
            mention = np.concatenate([p[2] for p in parts])
            uniq, inv = np.unique(key, return_inverse=True)
            net = np.zeros(len(uniq), dtype=np.int64)
            np.add.at(net, inv, w)                                       # < 2^26 rows x 7 x 2^31: exact in int64
            first = np.full(len(uniq), np.iinfo(np.uint64).max, dtype=np.uint64)
            np.minimum.at(first, inv, mention)
            for k, n, f in zip(uniq.tolist(), net.tolist(), first.tolist()):
                self.tuples[(s, k & P, k >> 31)] = (n % P, (f >> 40, (f >> 32) & 0xff, f & 0xffffffff))
        self.unbalanced = sorted(((s, v, i, net) + m for (s, v, i), (net, m) in self.tuples.items() if net),
                                 key=lambda u: (u[0], u[2], u[1]))
        self.ok = not self.n_noncanonical and not self.constraints and not self.unbalanced


def assert_equals_oracle(rep, ref, what):
    """every figure of the report against the oracle's, for equality"""
    assert rep.n_noncanonical == ref.n_noncanonical, (what, rep.n_noncanonical, ref.n_noncanonical)
    assert rep.first_noncanonical == ref.first_noncanonical, (what, rep.first_noncanonical, ref.first_noncanonical)
    assert rep.n_constraint_slots == len(ref.constraints), (what, rep.constraints, ref.constraints)
    assert rep.constraints == ref.constraints[:CAP], (what, rep.constraints, ref.constraints[:CAP])
    assert rep.constraints_truncated == (len(ref.constraints) > CAP), what
    assert rep.n_unbalanced == len(ref.unbalanced), (what, rep.n_unbalanced, len(ref.unbalanced))
    assert rep.tuples_truncated == (len(ref.unbalanced) > CAP), what
    if len(ref.unbalanced) <= CAP:
        assert rep.tuples == ref.unbalanced, (what, rep.tuples, ref.unbalanced)
    else:
        truth = set(ref.unbalanced)
        assert len(rep.tuples) == CAP and len(set(rep.tuples)) == CAP and all(u in truth for u in rep.tuples), what
    assert rep.ok == ref.ok and bool(rep.summary), (what, rep.summary)
    if not ref.ok:
        assert not rep.summary.startswith("ok"), rep.summary


def assert_clean(rep, what):
    assert rep.ok and rep.n_noncanonical == 0 and rep.first_noncanonical is None, (what, rep)
    assert rep.n_constraint_slots == 0 and rep.constraints == [] and not rep.constraints_truncated, (what, rep)
    assert rep.n_unbalanced == 0 and rep.tuples == [] and not rep.tuples_truncated, (what, rep)


def proves_and_verifies(ctx, tabs, luts=None):
    """(lmn_prove succeeded and lmn_verify accepted its bytes, what went wrong otherwise)"""
    try:
        proof = ctx.prove_tables(pie(tabs), luts)
        ctx.lib.verify(proof, int(ctx.config.protocol_variant))
        return True, ""
    except backend.LuminairBackendError as e:
        return False, "%d %s" % (e.code, e)


# ------------------------------------------------------------------------------------------------ 1: clean traces
def synthetic_pies():
    """(name, variant, tables, luts): the pies luminair_amd.synthetic builds, at sizes the emulation proves quickly"""
    act, act_luts = syn.activation_graph(24, ranges={"sin": (-40, 40), "exp2": (-30, 30), "log2": (1, 60)})
    bs, bs_luts = syn.config4_black_scholes_shape()
    return [("simple_example", KAT, syn.simple_example(), None),
            ("chain_graph", KAT, syn.chain_graph(37), None),
            ("sqrt_rem_graph", PINNED, syn.sqrt_rem_graph(21), None),
            ("activation_graph", PINNED, act, act_luts),
            ("less_than_graph", PINNED, syn.less_than_graph(19), None),
            ("linear_layer", KAT, syn.linear_layer(4, 8, with_max=True), None),
            ("config4_black_scholes_shape", PINNED, bs, bs_luts)]


def check_clean_synthetic(lib, skip_prove=()):
    """every pie reports ok; the same pie proves and verifies (skip_prove: names whose proof the caller leaves to another run)"""
    for name, variant, tabs, luts in synthetic_pies():
        ctx = ctx_for(lib, variant)
        assert Ref(tabs, luts).ok, name                                  # the oracle agrees that the pie is clean
        assert_clean(ctx.check_trace(pie(tabs), luts), name)
        if name not in skip_prove:
            ok, why = proves_and_verifies(ctx, tabs, luts)
            assert ok, (name, why)


def check_clean_producers(lib, builders=None, prove=True):
    """the producer scenarios: tables written by `DeviceGraph.gen_trace` on the device, checked where they lie"""
    import producer_scenarios as ps
    from luminair_amd.graph import DeviceGraph
    ctx = ctx_for(lib, PINNED)
    builders = builders if builders is not None else ps.EXPANSIONS + ps.OPS
    for n, build in enumerate(builders):
        g = DeviceGraph(ctx)
        for o in build(g, np.random.default_rng(42 + n)):
            g.output(o)
        tables, luts, bufs = g.gen_trace()
        try:
            assert_clean(ctx.check_trace(tables, luts), build.__name__)
            if prove:
                ctx.lib.verify(ctx.prove_tables(tables, luts), PINNED)
        finally:
            for b in bufs:
                b.free()


# ------------------------------------------------------------------------------------------------ 2: every slot, both ways
def _valid_rows(kind, n, rng):
    """n valid rows of a component with local constraints (multiplicities non-zero, so that relations are exercised too)"""
    a, b = rng.integers(1, 2048, size=n), rng.integers(1, 2048, size=n)
    if kind == air.KIND_ADD:
        return syn.add_rows(a - 1000, b, node=4, lhs_id=3, rhs_id=8, mults=(-1, 0, 1))
    if kind == air.KIND_MUL:
        return syn.mul_rows(a, b, node=3, lhs_id=6, rhs_id=7, mults=(0, -1, 2))
    if kind == air.KIND_RECIP:
        return syn.recip_rows(a + 7, node=5, input_id=4, mults=(-1, 1))
    if kind == air.KIND_SQRT:
        return syn.sqrt_rows(a, node=2, input_id=0, mults=(-1, 1))
    if kind == air.KIND_REM:
        return syn.rem_rows(a, b, node=3, lhs_id=2, rhs_id=1, mults=(-1, -1, 1))
    if kind == air.KIND_INPUTS:
        return syn.inputs_rows(a - 1000, 9, 3)
    if kind == air.KIND_CONTIGUOUS:
        return syn.contiguous_rows(a - 1000, node=2, input_id=0, input_mult=-1, out_mult=1)
    if kind in (air.KIND_SUM_REDUCE, air.KIND_MAX_REDUCE):
        f = syn.sum_reduce_rows if kind == air.KIND_SUM_REDUCE else syn.max_reduce_rows
        dim = 1 if n < 4 else 4 if n % 4 == 0 else n
        x = rng.integers(-2048, 2048, size=(n // dim, dim))
        return f(x, node=4, input_id=3, input_mult=-1, out_mult=1)
    if kind in (air.KIND_SIN, air.KIND_EXP2, air.KIND_LOG2):
        name = {air.KIND_SIN: "sin", air.KIND_EXP2: "exp2", air.KIND_LOG2: "log2"}[kind]
        return syn.unary_lut_rows(name, a, 1, node=10, input_id=0, mults=(-1, 1))[0]
    if kind == air.KIND_LESS_THAN:
        return syn.less_than_rows(a - 1000, b - 1000, node=4, lhs_id=3, rhs_id=2, mults=(-1, -1, 1))[0]
    raise ValueError(kind)


LOCAL_KINDS = [k for k in sorted(COMPONENTS) if COMPONENTS[k].n_local > 0]
SLOT_ROW_COUNTS = (1, 16, 17, 1000)


def slot_inputs(kind, seed=0):
    """(name, rows) per input of check 2: valid rows with a seeded sample of single-cell corruptions - every column is hit
    once the table has as many rows as columns - plus rows of random canonical words; for 1 row, each on its own"""
    comp = COMPONENTS[kind]
    out = []
    for n in SLOT_ROW_COUNTS:
        rng = np.random.default_rng([seed, kind, n])
        rows = _valid_rows(kind, n, rng)
        assert rows.shape == (n, comp.n_cols)
        random_rows = rng.integers(0, P, size=(n, comp.n_cols), dtype=np.uint64).astype(np.uint32)
        if n == 1:
            out += [("1 valid row", rows), ("1 random row", random_rows)]
            for c in range(comp.n_cols):
                one = rows.copy()
                one[0, c] = (int(one[0, c]) + 1 + int(rng.integers(0, P - 1))) % P
                out.append(("1 row, column %d changed" % c, one))
            continue
        rows = rows.copy()
        hit = rng.permutation(n)[:max(n // 3, 1)]
        for i, r in enumerate(hit):
            c = i % comp.n_cols if i < comp.n_cols else int(rng.integers(0, comp.n_cols))
            rows[r, c] = (int(rows[r, c]) + 1 + int(rng.integers(0, P - 1))) % P      # another canonical word
        rnd = rng.permutation(n)[:max(n // 8, 1)]
        rows[rnd] = random_rows[rnd]
        out.append(("%d rows" % n, rows))
    return out


def check_slots(lib, kinds=None):
    ctx = ctx_for(lib, PINNED)
    for kind in (kinds if kinds is not None else LOCAL_KINDS):
        comp = COMPONENTS[kind]
        violated, satisfied = set(), set()
        for name, rows in slot_inputs(kind):
            ref = Ref([(kind, rows)])
            for (_, slot), (n_bad, n_rows) in ref.slot_rows.items():
                if n_bad:
                    violated.add(slot)
                if n_bad < n_rows:
                    satisfied.add(slot)
            assert_equals_oracle(ctx.check_trace(pie([(kind, rows)])), ref, "%s, %s" % (comp.name, name))
        # the condition on the inputs, asserted of the ORACLE's results: every local slot seen violated and seen satisfied
        # (Mul's second slot is identically zero)
        zero_slots = {2} if kind == air.KIND_MUL else set()
        assert violated == set(range(comp.n_local)) - zero_slots, (comp.name, violated)
        assert satisfied == set(range(comp.n_local)), (comp.name, satisfied)


# ------------------------------------------------------------------------------------------------ 3: agreement with the prover
def prover_cases():
    """(name, variant, tables, luts): single-cell changes of small valid pies.  Between them the changes break a local
    constraint of every component that has one, so that the host's evaluation at the OODS point (the prover's self-check and
    lmn_verify) meets each component's constraints on a row that violates them as well as on rows that satisfy them."""
    def changed(tabs, t, r, c, delta):
        tabs = [(k, rows.copy()) for k, rows in tabs]
        tabs[t][1][r, c] = (int(tabs[t][1][r, c]) + delta) % P
        return tabs

    def of_kind(tabs, kind, r, c):                   # + 1 in row r, column c of the table of that kind
        return changed(tabs, [k for k, _ in tabs].index(kind), r, c, 1)
    se, lt = syn.simple_example(), syn.less_than_graph(19)
    # the smallest tables the prover takes: everything below 16 rows is padded to 2^4
    ch, sr, ll = syn.chain_graph(5), syn.sqrt_rem_graph(5), syn.linear_layer(2, 4, with_max=True)
    act = {n: syn.activation_graph(5, names=(n,), ranges={n: r}) for n, r in (("sin", (-7, 7)), ("exp2", (-7, 7)), ("log2", (1, 15)))}
    x = np.arange(5) - 2
    co = [(air.KIND_INPUTS, syn.inputs_rows(x, 0, 1)), (air.KIND_CONTIGUOUS, syn.contiguous_rows(x, node=2, input_id=0))]
    return [("simple_example unchanged", KAT, se, None),
            ("Mul out + 1", KAT, changed(se, 1, 2, 11, 1), None),
            ("Add lhs + 1", KAT, changed(se, 0, 0, 9, 1), None),
            ("Add is_last of a middle row", KAT, changed(se, 0, 1, 4, 1), None),
            ("Add next_node of the last row (unconstrained)", KAT, changed(se, 0, 3, 5, 7), None),
            ("Mul out multiplicity 2 -> 3", KAT, changed(se, 1, 0, 15, 1), None),
            ("Add lhs_id of the last row", KAT, changed(se, 0, 3, 1, 1), None),
            ("LessThan limb 0 + 1", PINNED, changed(lt, 1, 5, 14, 1), None),
            ("RangeCheckLookup multiplicity + 1", PINNED, changed(lt, 2, 200, 0, 1), None),
            # columns that no relation reads: the local constraint is the only thing the change breaks
            ("Recip rem + 1", KAT, of_kind(ch, air.KIND_RECIP, 2, 9), None),
            ("Sqrt rem + 1", PINNED, of_kind(sr, air.KIND_SQRT, 2, 9), None),
            ("Rem quotient + 1", PINNED, of_kind(sr, air.KIND_REM, 2, 12), None),
            ("Inputs idx of a middle row + 1", PINNED, of_kind(sr, air.KIND_INPUTS, 3, 1), None),
            ("SumReduce next_acc + 1", KAT, of_kind(ll, air.KIND_SUM_REDUCE, 1, 10), None),
            ("MaxReduce next_max + 1", KAT, of_kind(ll, air.KIND_MAX_REDUCE, 0, 10), None),
            ("Contiguous unchanged", PINNED, co, None),
            ("Contiguous idx of a middle row + 1", PINNED, of_kind(co, air.KIND_CONTIGUOUS, 1, 2), None),
            ("Sin idx of a middle row + 1", PINNED, of_kind(act["sin"][0], air.KIND_SIN, 1, 2), act["sin"][1]),
            ("Exp2 idx of a middle row + 1", PINNED, of_kind(act["exp2"][0], air.KIND_EXP2, 1, 2), act["exp2"][1]),
            ("Log2 idx of a middle row + 1", PINNED, of_kind(act["log2"][0], air.KIND_LOG2, 1, 2), act["log2"][1])]


def check_prover_agreement(lib):
    seen, broken = set(), set()
    for name, variant, tabs, luts in prover_cases():
        ctx = ctx_for(lib, variant)
        ref = Ref(tabs, luts)
        rep = ctx.check_trace(pie(tabs), luts)
        assert_equals_oracle(rep, ref, name)
        ok, why = proves_and_verifies(ctx, tabs, luts)
        assert rep.ok == ok, (name, rep.summary, why)
        seen.add(ok)
        broken |= {kind for _, kind, _, _, _ in ref.constraints}
        if "multiplicity" in name:                   # invisible to lmn_prove: it returns bytes, only the verifier objects
            assert not ok and str(backend.ERR_INVALID_LOGUP) in why.split()[0], (name, why)
    assert seen == {True, False}
    # the condition on the cases, asserted of the ORACLE's results: a local constraint of every component that has one is broken
    assert broken == set(LOCAL_KINDS), sorted(broken)


# ------------------------------------------------------------------------------------------------ 4: imbalances
def check_imbalances(lib):
    ctx = ctx_for(lib, KAT)
    # a consumer removed: nobody takes the Add outputs of the chain
    tabs = syn.chain_graph(20)[:2]
    ref = Ref(tabs)
    assert 0 < len(ref.unbalanced) <= CAP and not ref.constraints
    assert all(u[0] == air.ELEMS_NODE and u[2] == 4 and u[4:6] == (0, 8) for u in ref.unbalanced)   # Add (table 0) slot 6 + 2
    assert_equals_oracle(ctx.check_trace(pie(tabs)), ref, "consumer removed")
    # one id changed: the last Add row consumes tensor 2 instead of 3 - no local constraint sees it
    tabs = [(k, r.copy()) for k, r in syn.simple_example()]
    tabs[0][1][3, 1] = 2
    ref = Ref(tabs)
    assert len(ref.unbalanced) == 2 and not ref.constraints
    rep = ctx.check_trace(pie(tabs))
    assert_equals_oracle(rep, ref, "one id changed")
    assert "unbalanced" in rep.summary and "NodeElements" in rep.summary
    # more than the report holds
    tabs = syn.chain_graph(300)[:2]
    ref = Ref(tabs)
    assert len(ref.unbalanced) > CAP
    rep = ctx.check_trace(pie(tabs))
    assert rep.tuples_truncated and rep.n_unbalanced == len(ref.unbalanced) and len(rep.tuples) == CAP
    assert_equals_oracle(rep, ref, "more than 64 unbalanced tuples")


# ------------------------------------------------------------------------------------------------ 5: non-canonical words
def check_noncanonical(lib):
    ctx = ctx_for(lib, KAT)
    tabs = [(k, r.copy()) for k, r in syn.chain_graph(40)]
    tabs[1][1][7, 11] = P + 1                 # Mul out: as a canonical word it would break slot 1 and unbalance a tuple
    tabs[1][1][7, 3] = 0xffffffff
    tabs[1][1][30, 15] = P
    tabs[2][1][0, 12] = P + 5
    ref = Ref(tabs)
    assert ref.n_noncanonical == 4 and ref.first_noncanonical == (1, 7, 3)
    rep = ctx.check_trace(pie(tabs))
    assert_equals_oracle(rep, ref, "non-canonical words")
    assert not rep.ok and rep.constraints == [] and all(u[6] not in (7, 30) or u[4] != 1 for u in rep.tuples)
    # the same cells as canonical words: now the rows count
    tabs[1][1][7, 11] = 1
    tabs[1][1][7, 3], tabs[1][1][30, 15], tabs[2][1][0, 12] = 7, 1, 0
    ref = Ref(tabs)
    assert ref.n_noncanonical == 0 and ref.constraints
    assert_equals_oracle(ctx.check_trace(pie(tabs)), ref, "the same cells, canonical")


# ------------------------------------------------------------------------------------------------ 6: table forms
def check_table_forms(lib):
    ctx = ctx_for(lib, KAT)
    tabs = [(k, r.copy()) for k, r in syn.chain_graph(300)]
    tabs[0][1][299, 11] += 1
    tabs[1][1][17, 0] = P
    tabs[2][1][4, 11] = 5
    ref = Ref(tabs)
    host = ctx.check_trace(pie(tabs))
    assert_equals_oracle(host, ref, "host rows")
    bufs = [ctx.upload(r) for _, r in tabs]
    sinks = []
    try:
        dev = ctx.check_trace([(k, b, len(r)) for (k, r), b in zip(tabs, bufs)])
        assert dev == host, (dev, host)
        # a sink refuses a non-canonical word at finish: the sink form is compared on the tables without that cell
        tabs[1][1][17, 0] = 3
        host = ctx.check_trace(pie(tabs))
        assert_equals_oracle(host, Ref(tabs), "host rows (canonical)")
        for k, r in tabs:
            s = ctx.row_sink(k, len(r) + 5)
            s.push(r[:100]).push(r[100:]).finish()
            sinks.append(s)
        sunk = ctx.check_trace([(k, s, len(r)) for (k, r), s in zip(tabs, sinks)])
        assert sunk == host, (sunk, host)
        mixed = ctx.check_trace([(tabs[0][0], tabs[0][1], 300), (tabs[1][0], bufs[1], 300), (tabs[2][0], sinks[2], 300)])
        # (bufs[1] still holds the non-canonical cell)
        assert mixed.n_noncanonical == 1 and mixed.first_noncanonical == (1, 17, 0)
    finally:
        for s in sinks:
            s.close()
        for b in bufs:
            b.free()


# ------------------------------------------------------------------------------------------------ 7: refusals
def _codes(ctx, tables, luts):
    """(code, text) of lmn_trace_check and of lmn_prove for the same input"""
    out = []
    for f in (ctx.check_trace, ctx.prove_tables):
        try:
            f(tables, luts)
            out.append((0, ""))
        except backend.LuminairBackendError as e:
            out.append((e.code, str(e)))
    return out


def check_refusals(lib):
    ctx = ctx_for(lib, PINNED)
    L = lib.lib
    good = pie(syn.chain_graph(20))
    act, luts = syn.activation_graph(24, names=("sin",), ranges={"sin": (-40, 40)})
    act = pie(act)
    # null report
    arr, n, settings, _keep = ctx._marshal_tables(good, None)
    assert L.lmn_trace_check(ctx.handle, arr, n, C.byref(settings), None) == INV
    assert "report" in L.lmn_last_error(ctx.handle).decode()
    assert L.lmn_prove(ctx.handle, arr, n, C.byref(settings), None, None) == INV
    assert ctx.check_trace(good).ok
    cases = [("unsupported kind", [good[0], (99, good[1][1], 20)], None, 1),
             ("lookup table without its LUT", act, None, [k for k, _, _ in act].index(4)),
             ("lookup table of the wrong size", [(k, r[:len(r) // 4] if k == 4 else r, n // 4 if k == 4 else n) for k, r, n in act],
              luts, [k for k, _, _ in act].index(4)),
             ("descending kinds", good[::-1], None, 1),
             ("an empty table", [good[0], (good[1][0], good[1][1], 0)], None, 1)]
    for name, tables, lt, table in cases:
        (code, text), (pcode, ptext) = _codes(ctx, tables, lt)
        assert code == pcode and code != 0, (name, code, text, pcode, ptext)
        assert ("table %d " % table) in text, (name, text)
        assert ctx.check_trace(good).ok, name                            # the context is usable afterwards
    assert_clean(ctx.check_trace(act, luts), "the lookup pie itself")
    check_refusals_rule_by_rule(lib)


def _raw_codes(ctx, arr, n, settings):
    """(code, text) of lmn_trace_check and of lmn_prove on structs made by hand"""
    L = ctx.lib.lib
    rep = backend.LmnTraceReport()
    code = L.lmn_trace_check(ctx.handle, arr, n, C.byref(settings), C.byref(rep))
    text = L.lmn_last_error(ctx.handle).decode() if code else ""
    out, out_len = C.POINTER(C.c_uint8)(), C.c_size_t()
    pcode = L.lmn_prove(ctx.handle, arr, n, C.byref(settings), C.byref(out), C.byref(out_len))
    ptext = L.lmn_last_error(ctx.handle).decode() if pcode else ""
    if pcode == 0:
        L.lmn_free(out)
    return (code, text), (pcode, ptext)


def _prepare_code(ctx, settings, lookups):
    """the code lmn_settings_prepare answers the same lmn_settings with (tests/prepared_checks.py _raw_prepare)"""
    L = ctx.lib.lib
    h = C.c_void_p()
    rc = L.lmn_settings_prepare(0, C.byref(ctx.config), C.byref(settings), lookups, C.byref(h))
    if rc == 0:
        L.lmn_prepared_destroy(h)
    return rc


def check_refusals_rule_by_rule(lib):
    """One case per rule of the prover's input checks that `check_refusals` above does not reach: the same non-zero code from
    lmn_trace_check and lmn_prove, the table named where the rule belongs to one, a context that checks a good pie
    afterwards.  The smallest shapes that reach each rule: 16- to 32-row tables, the 256-row range check, 16-row LUTs."""
    kat, pinned = ctx_for(lib, KAT), ctx_for(lib, PINNED)
    cfg = lib.default_config()
    cfg.protocol_variant = PINNED
    cfg.log_last_layer = 4
    last4 = backend.Context(0, cfg, lib)
    good = pie(syn.chain_graph(20))                                      # Add, Mul, Recip: 20 rows each, padded to 32
    rows16 = syn.config2_add_only(16, 3)[0][1]
    lt = pie(syn.less_than_graph(19))
    rc_at = [k for k, _, _ in lt].index(air.KIND_RANGE_CHECK_LOOKUP)
    act, luts = syn.activation_graph(5, names=("sin",), ranges={"sin": (-7, 7)})
    act = pie(act)
    sin_at = [k for k, _, _ in act].index(air.KIND_SIN_LOOKUP)
    assert len(luts["sin"][0]) == 16 and len(lt[rc_at][1]) == 256
    assert kat.check_trace(good).ok and last4.check_trace(good).ok and pinned.check_trace(act, luts).ok

    def first_bad(c0, c1):
        c0 = c0.copy()
        c0[0] = P
        return {"sin": (c0, c1)}

    def last_bad(c0, c1):
        c1 = c1.copy()
        c1[-1] = P
        return {"sin": (c0, c1)}

    col = np.arange(16, dtype=np.uint32)
    p = col.ctypes.data

    def with_luts(*luts_c):
        def change(arr, st, keep):
            keep.append((backend.LmnLut * len(luts_c))(*luts_c))
            st.luts, st.n_luts = keep[-1], len(luts_c)
        return change

    def null_luts(arr, st, keep):
        st.luts, st.n_luts = C.POINTER(backend.LmnLut)(), 1

    # (name, context, tables, luts, change of the marshalled structs, table the text names, lookups for lmn_settings_prepare)
    cases = [("no claim slot under the KAT variant", kat, [good[0], (air.KIND_EXP2, good[1][1], 20)], None, None, 1, None),
             ("2^26 + 1 rows", pinned, [(0, rows16, (1 << 26) + 1)], None, None, 0, None),
             ("2^25 + 1 rows", pinned, [(0, rows16, (1 << 25) + 1)], None, None, 0, None),
             ("no more than 2^log_last_layer rows", last4, [(0, rows16, 16)] + good[1:], None, None, 0, None),
             ("both *_ON_DEVICE flags", pinned, good, None,
              lambda arr, st, keep: setattr(arr[1], "flags", backend.TABLE_ROWS_ON_DEVICE | backend.TABLE_COLS_ON_DEVICE), 1, None),
             ("null rows", pinned, good, None, lambda arr, st, keep: setattr(arr[2], "rows", None), 2, None),
             ("a lookup announced without its table", pinned, good, None,
              lambda arr, st, keep: setattr(st, "has_lookups", backend.LOOKUP_SIN), None, None),
             ("null luts with n_luts > 0", pinned, good, None, null_luts, None, backend.LOOKUP_SIN),
             ("unknown LUT kind", pinned, good, None, with_luts(backend.LmnLut(3, 4, p, p)), None, backend.LOOKUP_SIN),
             ("null LUT column", pinned, good, None, with_luts(backend.LmnLut(0, 4, p, None)), None, backend.LOOKUP_SIN),
             ("duplicate LUT", pinned, good, None, with_luts(backend.LmnLut(0, 4, p, p), backend.LmnLut(0, 4, p, p)), None,
              backend.LOOKUP_SIN),
             ("RangeCheckLookup of 16 rows", pinned, [(k, r[:16], 16) if i == rc_at else (k, r, n) for i, (k, r, n) in enumerate(lt)],
              None, None, rc_at, None),
             ("first LUT word 2^31 - 1", pinned, act, first_bad(*luts["sin"]), None, sin_at, None),
             ("last LUT word 2^31 - 1", pinned, act, last_bad(*luts["sin"]), None, sin_at, None)]
    try:
        for name, ctx, tables, lut_dict, change, table, lookups in cases:
            arr, n, settings, keep = ctx._marshal_tables(tables, lut_dict)
            if change:
                change(arr, settings, keep)
            (code, text), (pcode, ptext) = _raw_codes(ctx, arr, n, settings)
            assert code == pcode and code != 0, (name, code, text, pcode, ptext)
            assert text and ptext, name
            if table is not None:
                assert ("table %d " % table) in text, (name, text)
            if lookups is not None:
                assert _prepare_code(ctx, settings, lookups) == code, name
            assert ctx.check_trace(good).ok, name                        # the context is usable afterwards
    finally:
        last4.close()


# ------------------------------------------------------------------------------------------------ 8: hot keys
def check_hot_keys(lib, clean_too=True):
    """a LessThan table of 2^16 rows: 2^18 limbs on the 256 keys of the range check"""
    ctx = ctx_for(lib, PINNED)
    tabs = syn.less_than_graph(1 << 16)
    assert len(tabs[1][1]) >= 1 << 16 and len(tabs[2][1]) == 256
    if clean_too:
        assert_clean(ctx.check_trace(pie(tabs)), "less_than_graph(2^16)")
    tabs = [(k, r.copy()) for k, r in tabs]
    tabs[2][1][7, 0] += 1                    # the lookup yields limb value 7 once too often
    tabs[1][1][65000, 15] = 300              # a limb outside the 8-bit range: a key the lookup table does not have
    tabs[1][1][12345, 21] = 0                # a row that claims no range check at all
    ref = Ref(tabs)
    assert len([u for u in ref.unbalanced if u[0] == air.ELEMS_RANGE_CHECK]) >= 3
    assert_equals_oracle(ctx.check_trace(pie(tabs)), ref, "hot keys, three cells changed")


# ------------------------------------------------------------------------------------------------ 9: batch library
def check_batch_solo(lib, batch_lib):
    tabs = [(k, r.copy()) for k, r in syn.chain_graph(300)]
    tabs[0][1][299, 11] += 1
    tabs[1][1][17, 0] = P
    tabs[2][1][4, 11] = 5
    act, luts = syn.activation_graph(24, ranges={"sin": (-40, 40), "exp2": (-30, 30), "log2": (1, 60)})
    act[0][1][3, 8] += 1
    for variant, t, lt in ((KAT, tabs, None), (PINNED, act, luts)):
        main = ctx_for(lib, variant).check_trace(pie(t), lt)
        solo = ctx_for(batch_lib, variant).check_trace(pie(t), lt)
        assert_equals_oracle(main, Ref(t, lt), "main library")
        assert solo == main, (solo, main)


# ------------------------------------------------------------------------------------------------ 10: full size (GPU only)
def check_full_size(lib):
    """BASELINE config 2a (2^20 Add rows resident in HBM) and config 3 (2^21 + 2^20 + 2^20 rows, host): clean; with one cell
    changed near the last real row the report names that row"""
    ctx = ctx_for(lib, KAT)
    for name, tabs, resident in (("config 2a", syn.config2_add_only(1 << 20), True), ("config 3", syn.config3_mixed(), False)):
        def run(tabs):
            if not resident:
                return ctx.check_trace(pie(tabs))
            bufs = [ctx.upload(r) for _, r in tabs]
            try:
                return ctx.check_trace([(k, b, len(r)) for (k, r), b in zip(tabs, bufs)])
            finally:
                for b in bufs:
                    b.free()
        assert Ref(tabs).ok, name
        assert_clean(run(tabs), name)
        t = len(tabs) - 1
        row = len(tabs[t][1]) - 3
        out_col = {air.KIND_ADD: 11, air.KIND_RECIP: 8}[tabs[t][0]]
        tabs[t][1][row, out_col] = (int(tabs[t][1][row, out_col]) + 1) % P
        ref = Ref(tabs)
        assert ref.constraints == [(t, tabs[t][0], 1, 1, row)], (name, ref.constraints)
        rep = run(tabs)
        assert_equals_oracle(rep, ref, name + ", one cell changed")
        assert ("row %d" % row) in rep.summary, rep.summary


CHECKS = {"clean_synthetic": check_clean_synthetic, "clean_producers": check_clean_producers, "slots": check_slots,
          "prover_agreement": check_prover_agreement, "imbalances": check_imbalances, "noncanonical": check_noncanonical,
          "table_forms": check_table_forms, "refusals": check_refusals, "hot_keys": check_hot_keys,
          "full_size": check_full_size}


if __name__ == "__main__":
    library = backend.Library(sys.argv[1])
    if sys.argv[2] == "batch_solo":
        check_batch_solo(library, backend.Library(sys.argv[3]))
    else:
        CHECKS[sys.argv[2]](library)
    print("ok " + sys.argv[2])
