"""Trace reuse (csrc/phase_trace.cpp run_main_trace, LMN_TRACE_REUSE; docs/HISTORY.md "Trace reuse"): the transforms of the
trace columns that depend on the graph alone are skipped when a context proves the same graph again.  The checks shared by
tests/test_trace_reuse_emu.py (emulation build, CPU suite) and tests/test_gpu_trace_reuse.py (MI355X).

Every proof of a sequence is compared byte for byte with the proof of a FRESH context under LMN_TRACE_REUSE=0 (`Env.want`,
computed once per pie), at 2^13 rows with the oracle's as well, and `lmn_ctx_counter` 20 / 21 - candidate columns compared,
columns whose transforms were skipped - say which path it took.

Shapes: 2^13 rows is the smallest table with the three-launch transform (the generic strided pass + the 12-layer pass), 2^18
the first with a fixed-shape strided pass (RB = 6); each once with a row count just below the power of two, so that padding
rows are compared, and once full."""
import os

import numpy as np

from luminair_amd import backend, synthetic as syn
from oracle import air
from oracle.channel import ProtocolVariant
from oracle.field import P
from oracle.proof import to_bincode
from oracle.prover import prove as oracle_prove

KAT, PINNED = ProtocolVariant.KAT, ProtocolVariant.PINNED
SWITCH = "LMN_TRACE_REUSE"
ADD, MUL, INPUTS = air.KIND_ADD, air.KIND_MUL, air.KIND_INPUTS
N_CAND = {ADD: 12, MUL: 12, INPUTS: 6}      # graph_only_columns (csrc/constraints.h): 12 of 15, 12 of 16, 6 of 7
ORACLE_LOG = 13                              # pies whose tables have at most 2^13 rows are compared with the oracle too

SMALL = [(13, (1 << 13) - 3), (13, 1 << 13)]
LARGE = [(18, (1 << 18) - 3), (18, 1 << 18)]


def shape_id(s):
    return "2^%d rows %s" % (s[0], "full" if s[1] == 1 << s[0] else "minus 3")


class Env:
    """a library, the reference proofs of the pies seen so far, and (optionally) the oracle's kernels"""

    def __init__(self, lib, kernels=None):
        self.lib, self.kernels, self.refs = lib, kernels, {}

    def cfg(self, variant):
        cfg = self.lib.default_config()
        cfg.protocol_variant = backend.VARIANT_PINNED if variant == PINNED else backend.VARIANT_KAT
        return cfg

    def ctx(self, variant=KAT):
        return backend.Context(0, self.cfg(variant), self.lib)

    def want(self, tabs, variant=KAT):
        """("ok", bytes) or ("err", code) of a fresh context under LMN_TRACE_REUSE=0; computed once per pie"""
        key = (int(variant),) + tuple((k, hash(np.ascontiguousarray(r).tobytes())) for k, r in tabs)
        if key not in self.refs:
            old = os.environ.get(SWITCH)
            os.environ[SWITCH] = "0"
            try:
                c = self.ctx(variant)
                res = outcome(c, [(k, r, len(r)) for k, r in tabs])
                assert c.counter(20) == 0 and c.counter(21) == 0
                c.close()
            finally:
                if old is None:
                    del os.environ[SWITCH]
                else:
                    os.environ[SWITCH] = old
            if res[0] == "ok" and max(len(r) for _, r in tabs) <= 1 << ORACLE_LOG:
                o = to_bincode(oracle_prove([(k, r.astype(np.uint64)) for k, r in tabs], variant=variant, kernels=self.kernels))
                assert res[1] == o, "the reference proof differs from the oracle's"
            self.refs[key] = res
        return self.refs[key]


def outcome(ctx, tables):
    try:
        return ("ok", ctx.prove_tables(tables))
    except backend.LuminairBackendError as e:
        return ("err", e.code)


class Session:
    """one context proving pies one after the other, device-resident rows by default; `step` checks bytes and counters"""

    def __init__(self, env, variant=KAT, resident=True):
        self.env, self.variant, self.resident = env, variant, resident
        self.ctx = env.ctx(variant)
        self.bufs = {}

    def counters(self):
        return self.ctx.counter(20), self.ctx.counter(21)

    def _tables(self, tabs):
        out = []
        for i, (k, r) in enumerate(tabs):
            if not self.resident:
                out.append((k, r, len(r)))
                continue
            key = (i, k, r.shape)
            if key in self.bufs:
                self.ctx.upload_to(self.bufs[key], r)
            else:
                self.bufs[key] = self.ctx.upload(r)
            out.append((k, self.bufs[key], len(r)))
        return out

    def step(self, tabs, compared, skipped, what=""):
        """prove `tabs`; the outcome is the fresh context's, counters 20 / 21 rise by `compared` / `skipped`"""
        c0, s0 = self.counters()
        got = outcome(self.ctx, self._tables(tabs))
        want = self.env.want(tabs, self.variant)
        assert got[0] == want[0] and got[1] == want[1], "%s: %s instead of %s" % (what, got[0], want[0])
        c1, s1 = self.counters()
        assert (c1 - c0, s1 - s0) == (compared, skipped), (what, c1 - c0, s1 - s0, compared, skipped)
        return got


def add_pie(n, seed):
    """one Add table: the graph's columns do not depend on the seed, lhs / rhs / out do"""
    return syn.config2_add_only(n, seed)


def with_word(tabs, table, row, col, value=None):
    """a copy with one word changed (by default: its lowest bit flipped)"""
    out = [(k, r.copy()) for k, r in tabs]
    r = out[table][1]
    r[row, col] = (int(r[row, col]) ^ 1) if value is None else value
    return out


# ------------------------------------------------------------------------------------------------ the sequences
def check_same_pie_then_new_values(env, shape):
    """1, 2: the first proof of a context compares nothing; the same pie again skips all 12 graph columns; so does the same
    graph on other values, whose bytes are the new pie's"""
    log, n = shape
    s = Session(env)
    a, b = add_pie(n, 100 + log), add_pie(n, 200 + log)
    assert not np.array_equal(a[0][1][:, 9:12], b[0][1][:, 9:12]) and np.array_equal(a[0][1][:, :9], b[0][1][:, :9])
    s.step(a, 0, 0, "first proof")
    t0 = s.ctx.timings()
    s.step(a, 12, 12, "same pie")
    got = s.step(b, 12, 12, "other values")
    assert got[1] != env.want(a)[1]
    # the timings say what ran: 12 columns less went through the transforms, 20 bytes and 1.5 log N butterflies per cell
    t1 = s.ctx.timings()
    N = 1 << log
    assert t0["fft_bytes"] - t1["fft_bytes"] == 12 * 20 * N, (t0["fft_bytes"], t1["fft_bytes"])
    assert t0["fft_butterflies"] - t1["fft_butterflies"] == 12 * (N // 2 + N) * log, (t0["fft_butterflies"], t1["fft_butterflies"])


def check_single_graph_words(env, shape, cells):
    """3: one word of one graph column changed against the previous pie: that column alone is transformed again (11 skipped).
    `cells`: (row, column) with negative rows counted from the last real row; the changes accumulate, so every step differs
    from the one before in exactly one column.  A changed next_idx breaks a transition: then the error is the parent's."""
    log, n = shape
    s = Session(env)
    cur = add_pie(n, 100 + log)
    s.step(cur, 0, 0)
    s.step(cur, 12, 12)
    for row, col in cells:
        cur = with_word(cur, 0, row if row >= 0 else n + row, col)
        s.step(cur, 12, 11, "word (%d, %d)" % (row, col))
    s.step(cur, 12, 12, "and again")


def check_other_shapes_skip_nothing(env, shape, and_back=True):
    """4: one row fewer (the padding row moves), another log_size, a Mul table of the same size: nothing is compared.
    and_back: the first pie again after each of them - nothing is compared then either"""
    log, n = shape
    s = Session(env)
    a = add_pie(n, 100 + log)
    s.step(a, 0, 0)
    s.step(a, 12, 12)
    others = [("one row fewer", [(ADD, a[0][1][:n - 1].copy())]), ("another log_size", add_pie((1 << (log + 1)) - 1, 7)),
              ("a Mul table of the same size", syn.config2_mul_only(n, 5))]
    for what, pie in others:
        s.step(pie, 0, 0, what)
        if and_back:
            s.step(a, 0, 0, "the first pie after " + what)
    if and_back:
        s.step(a, 12, 12, "and reuse again")


def check_other_arena_users(env, shape):
    """5: a trace check or a level-2 op between two proofs starts over in the arena: the next proof compares nothing"""
    log, n = shape
    s = Session(env)
    a = add_pie(n, 100 + log)
    s.step(a, 0, 0)
    s.step(a, 12, 12)
    rep = s.ctx.check_trace(s._tables(a))
    assert rep.ok
    s.step(a, 0, 0, "after lmn_trace_check")
    s.step(a, 12, 12)
    cols = np.arange(2 << 6, dtype=np.uint32).reshape(2, 1 << 6)
    s.ctx.interpolate(cols)
    s.step(a, 0, 0, "after a level-2 op")
    s.step(a, 12, 12)


def check_rejected_pies(env, shape):
    """6: a rejected pie leaves consistent blocks - its main-trace phase was enqueued whole - so the proof after it compares,
    skips what is unchanged against the REJECTED pie's columns, and is right"""
    log, n = shape
    s = Session(env)
    a = add_pie(n, 100 + log)
    s.step(a, 0, 0)
    bad_value = with_word(a, 0, 5, 9, P)                      # a non-canonical word in a value column
    got = s.step(bad_value, 12, 12, "non-canonical lhs")
    assert got == ("err", backend.ERR_INVALID_ARGUMENT)
    s.step(a, 12, 12, "after the rejected pie")
    bad_graph = with_word(a, 0, n - 1, 13, P + 1)             # ... in a graph column: that column is stale afterwards
    assert s.step(bad_graph, 12, 11, "non-canonical multiplicity") == ("err", backend.ERR_INVALID_ARGUMENT)
    s.step(a, 12, 11, "after the rejected graph column")
    broken = with_word(a, 0, 3, 11)                           # out of row 3: a broken constraint
    assert s.step(broken, 12, 12, "broken constraint") == ("err", backend.ERR_CONSTRAINTS)
    s.step(a, 12, 12, "after the broken pie")


def check_host_rows(env, shape):
    """7: host rows are staged in the arena in front of the columns: the same pie gets the same addresses"""
    log, n = shape
    s = Session(env, resident=False)
    a, b = add_pie(n, 100 + log), add_pie(n, 200 + log)
    s.step(a, 0, 0)
    s.step(a, 12, 12)
    s.step(b, 12, 12)
    s.step(with_word(b, 0, 0, 12), 12, 11)


def check_two_tables(env, log_add=13, brief=False):
    """8: Add + Inputs (the PINNED variant's balanced pie): 12 + 6 candidates; a change in one table's graph columns leaves the
    other table's alone.  brief: the first three proofs only"""
    s = Session(env, PINNED)
    a = syn.config2_graph_faithful(1 << log_add, 11)
    assert [k for k, _ in a] == [ADD, INPUTS]
    s.step(a, 0, 0)
    s.step(a, 18, 18)
    n_in = len(a[1][1])
    s.step(with_word(a, 1, n_in - 1, 6), 18, 17, "a multiplicity of Inputs")
    if brief:
        return
    s.step(with_word(a, 1, n_in - 1, 6), 18, 18)
    add_changed = with_word(a, 0, 0, 12)
    s.step(add_changed, 18, 16, "Inputs back, a multiplicity of Add")
    # another Inputs table (one row fewer): Add is still compared
    short = [add_changed[0], (INPUTS, a[1][1][:n_in - 1].copy())]
    s.step(short, 12, 12, "Inputs with one row fewer")


def check_sharded_leaves_counters_at_zero(env, shape):
    """9: a sharded context (a world of one rank, the thread transport of tests/test_sharded_prove.py)"""
    import test_sharded_prove as tsp
    log, n = shape
    a = add_pie(n, 100 + log)
    ctx = env.ctx()
    tsp._thread_shard(ctx, tsp._ThreadGroup(1), 0, 0)
    t = [(k, r, len(r)) for k, r in a]
    for _ in range(2):
        assert ("ok", ctx.prove_tables(t)) == env.want(a)
    assert (ctx.counter(20), ctx.counter(21)) == (0, 0)
    ctx.clear_shard()
    assert ("ok", ctx.prove_tables(t)) == env.want(a)
    assert (ctx.counter(20), ctx.counter(21)) == (0, 0)       # the first unsharded proof: the sharded ones left no record
    assert ("ok", ctx.prove_tables(t)) == env.want(a)
    assert (ctx.counter(20), ctx.counter(21)) == (12, 12)


def check_batch_library_leaves_counters_at_zero(env, batch_lib, shape):
    """9: the lock-step batch library's build of the prover never compares"""
    log, n = shape
    a = add_pie(n, 100 + log)
    ctx = backend.Context(0, batch_lib.default_config(), batch_lib)
    t = [(k, r, len(r)) for k, r in a]
    for _ in range(3):
        assert ("ok", ctx.prove_tables(t)) == env.want(a)
    assert (ctx.counter(20), ctx.counter(21)) == (0, 0)


def other_graph(tabs):
    """the same values under another graph of the same shape: all 12 graph columns of the Add table differ (where its rows
    break a transition the prover answers ConstraintsNotSatisfied, after all of its device work - as the parent does)"""
    r = tabs[0][1]
    n = len(r)
    lhs = np.where(r[:, 9] > P // 2, r[:, 9].astype(np.int64) - P, r[:, 9].astype(np.int64))
    rhs = np.where(r[:, 10] > P // 2, r[:, 10].astype(np.int64) - P, r[:, 10].astype(np.int64))
    o = syn.add_rows(lhs, rhs, node=5, lhs_id=3, rhs_id=4, mults=(2, 3, 4))
    o[:, 3] = (o[:, 3] + 1) % P
    o[:, 4] ^= 1
    o[:, 8] = (o[:, 8] + 1) % P
    assert len(o) == n and all(not np.array_equal(o[:, c], r[:, c]) for c in (0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 14))
    return [(ADD, o)]


REUSE_BACKOFF, REUSE_RETRY = 2, 64           # csrc/prover.h TraceReuse


def check_back_off(env, shape, retry=False):
    """two graphs of one shape in turn: after REUSE_BACKOFF = 2 compared proofs without one unchanged candidate the table is
    not compared any more, until its signature changes.  retry: or until the REUSE_RETRY-th proof since, which is compared
    once more - in vain while the graphs still alternate, for good once one of them stays"""
    log, n = shape
    s = Session(env)
    a = add_pie(n, 100 + log)
    b = other_graph(a)
    s.step(a, 0, 0)
    s.step(b, 12, 0, "another graph")
    s.step(a, 12, 0, "and back")
    s.step(b, 0, 0, "backed off")
    s.step(a, 0, 0, "backed off")
    s.step(a, 0, 0, "still backed off: the signature is the same")
    if retry:
        cur, count = a, REUSE_BACKOFF + 3                       # the record's count after the three proofs above
        while count < REUSE_RETRY:
            cur = b if cur is a else a
            s.step(cur, 0, 0, "backed off, count %d" % count)
            count += 1
        cur = b if cur is a else a
        s.step(cur, 12, 0, "the retry, in vain")
        for _ in range(3):
            s.step(cur, 0, 0, "backed off again")
        count = REUSE_RETRY + 1 + 3
        while count < 2 * REUSE_RETRY:
            s.step(cur, 0, 0, "one graph now, count %d" % count)
            count += 1
        s.step(cur, 12, 12, "the second retry finds it unchanged")
        s.step(cur, 12, 12, "and the back-off is over")
        return
    s.step([(ADD, a[0][1][:n - 1].copy())], 0, 0, "another signature")
    s.step(a, 0, 0, "the first signature again: a new record")
    s.step(a, 12, 12, "compared again")


def check_switch_off(env, shape):
    """LMN_TRACE_REUSE=0 on a context that has a record: nothing is compared, and the switch is read per proof"""
    log, n = shape
    s = Session(env)
    a = add_pie(n, 100 + log)
    s.step(a, 0, 0)
    os.environ[SWITCH] = "0"
    try:
        s.step(a, 0, 0, "switched off")
    finally:
        del os.environ[SWITCH]
    s.step(a, 0, 0, "on again: the proof before left no record")
    s.step(a, 12, 12)
