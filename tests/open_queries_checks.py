"""Checks of openings planned on the device (`lmn_positions_*`, `lmn_open_queries`, `lmn_col_fri_close_keep`;
luminair_amd.backend.Positions, Context.open_queries, Context.fri_close(keep=True)), shared by the emulation suite
(tests/test_open_queries_emu.py) and the GPU suite (tests/test_gpu_open_queries.py), both in process.  Every comparison
is exact.  The references are `Tree.decommit` (the host walk of lmn_tree_decommit) with the folded groups, the oracle's
`MerkleTree.decommit` / `verify_decommitment`, and the oracle's `decommit_positions_and_witness` for the pair expansion."""
import ctypes as C

import numpy as np

import fri_close_checks as fc
import level2_decommit_checks as dc
from luminair_amd import backend, synthetic as syn
from oracle.merkle import MerkleTree, verify_decommitment
from oracle.prover import decommit_positions_and_witness, fold_positions

INV = backend.ERR_INVALID_ARGUMENT
PAIRS = backend.OPEN_FRI_PAIRS

# every tree of level2_decommit_checks.SHAPES, a FRI-like tree of three sizes, and a trace-like tree of two
SHAPES = list(dc.SHAPES) + [("secure columns of three sizes", [(4, 11), (4, 10), (4, 3)]),
                            ("15 columns and a secure column", [(15, 12), (4, 11)])]
PAIR_SHAPES = [name for name, shape in SHAPES if all(n == 4 and lg > 0 for n, lg in shape)]
assert PAIR_SHAPES == ["a secure column alone", "secure columns of three sizes"]


class Shape:
    """a committed tree with its oracle twin, built once per (library, shape) and left unchanged"""

    def __init__(self, ctx, si):
        self.name, self.shape = SHAPES[si]
        self.t = dc.Committed(ctx, self.shape, 300 + si)
        self.ref = MerkleTree(self.t.columns)
        assert self.t.tree.root() == self.ref.root(), self.name
        self.sizes = sorted(set(self.t.log_sizes), reverse=True)
        self.top = self.t.max_log
        # {log size: the (4, n) host array of that size} for the trees the pair expansion applies to
        self.secure = {lg: a for a, (n, lg) in zip(self.t.host, self.shape)} if self.name in PAIR_SHAPES else None

    def item(self, flags=0):
        return (self.t.tree, self.t.handles, flags)


_shapes = {}


def shape_for(lib, si):
    key = (id(lib), si)
    if key not in _shapes:
        _shapes[key] = Shape(dc.ctx_for(lib), si)
    return _shapes[key]


def position_sets(log_domain, pairs_2_11=False):
    """(name, ascending distinct positions) in the domain 2^log_domain"""
    n = 1 << log_domain
    last = n - 1
    k = (last // 2) & ~1
    sets = [("empty", []), ("one position", [last // 3]), ("0 and the last", sorted({0, last}))]
    if n >= 2:
        sets.append(("both children of a node", [k, k + 1]))
    if n >= 4:
        sets.append(("neighbours in different pairs", [k + 1, k + 2] if k + 2 < n else [1, 2]))
        j = (last // 8) * 4
        sets.append(("four consecutive positions under one node", [j, j + 1, j + 2, j + 3]))
    if log_domain <= 10:
        sets.append(("every position", list(range(n))))
    if log_domain >= 11:
        rng = np.random.default_rng(900 + log_domain)
        for count in (63, 64, 65, 1024):
            drawn = set()
            while len(drawn) < count:
                drawn.update(int(x) for x in rng.integers(0, n, size=count - len(drawn)))
            sets.append(("%d seeded positions" % count, sorted(drawn)))
    if pairs_2_11:
        sets.append(("the 1024 even positions", list(range(0, 2048, 2))))
    return sets


def groups_of(s, positions, log_domain):
    return {lg: fold_positions(positions, log_domain - lg) for lg in s.sizes}


class _HostSecure:
    """`secure_at` of the oracle's kernel set on a (4, n) host array"""

    @staticmethod
    def secure_at(col, pos):
        return tuple(int(w) for w in col[:, pos])


def expected_pairs(s, positions, log_domain):
    """-> (the expanded groups, the FRI witness): per size, descending, `decommit_positions_and_witness(col, folded, 1)`"""
    groups, wit = {}, []
    for lg in s.sizes:
        dec, w = decommit_positions_and_witness(s.secure[lg], fold_positions(positions, log_domain - lg), 1, _HostSecure)
        groups[lg] = dec
        wit += w
    return groups, wit


def assert_opening(got, want, what):
    want_v, want_h, want_c = want
    assert got.queried_values.dtype == np.uint32 and got.column_witness.dtype == np.uint32
    assert got.queried_values.tolist() == [int(v) for v in want_v], what
    assert got.hash_witness == list(want_h), what
    assert got.column_witness.tolist() == [int(v) for v in want_c], what


def open_one(ctx, s, positions, log_domain, flags=0):
    pos = ctx.positions_from_cpu(positions, log_domain)
    try:
        assert pos.log_domain == log_domain and pos.to_cpu() == list(positions)
        return ctx.open_queries(pos, [s.item(flags)])[0]
    finally:
        pos.free()


# ------------------------------------------------------------------------------------------------ A
def check_opening(lib, si, extra_log):
    """A: one tree, every position set, log_domain = the tree's top log + extra_log; without the flag against the host
    walk and the oracle, with it against the oracle's pair expansion"""
    ctx = dc.ctx_for(lib)
    s = shape_for(lib, si)
    D = s.top + extra_log
    for name, positions in position_sets(D):
        what = (s.name, D, name)
        groups = groups_of(s, positions, D)
        got = open_one(ctx, s, positions, D)
        assert got.fri_witness == [], what
        vals, hw, cw = s.t.tree.decommit(s.t.handles, groups)
        assert_opening(got, (vals.tolist(), hw, cw.tolist()), what)
        assert_opening(got, s.ref.decommit(groups), what)
        if positions:
            assert verify_decommitment(s.t.tree.root(), s.t.log_sizes, groups, got.queried_values.tolist(), got.hash_witness,
                                       got.column_witness.tolist()), what
        else:
            assert len(got.queried_values) == 0 and got.hash_witness == [] and len(got.column_witness) == 0, what
        if name == "every position":
            assert got.hash_witness == [] and len(got.column_witness) == 0, what
            assert len(got.queried_values) == sum(1 << lg for lg in s.t.log_sizes), what
    if s.name not in PAIR_SHAPES:
        return
    for name, positions in position_sets(D, pairs_2_11=(D == 11 and s.top == 11)):
        what = (s.name, D, name, "pairs")
        groups, wit = expected_pairs(s, positions, D)
        got = open_one(ctx, s, positions, D, PAIRS)
        assert got.fri_witness == wit, what
        assert_opening(got, s.ref.decommit(groups), what)
        if positions:
            assert verify_decommitment(s.t.tree.root(), s.t.log_sizes, groups, got.queried_values.tolist(), got.hash_witness,
                                       got.column_witness.tolist()), what
        if name == "both children of a node" and extra_log == 0:
            assert len(got.fri_witness) == sum(1 for lg in s.sizes if lg < s.top), what   # none at the top: the pair is whole
        if name == "the 1024 even positions":
            # every pair is half-queried: all 2048 leaves are opened, 1024 witness values at the top size and - every
            # smaller size being queried whole - none below, and no hash anywhere
            assert groups[11] == list(range(2048)) and len(got.fri_witness) == 1024, what
            assert wit == [_HostSecure.secure_at(s.secure[11], p) for p in range(1, 2048, 2)], what
            assert got.hash_witness == [] and len(got.column_witness) == 0, what


# ------------------------------------------------------------------------------------------------ B
def check_many_items(lib):
    """B: three items - two over the same tree with different flags, one of another size - equal three separate calls, with
    one plan launch, one fetch launch and one wait for all of them"""
    ctx = dc.ctx_for(lib)
    a, b = shape_for(lib, SHAPES.index(next(x for x in SHAPES if x[0] == "secure columns of three sizes"))), shape_for(lib, 0)
    D = 13
    positions = position_sets(D)[-2][1]                       # 65 seeded positions
    assert len(positions) == 65
    pos = ctx.positions_from_cpu(positions, D)
    try:
        items = [a.item(0), b.item(0), a.item(PAIRS)]
        counters = (backend.COUNTER_OPEN_PLAN_LAUNCHES, backend.COUNTER_OPEN_FETCH_LAUNCHES, backend.COUNTER_OPEN_WAITS)
        before = [ctx.counter(c) for c in counters]
        together = ctx.open_queries(pos, items)
        assert [ctx.counter(c) - x for c, x in zip(counters, before)] == [1, 1, 1]
        apart = [ctx.open_queries(pos, [it])[0] for it in items]
        for k, (x, y) in enumerate(zip(together, apart)):
            assert x.fri_witness == y.fri_witness and x.hash_witness == y.hash_witness, k
            assert np.array_equal(x.queried_values, y.queried_values) and np.array_equal(x.column_witness, y.column_witness), k
        assert_opening(together[0], a.ref.decommit(groups_of(a, positions, D)), "item 0")
        assert_opening(together[1], b.ref.decommit(groups_of(b, positions, D)), "item 1")
        groups, wit = expected_pairs(a, positions, D)
        assert together[2].fri_witness == wit and together[0].fri_witness == []
        assert_opening(together[2], a.ref.decommit(groups), "item 2")
        # no items: nothing is launched
        before = [ctx.counter(c) for c in counters]
        assert ctx.open_queries(pos, []) == []
        assert [ctx.counter(c) for c in counters] == before
    finally:
        pos.free()


# ------------------------------------------------------------------------------------------------ C
def _same_close(a, b):
    return (a.coeffs, a.first_bad, a.nonce, a.positions, a.digest_after_coeffs, a.digest_after_nonce, a.digest_end,
            a.n_sent_end) == (b.coeffs, b.first_bad, b.nonce, b.positions, b.digest_after_coeffs, b.digest_after_nonce,
                              b.digest_end, b.n_sent_end)


def _keep_and_compare(lib, ctx, values, start, lqd, what):
    """fri_close(keep=True) against fri_close on the same input; the handle against the result's positions; a tree opened
    with the handle against the same tree opened with positions_from_cpu(result.positions)"""
    col = ctx.col_from_cpu(np.ascontiguousarray(values.T))
    try:
        plain = ctx.fri_close(col, start, lqd)
        kept, pos = ctx.fri_close(col, start, lqd, keep=True)
    finally:
        col.free()
    try:
        assert _same_close(kept, plain), what
        assert pos.log_domain == lqd and pos.to_cpu() == plain.positions, what
        if lqd >= 6:
            # a 2^6 tree of the closing context, opened with the kept handle and with the result's positions
            rng = np.random.default_rng(5)
            host = rng.integers(0, dc.P, size=(3, 64), dtype=np.uint64).astype(np.uint32)
            h = ctx.col_from_cpu(host)
            tree = ctx.commit([h])
            again = ctx.positions_from_cpu(plain.positions, lqd)
            try:
                x, y = ctx.open_queries(pos, [(tree, [h])])[0], ctx.open_queries(again, [(tree, [h])])[0]
                assert_opening(x, (y.queried_values.tolist(), y.hash_witness, y.column_witness.tolist()), what)
                assert_opening(x, MerkleTree(list(host)).decommit({6: fold_positions(plain.positions, lqd - 6)}), what)
            finally:
                again.free()
                tree.free()
                h.free()
        return plain
    finally:
        pos.free()


def check_keep_draws(ctxs, n_queries, u32_counter):
    variant = backend.PV_DRAW_CTR_U32 if u32_counter else backend.VARIANT_KAT
    ctx = ctxs.get(n_queries=n_queries, variant=variant)
    values, coeffs = fc.layer("random", 0, 1)
    for lqd in ((4, 12) if n_queries == 70 else (12,)):
        got = _keep_and_compare(ctxs.lib, ctx, values, fc.digest_of(7000 + 40 * n_queries + lqd), lqd, (n_queries, u32_counter, lqd))
        if lqd == 4 and n_queries == 70:
            assert len(got.positions) < 70                               # heavy duplicates
        assert len(got.positions) <= n_queries


def check_keep_fallback(ctxs):
    """a nonce beyond the queued windows (2^11-nonce windows, pow_bits 16): the handle is filled from the host's positions.
    The seed is the op's own second GRIND_SEEDS_16 seed - a start digest whose nonce lies past the queue; FALLBACK_SEEDS
    of fri_close_checks are table seeds of whole proofs and do not apply to a call on a handle."""
    variant = backend.PV_MIX_U64_HASHED
    seed = fc.GRIND_SEEDS_16[variant][1]
    ll, lb = fc.GRIND_SHAPE
    values, coeffs = fc.layer("random", ll, lb)
    ctx = ctxs.get(log_last_layer=ll, log_blowup=lb, pow_bits=16, variant=variant)
    got = _keep_and_compare(ctxs.lib, ctx, values, fc.digest_of(seed), 12, "fallback")
    assert got.grind_rounds >= 1 and got.nonce >= fc.QUEUED
    fc.compare(got, coeffs, 1 << ll, fc.grind_reference(variant, 16, seed), "fallback")


# ------------------------------------------------------------------------------------------------ D
def _raw_open(ctx, pos, items, n_items=None, null=()):
    """the C call itself -> (rc, error text, the results)"""
    L = ctx.lib.lib
    n = len(items)
    c_items = (backend.LmnOpenItem * max(n, 1))()
    keep = []
    for k, (tree, cols, flags, *rest) in enumerate(items):
        arr = (C.c_void_p * max(len(cols), 1))(*[getattr(c, "handle", c) for c in cols])
        keep.append(arr)
        c_items[k] = backend.LmnOpenItem(getattr(tree, "handle", tree), None if "cols" in rest else arr, len(cols), flags)
    res = (backend.LmnOpening * max(n, 1))()
    for r in res:
        r.queried_values, r.n_values, r.n_fri_words = 1, 9, 9
    rc = L.lmn_open_queries(ctx.handle, getattr(pos, "handle", pos), None if "items" in null else c_items,
                            n if n_items is None else n_items, None if "out" in null else res)
    text = L.lmn_last_error(ctx.handle).decode()
    outs = [(r.queried_values, r.hash_witness, r.column_witness, r.fri_witness, r.n_values, r.n_hashes, r.n_column_words,
             r.n_fri_words) for r in res[:n]]
    if rc == backend.LMN_OK:
        for r in res[:n]:
            for name in ("queried_values", "hash_witness", "column_witness", "fri_witness"):
                if getattr(r, name):
                    L.lmn_free(getattr(r, name))
    return rc, text, outs


ZERO = (None, None, None, None, 0, 0, 0, 0)


def check_refusals(lib):
    """D: every refusal names its argument, zeroes the outputs, launches nothing and leaves context and handles usable"""
    ctx = dc.ctx_for(lib)
    L = ctx.lib.lib
    s = shape_for(lib, SHAPES.index(next(x for x in SHAPES if x[0].startswith("three sizes"))))   # (3,5) (2,7) (1,4)
    sec = shape_for(lib, SHAPES.index(next(x for x in SHAPES if x[0] == "a secure column alone")))  # (4, 8)
    low = shape_for(lib, SHAPES.index(next(x for x in SHAPES if x[0] == "log sizes 1 and 0")))
    tree, handles = s.t.tree, s.t.handles
    D = 9
    good = [3, 100, 101, 511]
    pos = ctx.positions_from_cpu(good, D)
    small = ctx.positions_from_cpu([1, 2], 5)
    full = ctx.positions_from_cpu(list(range(0, 2048, 2)), 27)
    other = ctx.col_from_cpu(np.zeros((1, 128), np.uint32))
    big = ctx.col_from_cpu(np.zeros((1, 256), np.uint32))
    wide = ctx.col_from_cpu(np.zeros((4096, 1 << 10), np.uint32))         # 1024 positions may open 4096 x 1024 words of it
    wide_tree = ctx.commit([wide])
    counters = (backend.COUNTER_OPEN_PLAN_LAUNCHES, backend.COUNTER_OPEN_FETCH_LAUNCHES, backend.COUNTER_OPEN_WAITS)

    def good_call(what):
        got = ctx.open_queries(pos, [(tree, handles)])[0]
        assert_opening(got, s.ref.decommit(groups_of(s, good, D)), what)

    try:
        good_call("before")
        a, b, c = handles
        cases = [
            ("null positions", dict(pos=None, items=[(tree, handles, 0)]), ("positions is null",)),
            ("null items", dict(pos=pos, items=[(tree, handles, 0)], null=("items",)), ("items is null", "n_items = 1")),
            ("null out", dict(pos=pos, items=[(tree, handles, 0)], null=("out",)), ("out is null",)),
            ("null tree", dict(pos=pos, items=[(None, handles, 0)]), ("items[0].tree is null",)),
            ("null cols", dict(pos=pos, items=[(tree, handles, 0, "cols")]), ("items[0].cols is null", "n_cols = 3")),
            ("a null handle", dict(pos=pos, items=[(tree, [a, None, c], 0)]), ("items[0].cols[1] is null",)),
            ("more than 64 items", dict(pos=pos, items=[(tree, handles, 0)] * 65), ("n_items is 65", "64")),
            ("a tree larger than the domain", dict(pos=small, items=[(tree, handles, 0)]), ("items[0].tree", "log size 7", "log_domain 5")),
            ("a column too few", dict(pos=pos, items=[(sec.t.tree, sec.t.handles, 0), (tree, [a, b], 0)]),
             ("items[1].cols", "log size 4", "committed from 1")),
            ("a column too many", dict(pos=pos, items=[(tree, [a, b, other, c], 0)]), ("items[0].cols", "log size 7")),
            ("a column larger than the tree", dict(pos=pos, items=[(tree, [a, b, c, big], 0)]), ("items[0].cols[3]", "log size 8")),
            ("pairs on a tree of 3 + 2 + 1 columns", dict(pos=pos, items=[(tree, handles, PAIRS)]),
             ("items[0].flags", "LMN_OPEN_FRI_PAIRS", "exactly 4")),
            ("pairs on columns of log size 0", dict(pos=pos, items=[(low.t.tree, low.t.handles, PAIRS)]),
             ("items[0].flags", "LMN_OPEN_FRI_PAIRS")),
            ("an unknown flag", dict(pos=pos, items=[(tree, handles, 2)]), ("items[0].flags", "unknown")),
            ("an opening above 12 MiB", dict(pos=full, items=[(tree, handles, 0), (wide_tree, [wide], 0)]),
             ("items", "upper bound", "items[1]", "1024 positions", "12582912")),
        ]
        for name, kw, words in cases:
            before = [ctx.counter(k) for k in counters]
            rc, text, outs = _raw_open(ctx, kw["pos"], kw["items"], null=kw.get("null", ()))
            assert rc == INV, (name, rc, text)
            assert "open_queries" in text and all(w in text for w in words), (name, text)
            if "out" not in kw.get("null", ()):
                assert all(o == ZERO for o in outs), (name, outs)
            assert [ctx.counter(k) for k in counters] == before, name      # nothing was launched
            good_call(("after", name))
        assert L.lmn_open_queries(None, pos.handle, None, 0, None) == INV
        # zero positions, zero items: LMN_OK and empty outputs
        none = ctx.positions_from_cpu([], D)
        rc, _, outs = _raw_open(ctx, none, [(tree, handles, 0), (sec.t.tree, sec.t.handles, PAIRS)])
        assert rc == backend.LMN_OK and outs == [ZERO, ZERO]
        none.free()
        rc, _, _ = _raw_open(ctx, pos, [], null=("items", "out"))
        assert rc == backend.LMN_OK
        # positions_from_cpu
        for name, positions, log_domain, words in (
                ("1025 positions", list(range(1025)), 12, ("n is 1025", "1024")),
                ("unsorted", [5, 40, 7], 9, ("positions", "ascending", "index 2", "40 then 7")),
                ("repeated", [5, 5], 9, ("positions", "ascending", "index 1")),
                ("out of range", [5, 512], 9, ("positions[1] = 512", "out of range", "log_domain 9")),
                ("log_domain 32", [5], 32, ("log_domain is 32", "31"))):
            arr = np.array(positions, dtype=np.uint32)
            out = C.c_void_p(1)
            assert L.lmn_positions_from_cpu(ctx.handle, arr.ctypes.data, len(arr), log_domain, C.byref(out)) == INV, name
            text = L.lmn_last_error(ctx.handle).decode()
            assert "positions_from_cpu" in text and all(w in text for w in words), (name, text)
            assert out.value is None, name
            good_call(("after", name))
        out = C.c_void_p(1)
        assert L.lmn_positions_from_cpu(ctx.handle, None, 3, 9, C.byref(out)) == INV and out.value is None
        assert "positions is null with n = 3" in L.lmn_last_error(ctx.handle).decode()
        assert L.lmn_positions_from_cpu(ctx.handle, None, 0, 9, None) == INV
        assert "out is null" in L.lmn_last_error(ctx.handle).decode()
        n = C.c_uint32(7)
        buf = np.zeros(1024, np.uint32)
        assert L.lmn_positions_to_cpu(ctx.handle, None, buf.ctypes.data, C.byref(n)) == INV and n.value == 0
        assert L.lmn_positions_to_cpu(ctx.handle, pos.handle, None, C.byref(n)) == INV
        assert "host is null" in L.lmn_last_error(ctx.handle).decode()
        assert L.lmn_positions_log_domain(None) == 0
        L.lmn_positions_free(ctx.handle, None)
        # exactly 1024 positions and log_domain 31 are accepted
        edge = ctx.positions_from_cpu([(1 << 31) - 1 - 3 * k for k in range(1023, -1, -1)], 31)
        assert edge.log_domain == 31 and len(edge.to_cpu()) == 1024
        got = ctx.open_queries(edge, [(tree, handles)])[0]
        assert_opening(got, s.ref.decommit(groups_of(s, edge.to_cpu(), 31)), "log_domain 31")
        edge.free()
        assert pos.to_cpu() == good
        good_call("at the end")
    finally:
        for h in (pos, small, full, wide_tree, other, big, wide):
            h.free()


def check_sharded_context_refused(lib):
    ctx = dc.ctx_for(lib)
    s = shape_for(lib, 0)
    pos = ctx.positions_from_cpu([1, 2], 6)
    ctx.set_shard(0, 1, lambda *a: None)
    try:
        rc, text, outs = _raw_open(ctx, pos, [(s.t.tree, s.t.handles, 0)])
        assert rc == INV and "sharded" in text and "open_queries" in text and outs == [ZERO], (rc, text)
    finally:
        ctx.clear_shard()
    try:
        got = ctx.open_queries(pos, [s.item()])[0]
        assert_opening(got, s.ref.decommit({6: [1, 2]}), "after the shard is cleared")
    finally:
        pos.free()


def check_keep_refusals(ctxs):
    """lmn_col_fri_close_keep refuses what lmn_col_fri_close refuses, and leaves no handle behind"""
    ctx = ctxs.get(log_last_layer=1, log_blowup=1)
    L = ctx.lib.lib
    values, coeffs = fc.layer("random", 1, 1)
    good = ctx.col_from_cpu(np.ascontiguousarray(values.T))
    three = ctx.col_from_cpu(np.zeros((3, 4), np.uint32))
    dig = (C.c_uint8 * 32)(*fc.digest_of(1))
    try:
        for args, word in (((ctx.handle, three.handle, dig, 12), "last_layer"), ((ctx.handle, good.handle, dig, 32), "log_query_domain"),
                           ((ctx.handle, None, dig, 12), "last_layer"), ((ctx.handle, good.handle, None, 12), "start_digest")):
            res = backend.LmnFriCloseResult()
            res.n_coeffs = 5
            out = C.c_void_p(1)
            assert L.lmn_col_fri_close_keep(*args, C.byref(res), C.byref(out)) == INV, word
            assert word in L.lmn_last_error(ctx.handle).decode(), word
            assert res.n_coeffs == 0 and not res.positions and out.value is None, word
        res = backend.LmnFriCloseResult()
        assert L.lmn_col_fri_close_keep(ctx.handle, good.handle, dig, 12, C.byref(res), None) == INV
        assert "positions_out" in L.lmn_last_error(ctx.handle).decode()
        _keep_and_compare(ctxs.lib, ctx, values, fc.digest_of(1), 12, "after the refusals")
    finally:
        good.free()
        three.free()


def check_batch_library(batch_so):
    """the lock-step library on a thread outside any batch: lmn_open_queries and lmn_col_fri_close_keep work"""
    lib = backend.Library(batch_so)
    ctxs = fc.Contexts(lib)
    try:
        check_opening(lib, SHAPES.index(next(x for x in SHAPES if x[0] == "a secure column alone")), 2)
        check_keep_draws(ctxs, 70, False)
    finally:
        ctxs.close()


# ------------------------------------------------------------------------------------------------ E: whole proofs
BOTH = dict(LMN_DEVICE_FRI_CLOSE=1, LMN_DEVICE_DECOMMIT=1)
C_CLOSE, C_OPEN, C_OPEN_FALLBACK = backend.COUNTER_DEVICE_CLOSES, backend.COUNTER_DEVICE_OPENINGS, backend.COUNTER_DEVICE_OPENING_FALLBACKS
C_CLOSE_FALLBACK = backend.COUNTER_DEVICE_CLOSE_FALLBACKS


def prove_under(lib, cfg, tables, env, luts=None, prepared=None):
    """-> (proof bytes, {counter: its value}) of one proof on a context of its own, created and run under `env`"""
    with fc.Env(**env):
        ctx = backend.Context(0, cfg, lib)
        try:
            proof = ctx.prove_tables(tables, luts, prepared) if prepared is not None or luts is not None else ctx.prove_tables(tables)
            return proof, {c: ctx.counter(c) for c in (C_CLOSE, C_CLOSE_FALLBACK, C_OPEN, C_OPEN_FALLBACK)}
        finally:
            ctx.close()


def check_proof_case(lib, case):
    """every case of fri_close_checks.PROOF_CASES under both switches: the default path's bytes, accepted, counted"""
    cfg, tables = fc.proof_config(lib, case), fc.tables_of(case)
    dev, dc = prove_under(lib, cfg, tables, BOTH)
    host, hc = prove_under(lib, cfg, tables, {})
    assert dev == host, case.name
    lib.verify(dev, case.variant, cfg)
    assert hc[C_OPEN] == 0 and hc[C_OPEN_FALLBACK] == 0 and hc[C_CLOSE] == 0, hc
    assert dc[C_CLOSE] == 1 and dc[C_OPEN] == 1, dc
    assert dc[C_OPEN_FALLBACK] == dc[C_CLOSE_FALLBACK], dc           # the plan falls back exactly when the close does
    if dc[C_CLOSE_FALLBACK] == 0:
        assert dc[C_OPEN_FALLBACK] == 0, dc


def check_fallback_seeds(lib):
    """both FALLBACK_SEEDS under 2^11-nonce windows: (11, 12) == (1, 0) and (1, 1), both byte-equal to the default path"""
    case = fc.ProofCase("fallback", fc.KAT, 16, 0, 1, 3)
    cfg = fc.proof_config(lib, case)
    seen = []
    for seed in fc.FALLBACK_SEEDS:
        tables = fc.tables_of(case, seed)
        dev, dc = prove_under(lib, cfg, tables, dict(BOTH, LMN_POW_WINDOW_LOG=fc.WINDOW_LOG))
        host, _ = prove_under(lib, cfg, tables, dict(LMN_POW_WINDOW_LOG=fc.WINDOW_LOG))
        assert dev == host, seed
        lib.verify(dev, case.variant, cfg)
        seen.append((dc[C_OPEN], dc[C_OPEN_FALLBACK]))
    assert seen == [(1, 0), (1, 1)], seen


MIXED = {"2^13 + 2^11": lambda: [(0, syn.chain_graph(5000, 4)[0][1]), (1, syn.chain_graph(2000, 5)[1][1])],
         "2^13 + 2^12": lambda: [(0, syn.chain_graph(5000, 4)[0][1]), (1, syn.chain_graph(3000, 5)[1][1])]}


def check_recompute_jobs(lib, name, capfd=None):
    """trees stored without their register levels (LMN_MERKLE_SUB=3), then with the leaf level hashed from above as well
    (LMN_MERKLE_BELOW_MIN_LOG=12): the recompute jobs come from the device planner; the same bytes as the same switches
    without LMN_DEVICE_DECOMMIT and as whole-tree storage.  capfd (pytest's): one more proof under LMN_HOST_PROFILE=1, whose
    mark says how many tree nodes k_open_recompute produced - more than none, or the case would prove nothing about it"""
    cfg = lib.default_config()
    cfg.pow_bits = 12
    tables = [(k, r, len(r)) for k, r in MIXED[name]()]
    full, _ = prove_under(lib, cfg, tables, dict(LMN_DEVICE_FRI_CLOSE=1, LMN_MERKLE_FULL=1))
    for merkle in (dict(LMN_MERKLE_SUB=3), dict(LMN_MERKLE_SUB=3, LMN_MERKLE_BELOW_MIN_LOG=12)):
        dev, dc = prove_under(lib, cfg, tables, dict(BOTH, **merkle))
        close_only, cc = prove_under(lib, cfg, tables, dict(LMN_DEVICE_FRI_CLOSE=1, **merkle))
        assert dev == close_only and dev == full, (name, merkle)
        assert dc[C_OPEN] == 1 and cc[C_OPEN] == 0 and dc[C_OPEN_FALLBACK] == dc[C_CLOSE_FALLBACK], (dc, cc)
        if capfd is not None and dc[C_OPEN_FALLBACK] == 0:
            import re
            capfd.readouterr()
            again, _ = prove_under(lib, cfg, tables, dict(BOTH, LMN_HOST_PROFILE=1, **merkle))
            m = re.search(r"device plan, (\d+) entries fetched, (\d+) tree nodes recomputed", capfd.readouterr().err)
            assert again == full and m and int(m.group(1)) > 0 and int(m.group(2)) > 0, (name, merkle, m and m.groups())
    # (tables of two different graphs: the logup sums do not balance, so there is no verifier's verdict to ask for)


def check_prepared_sin(lib):
    """a Sin circuit through prepared settings: tree 0 is read through the prepared slab"""
    import prepared_checks as pc
    cfg = pc.config(lib, pow_bits=12)
    tabs, luts = syn.activation_graph(30, 4, names=("sin",), ranges={"sin": (-300, 200)})
    pie = [(k, r, len(r)) for k, r in tabs]
    with backend.PreparedSettings(0, cfg, luts, backend.LOOKUP_SIN, lib) as pp:
        want, hc = prove_under(lib, cfg, pie, {}, prepared=pp)
        got, dc = prove_under(lib, cfg, pie, BOTH, prepared=pp)
    assert got == want
    assert dc[C_OPEN] == 1 and hc[C_OPEN] == 0, (dc, hc)
    lib.verify(got, cfg.protocol_variant, cfg)


def check_inert_at_pow_bits_5(lib):
    cfg = lib.default_config()
    assert cfg.pow_bits == 5
    tables = [(k, r, len(r)) for k, r in syn.config2_add_only(64, 11)]
    want, _ = prove_under(lib, cfg, tables, {})
    got, dc = prove_under(lib, cfg, tables, BOTH)
    assert got == want and dc[C_CLOSE] == 0 and dc[C_OPEN] == 0 and dc[C_OPEN_FALLBACK] == 0, dc


def check_batch_library_proof(batch_so):
    """the lock-step library outside any batch: a proof under both switches plans on the host"""
    lib = backend.Library(batch_so)
    case = fc.ProofCase("batch", fc.KAT, 12, 0, 1, 3)
    cfg, tables = fc.proof_config(lib, case), fc.tables_of(case)
    want, _ = prove_under(lib, cfg, tables, {})
    got, dc = prove_under(lib, cfg, tables, BOTH)
    assert got == want and dc[C_OPEN] == 0, dc


def check_error_precedence(lib):
    """as fri_close_checks.check_error_precedence, with both switches"""
    case = fc.ProofCase("errors", fc.KAT, 12, 0, 1, 3)
    bad_word = syn.config2_add_only(64, 9)[0][1].copy()
    bad_word[5, 9] = 0x7fffffff
    bad_constraint = syn.config2_add_only(64, 9)[0][1].copy()
    bad_constraint[3, 11] ^= 1
    for rows, code in ((bad_word, backend.ERR_INVALID_ARGUMENT), (bad_constraint, backend.ERR_CONSTRAINTS)):
        got = []
        for env in (BOTH, {}):
            try:
                prove_under(lib, fc.proof_config(lib, case), [(0, rows, len(rows))], env)
            except backend.LuminairBackendError as e:
                got.append(e.code)
            else:
                got.append(0)
        assert got == [code, code], got


def check_2_16_rows(lib):
    """GPU only: a 2^16-row Add proof, pow_bits 16, 70 queries, default Merkle switches"""
    case = fc.ProofCase("2^16 rows", fc.KAT, 16, 0, 1, 70)
    cfg = fc.proof_config(lib, case)
    tables = [(k, r, len(r)) for k, r in syn.config2_add_only(1 << 16, 5)]
    dev, dc = prove_under(lib, cfg, tables, BOTH)
    host, _ = prove_under(lib, cfg, tables, {})
    assert dev == host
    lib.verify(dev, case.variant, cfg)
    assert dc[C_OPEN] == 1 and dc[C_OPEN_FALLBACK] == dc[C_CLOSE_FALLBACK], dc
