"""Checks of decommitment on device handles (`lmn_tree_decommit`, `lmn_col_gather`; luminair_amd.backend.Tree.decommit,
Col.gather), shared by the emulation suite (tests/test_level2_decommit_emu.py, in process) and the GPU suite
(tests/test_gpu_level2_decommit.py, one child process per check: `python tests/level2_decommit_checks.py <library> <check>`).
The reference of every comparison is the oracle's restatement of stwo's `MerkleProver::decommit` / `MerkleVerifier::verify`
(oracle/merkle.py) on host copies of the same columns."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from luminair_amd import backend, synthetic as syn                                 # noqa: E402
from oracle.channel import ProtocolVariant                                          # noqa: E402
from oracle.merkle import MerkleTree, verify_decommitment                           # noqa: E402
from oracle.proof import to_bincode                                                 # noqa: E402
from oracle.prover import fold_positions, prove as oracle_prove                     # noqa: E402

from level2_prover import Level2Kernels, _q, _whole_handles                         # noqa: E402

P = (1 << 31) - 1
INV = backend.ERR_INVALID_ARGUMENT

_ctx_cache = {}


def ctx_for(lib):
    if id(lib) not in _ctx_cache:
        _ctx_cache[id(lib)] = backend.Context(0, None, lib)
    return _ctx_cache[id(lib)]


class Committed:
    """a device tree, the handles it was committed from, and host copies of the columns in the same order"""

    def __init__(self, ctx, shape, seed):
        rng = np.random.default_rng(seed)
        self.host = [rng.integers(0, P, size=(ncols, 1 << log), dtype=np.uint64).astype(np.uint32) for ncols, log in shape]
        self.handles = [ctx.col_from_cpu(a) for a in self.host]
        self.tree = ctx.commit(self.handles)
        self.columns = [c for a in self.host for c in a]
        self.log_sizes = [log for ncols, log in shape for _ in range(ncols)]
        self.max_log = max(self.log_sizes)

    def free(self):
        self.tree.free()
        for h in self.handles:
            h.free()


# (name, [(ncols, log_size) per handle, in commit order])
SHAPES = [
    ("one size", [(3, 6)]),
    ("three sizes, layer 6 without columns, small handle first", [(3, 5), (2, 7), (1, 4)]),
    ("handles of one size with different ncols", [(1, 6), (4, 6), (2, 6), (3, 4)]),
    ("a secure column alone", [(4, 8)]),
    ("log size 0", [(2, 0)]),
    ("log size 1", [(1, 1)]),
    ("log sizes 1 and 0", [(1, 0), (2, 1)]),
    ("log sizes 5, 3 and 0", [(1, 3), (2, 5), (1, 0)]),
    ("a root layer without columns of its own", [(2, 3), (1, 2)]),
]


def query_sets(t, n_queries, seed):
    """(name, {log_size: sorted positions}) for the tree `t`"""
    top, sizes = t.max_log, sorted(set(t.log_sizes), reverse=True)
    last = (1 << top) - 1
    qs = [("no groups", {}), ("an empty group", {top: []}), ("single position", {top: [last // 3]}),
          ("position 0 and the last", {top: sorted({0, last})}),
          ("only the smallest size", {sizes[-1]: [((1 << sizes[-1]) - 1) // 2]}),
          ("every leaf", {ls: list(range(1 << ls)) for ls in sizes})]
    if top >= 1:
        k = (last // 2) & ~1
        qs.append(("both children of one node", {top: [k, k + 1]}))
    if top >= 2:
        qs.append(("neighbours that are no siblings", {top: [1, 2]}))
    absent = [lg for lg in range(top, -1, -1) if lg not in sizes]
    if absent:
        qs.append(("a log size without columns", {absent[0]: [(1 << absent[0]) - 1], top: [1]}))
    rng = np.random.default_rng(seed)
    drawn = sorted({int(x) for x in rng.integers(0, 1 << top, size=n_queries)})
    qs.append(("n_queries seeded positions, folded", {ls: fold_positions(drawn, top - ls) for ls in sizes}))
    return qs


def assert_opening_equals_oracle(t, ref, queries, what):
    vals, hw, cw = t.tree.decommit(t.handles, queries)
    want_v, want_h, want_c = ref.decommit(queries)
    assert vals.dtype == np.uint32 and cw.dtype == np.uint32
    assert vals.tolist() == want_v, what
    assert hw == want_h, what
    assert cw.tolist() == want_c, what
    # (the verifier's walk ends at the root only if it starts somewhere: with no position at all it rejects the oracle's own
    # - empty - opening as well, so there is nothing to verify then)
    if any(len(q) for q in queries.values()):
        assert verify_decommitment(t.tree.root(), t.log_sizes, queries, vals.tolist(), hw, cw.tolist()), what
        if hw:      # (every leaf opened: no hash to take away) - one hash short, the walk runs out of witness
            assert not verify_decommitment(t.tree.root(), t.log_sizes, queries, vals.tolist(), hw[:-1], cw.tolist()), what
    return vals, hw, cw


# ------------------------------------------------------------------------------------------------ the checks
def check_oracle(lib):
    """item 1: all three outputs equal the oracle's, and its verifier accepts them under the device tree's root"""
    ctx = ctx_for(lib)
    for si, (name, shape) in enumerate(SHAPES):
        t = Committed(ctx, shape, 100 + si)
        try:
            ref = MerkleTree(t.columns)
            assert t.tree.root() == ref.root(), name
            for qname, queries in query_sets(t, ctx.config.n_queries, 200 + si):
                vals, hw, cw = assert_opening_equals_oracle(t, ref, queries, (name, qname))
                if qname == "every leaf":
                    assert hw == [] and len(cw) == 0 and len(vals) == sum(1 << lg for lg in t.log_sizes)
                if qname in ("no groups", "an empty group"):
                    assert len(vals) == 0 and hw == [] and len(cw) == 0
        finally:
            t.free()
    # views: the same columns handed over as views of one wider handle
    rng = np.random.default_rng(7)
    host = rng.integers(0, P, size=(6, 64), dtype=np.uint64).astype(np.uint32)
    whole = ctx.col_from_cpu(host)
    a, b = whole.view(0, 2), whole.view(2, 4)
    tree = ctx.commit([a, b])
    ref = MerkleTree(list(host))
    q = {6: [3, 17, 18, 63]}
    vals, hw, cw = tree.decommit([a, b], q)
    assert (vals.tolist(), hw, cw.tolist()) == ref.decommit(q)
    vals2, hw2, cw2 = tree.decommit([whole], q)            # 6 columns of the same size in the same order
    assert (vals2.tolist(), hw2, cw2.tolist()) == ref.decommit(q)
    for h in (a, b):
        h.free()
    tree.free()
    whole.free()


def check_gather(lib):
    """item 2: Col.gather equals numpy indexing of the uploaded array"""
    ctx = ctx_for(lib)
    rng = np.random.default_rng(11)
    for ncols, log in ((1, 5), (4, 7), (15, 6), (4, 0)):
        host = rng.integers(0, P, size=(ncols, 1 << log), dtype=np.uint64).astype(np.uint32)
        h = ctx.col_from_cpu(host)
        n = 1 << log
        for pos in ([n - 1, 0, n // 2, 0, 0, n - 1], [], [n - 1], list(range(n)), list(range(n - 1, -1, -1)),
                    [int(x) for x in rng.integers(0, n, size=300)]):
            got = h.gather(pos)
            assert got.shape == (ncols, len(pos)) and got.dtype == np.uint32
            assert np.array_equal(got, host[:, pos] if pos else np.zeros((ncols, 0), np.uint32)), (ncols, log, pos[:8])
        if ncols >= 4 and n >= 2:
            v = h.view(1, 2)
            pos = [n - 1, 1, 1, 0]
            assert np.array_equal(v.gather(pos), host[1:3, pos])
            v.free()
        # n = 0 writes nothing, whatever the pointers
        assert ctx.lib.lib.lmn_col_gather(ctx.handle, h.handle, None, 0, None) == backend.LMN_OK
        h.free()


def _raw_decommit(ctx, tree, handles, logs, counts, flat, n_cols=None, n_groups=None, null=()):
    """the C call itself -> (rc, error text, the six outputs)"""
    L = ctx.lib.lib
    arr = (C.c_void_p * max(len(handles), 1))(*[getattr(h, "handle", h) for h in handles])
    lg, ct, fl = (np.array(x, dtype=np.uint32) for x in (logs, counts, flat))
    vals, hashes, wit = C.c_void_p(1), C.c_void_p(1), C.c_void_p(1)
    nv, nh, nw = C.c_size_t(9), C.c_size_t(9), C.c_size_t(9)
    rc = L.lmn_tree_decommit(ctx.handle, getattr(tree, "handle", tree), None if "cols" in null else arr,
                             len(handles) if n_cols is None else n_cols,
                             None if "query_logs" in null else lg.ctypes.data,
                             None if "query_counts" in null else ct.ctypes.data,
                             len(logs) if n_groups is None else n_groups, None if "queries" in null else fl.ctypes.data,
                             C.byref(vals), C.byref(nv), C.byref(hashes), C.byref(nh), C.byref(wit), C.byref(nw))
    text = L.lmn_last_error(ctx.handle).decode()
    outs = (vals.value, nv.value, hashes.value, nh.value, wit.value, nw.value)
    if rc == backend.LMN_OK:
        for p in (vals, hashes, wit):
            if p.value:
                L.lmn_free(p)
    return rc, text, outs


def check_refusals(lib):
    """item 3: every refusal names the offending argument, leaves all six outputs null / 0, and the same context and
    tree go on to a successful call"""
    ctx = ctx_for(lib)
    t = Committed(ctx, [(2, 6), (3, 4)], 31)
    ref = MerkleTree(t.columns)
    good = {6: [5, 40], 4: [1, 10]}
    other = ctx.col_from_cpu(np.zeros((1, 64), np.uint32))
    big = ctx.col_from_cpu(np.zeros((1, 128), np.uint32))
    a, b = t.handles
    cases = [
        ("a column too few", dict(handles=[a], logs=[6], counts=[1], flat=[0]), ("cols", "log size 4")),
        ("a column too many", dict(handles=[a, other, b], logs=[6], counts=[1], flat=[0]), ("cols", "log size 6")),
        ("a column larger than the tree", dict(handles=[a, b, big], logs=[6], counts=[1], flat=[0]), ("cols[2]", "log size 7")),
        ("a null handle", dict(handles=[a, None], logs=[6], counts=[1], flat=[0]), ("cols[1]", "null")),
        ("unsorted positions", dict(handles=[a, b], logs=[6], counts=[3], flat=[5, 40, 7]), ("queries", "ascending", "index 2")),
        ("a repeated position", dict(handles=[a, b], logs=[6, 4], counts=[1, 2], flat=[5, 3, 3]), ("queries", "group 1", "ascending")),
        ("a position out of range", dict(handles=[a, b], logs=[6, 4], counts=[1, 1], flat=[5, 16]), ("queries", "position 16", "out of range")),
        ("a repeated log size", dict(handles=[a, b], logs=[6, 4, 6], counts=[1, 1, 1], flat=[5, 3, 6]), ("query_logs[2]", "repeats")),
        ("a log size above the tree's", dict(handles=[a, b], logs=[7], counts=[1], flat=[5]), ("query_logs[0]", "exceeds")),
        ("null cols", dict(handles=[a, b], logs=[6], counts=[1], flat=[0], null=("cols",)), ("cols is null",)),
        ("null query_logs", dict(handles=[a, b], logs=[6], counts=[1], flat=[0], null=("query_logs",)), ("query_logs is null",)),
        ("null query_counts", dict(handles=[a, b], logs=[6], counts=[1], flat=[0], null=("query_counts",)), ("query_counts is null",)),
        ("null queries", dict(handles=[a, b], logs=[6], counts=[1], flat=[0], null=("queries",)), ("queries is null",)),
    ]
    for name, kw, words in cases:
        rc, text, outs = _raw_decommit(ctx, t.tree, **kw)
        assert rc == INV, (name, rc)
        assert all(w in text for w in words), (name, text)
        assert outs == (None, 0, None, 0, None, 0), (name, outs)
        assert_opening_equals_oracle(t, ref, good, ("after", name))
    # through the wrapper: the same refusal as an exception that carries the text
    try:
        t.tree.decommit(t.handles, {6: [9, 9]})
        raise AssertionError("a repeated position was accepted")
    except backend.LuminairBackendError as e:
        assert e.code == INV and "ascending" in str(e)
    # null context / tree / output pointers
    L = ctx.lib.lib
    assert _raw_decommit(ctx, None, [a, b], [6], [1], [0])[0] == INV
    z = C.c_size_t()
    p = C.c_void_p()
    arr = (C.c_void_p * 2)(a.handle, b.handle)
    assert L.lmn_tree_decommit(None, t.tree.handle, arr, 2, None, None, 0, None, C.byref(p), C.byref(z), C.byref(p), C.byref(z),
                               C.byref(p), C.byref(z)) == INV
    assert L.lmn_tree_decommit(ctx.handle, t.tree.handle, arr, 2, None, None, 0, None, None, C.byref(z), C.byref(p), C.byref(z),
                               C.byref(p), C.byref(z)) == INV
    assert "output" in L.lmn_last_error(ctx.handle).decode()
    # zero groups with null query arrays is legal
    rc, _, outs = _raw_decommit(ctx, t.tree, [a, b], [], [], [], null=("query_logs", "query_counts", "queries"))
    assert rc == backend.LMN_OK and outs == (None, 0, None, 0, None, 0)
    # gather
    pos = np.array([1, 64, 2], dtype=np.uint32)
    out = np.full((2, 3), 0xAAAAAAAA, dtype=np.uint32)
    assert L.lmn_col_gather(ctx.handle, a.handle, pos.ctypes.data, 3, out.ctypes.data) == INV
    text = L.lmn_last_error(ctx.handle).decode()
    assert "positions[1]" in text and "64" in text and "out of range" in text, text
    assert (out == 0xAAAAAAAA).all()                                   # refused before anything was launched
    assert L.lmn_col_gather(ctx.handle, a.handle, None, 3, out.ctypes.data) == INV
    assert "positions is null" in L.lmn_last_error(ctx.handle).decode()
    assert L.lmn_col_gather(ctx.handle, a.handle, pos.ctypes.data, 3, None) == INV
    assert "host_out is null" in L.lmn_last_error(ctx.handle).decode()
    assert L.lmn_col_gather(ctx.handle, None, pos.ctypes.data, 3, out.ctypes.data) == INV
    assert L.lmn_col_gather(None, a.handle, pos.ctypes.data, 3, out.ctypes.data) == INV
    assert np.array_equal(a.gather([63, 0]), t.host[0][:, [63, 0]])
    assert_opening_equals_oracle(t, ref, good, "after the gather refusals")
    other.free()
    big.free()
    t.free()


# ---- item 4: a whole proof whose trees keep only handles
class HandleMerkle:
    """what `oracle.prover.prove` needs of a tree - root() and decommit() - on an `lmn_tree` and the handles it was
    committed from: no host copy of a column or of a layer exists"""

    def __init__(self, ctx, handles):
        self.handles = list(handles)
        self.tree = ctx.commit(self.handles)

    def root(self):
        return self.tree.root()

    def decommit(self, queries_per_log_size):
        vals, hw, cw = self.tree.decommit(self.handles, queries_per_log_size)
        return [int(v) for v in vals], hw, [int(v) for v in cw]


class HandleOnlyKernels(Level2Kernels):
    name = "level-2 C ABI on device handles, trees opened on the device"

    def __init__(self, ctx):
        super().__init__(ctx)
        self.sent_whole = []      # handles read through to_cpu: the FRI last layer, which the proof carries whole

    def merkle(self, cols):
        if not cols:
            return MerkleTree([])
        self._count("commit")
        return HandleMerkle(self.ctx, _whole_handles(cols))

    def secure_merkle(self, cols):
        self._count("commit")
        for c in cols:
            c.committed = True
        return HandleMerkle(self.ctx, [c.h for c in cols])

    def secure_at(self, col, pos):
        if getattr(col, "committed", False):            # a committed layer: only the witness value travels
            self._count("gather")
            return _q(col.h.gather([pos])[:, 0])
        if col._host is None:                           # never committed: the last layer, interpolated on the host
            self.sent_whole.append(col.h)
        return _q(col.host()[:, pos])


def prove_with_handles_only(ctx, tables, variant=None, luts=None):
    """-> (proof bytes, the kernel set); Tree.layer and Col.to_cpu are wrapped while the proof runs"""
    K = HandleOnlyKernels(ctx)
    seen = {"layer": 0, "to_cpu": []}
    orig_layer, orig_to_cpu = backend.Tree.layer, backend.Col.to_cpu

    def layer(self, layer_log):
        seen["layer"] += 1
        return orig_layer(self, layer_log)

    def to_cpu(self):
        seen["to_cpu"].append(self)
        return orig_to_cpu(self)
    backend.Tree.layer, backend.Col.to_cpu = layer, to_cpu
    try:
        proof = oracle_prove([(k, np.asarray(r).astype(np.uint64)) for k, r in tables],
                             variant=variant if variant is not None else ProtocolVariant.KAT, kernels=K, luts=luts)
    finally:
        backend.Tree.layer, backend.Col.to_cpu = orig_layer, orig_to_cpu
    assert seen["layer"] == 0, "a tree layer was downloaded"
    assert len(seen["to_cpu"]) == 1 and seen["to_cpu"] == K.sent_whole, "a column other than the FRI last layer was downloaded"
    assert seen["to_cpu"][0].ncols == 4
    assert K.calls["gather"] >= 1
    return to_bincode(proof), K


def check_whole_proof(lib):
    ctx = ctx_for(lib)
    kat = open(os.path.join(ROOT, "tests", "golden", "kat_simple", "proof"), "rb").read()
    got, _ = prove_with_handles_only(ctx, syn.simple_example())
    assert len(kat) == 4876 and got == kat
    mixed = [(0, syn.chain_graph(64, 4)[0][1]), (1, syn.chain_graph(500, 5)[1][1])]
    want = to_bincode(oracle_prove([(k, r.astype(np.uint64)) for k, r in mixed], variant=ProtocolVariant.KAT))
    assert prove_with_handles_only(ctx, mixed)[0] == want
    tabs, luts = syn.activation_graph(30, 4, names=("sin",), ranges={"sin": (-300, 200)})
    want = to_bincode(oracle_prove([(k, r.astype(np.uint64)) for k, r in tabs], variant=ProtocolVariant.PINNED, luts=luts))
    assert prove_with_handles_only(ctx, tabs, ProtocolVariant.PINNED, luts)[0] == want


# ---- GPU only
FULL_SHAPE = [(15, 21), (4, 20)]      # BASELINE config 2a's trace tree (15 columns, 2^21-row LDE) with a second size in it


def seeded_queries(n_queries, top, sizes, seed):
    rng = np.random.default_rng(seed)
    drawn = sorted({int(x) for x in rng.integers(0, 1 << top, size=n_queries)})
    return {ls: fold_positions(drawn, top - ls) for ls in sizes}


def check_full_size(lib):
    """item 5: the oracle tree is too slow to build at this size; the queried values are checked against the uploaded
    columns, and the oracle's verifier - which accepts exactly one witness for given values - against Tree.root()"""
    ctx = ctx_for(lib)
    t = Committed(ctx, FULL_SHAPE, 51)
    try:
        queries = seeded_queries(ctx.config.n_queries, 21, [21, 20], 52)
        vals, hw, cw = t.tree.decommit(t.handles, queries)
        want = [int(t.host[0][c, p]) for p in queries[21] for c in range(15)] + \
               [int(t.host[1][c, p]) for p in queries[20] for c in range(4)]
        assert vals.tolist() == want
        assert verify_decommitment(t.tree.root(), t.log_sizes, queries, vals.tolist(), hw, cw.tolist())
    finally:
        t.free()


def check_big_gather(lib):
    ctx = ctx_for(lib)
    rng = np.random.default_rng(61)
    host = rng.integers(0, P, size=(4, 1 << 22), dtype=np.uint64).astype(np.uint32)
    h = ctx.col_from_cpu(host)
    pos = rng.integers(0, 1 << 22, size=1000)
    pos[0], pos[1] = 0, (1 << 22) - 1
    assert np.array_equal(h.gather(pos), host[:, pos])
    h.free()


GPU_CHECKS = {"oracle": check_oracle, "gather": check_gather, "refusals": check_refusals, "whole_proof": check_whole_proof,
              "full_size": check_full_size, "big_gather": check_big_gather}

if __name__ == "__main__":
    GPU_CHECKS[sys.argv[2]](backend.Library(sys.argv[1]))
    print("ok", sys.argv[2])
