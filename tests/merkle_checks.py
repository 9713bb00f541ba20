"""Every layer and every launch form of the standalone Blake2s Merkle commit (`lmn_op_merkle_root`, `lmn_col_commit`,
`lmn_tree_layer_to_cpu`): kernels_merkle.hip behind the level planner of commit.cpp `build_merkle_levels`.  Run against the
emulation build on CPU (tests/test_merkle_edges_emu.py) and the HIP library on GPU (tests/test_gpu_merkle_edges.py).

Reference.  A node is H(left || right || this layer's column words, u32 LE, columns in size-sorted stable order), H =
Blake2s-256; the tallest columns are the leaves, the empty tree is H("").  Up to 2^10 leaves every node is computed here with
`hashlib.blake2s` from that rule, and `oracle.merkle.MerkleTree` must give the same layers (this pins the numpy oracle).
Above 2^10 leaves the reference is `MerkleTree` (numpy), and from 2^17 leaves the C oracle (`oracle.cbackend`, tied to numpy
by test_oracle_c.py).  For every tree above 2^10 leaves a fixed-seed sample of the DEVICE's own nodes is re-hashed with
hashlib from the device's children layer and the host columns as well (64 nodes per layer or the whole layer, always node
0, the last node and the nodes either side of the multiples of 64, 256 and 2048 around every drawn node), so that a slip in
the fast oracle cannot hide a matching slip in the kernel.

What a case asserts: `Context.merkle_root` and `Tree.root()` equal the reference root, `Tree.log_size` the tree's height,
EVERY layer 0..log_size equals the reference layer in full (the message names the layer, the first differing node and how
many differ), and a decommitment at positions {0, last, seeded} per column size equals `MerkleTree.decommit`
(level2_decommit_checks.assert_opening_equals_oracle).

Which kernel a case reaches.  `plan()` restates the planner on the handles' device addresses (`Col.device_ptr`: a handle is
one allocation, so its columns are one run; views alias it; `lmn_op_merkle_root` places column after column in the arena on
256-byte boundaries, so columns of 2^6 words or more form one run and shorter ones one run each).  The launch counters of
the commit (`merkle_launches`, `merkle_fused_launches`) must equal the plan's, and the forms a case names must be in it:
  layer                      k_merkle_layer (pointer table: more than MERKLE_MAX_SEG = 4 runs on a level)
  small<0|1|2>               k_merkle_small (start level <= 2^10): anything / a leaf level of one run of <= 16 columns /
                             children only
  fused<0>x1..4              k_merkle_fused<0> with that many runs (a leaf of more than 16 columns counts as x1)
  fused<1,4|8|12|15|16>      leaf level of one run, message words NZ..15 compile-time zeros
  fused<2>                   children only
  sub=0..3                   per-lane register subtree depth of a fused launch
Modes 3 and 4 of k_merkle_fused (the FRI fold inside the leaf launch, and the leaf level hashed by the launch of the level
above it) exist only inside the FRI commit loop and trees stored without their register levels: tests/fri_checks.py
compares them layer by layer through `lmn_col_fri_commit`, next to the proof parity tests.

Value classes (numeric_checks.words): all 0, all P-1, alternating 0 / P-1, EDGE_WORDS, uniform random - on the leaf-count
axis at the fused size; random elsewhere.  Axes: leaf column count (LEAF_COUNTS, thresholds of NZ and of the 16-word
blocks), children plus own columns (OWN_COUNTS), runs (RUN_VARIANTS), tree height (every log from 0), mixed-size trees
chosen against the planner (mixed_shapes, check_fused_run_end), LMN_MERKLE_SUB."""
import hashlib
import types

import numpy as np

import numeric_checks as nc
from numeric_checks import P, U64, words

U32 = np.uint32
LEAF_COUNTS = (1, 3, 4, 5, 7, 8, 9, 12, 13, 15, 16, 17, 18, 31, 32, 33, 48, 49)
OWN_COUNTS = (1, 2, 15, 16, 17, 32)
VALUE_CLASSES = ("zero", "pm1", "alt", "edge", "random")
PY_MAX_LOG = 10       # hashlib for every node up to 2^10 leaves
C_MIN_LOG = 17        # the C oracle from 2^17 leaves
MERKLE_MAX_SEG, MERKLE_MAX_SUB, MERKLE_MAX_FUSED = 4, 3, 11      # kernels.h


# ----------------------------------------------------------------------------- reference
def tree_order(cols):
    return [cols[i] for i in sorted(range(len(cols)), key=lambda i: -len(cols[i]))]      # sorted() is stable


def _own(cols_sorted, log):
    own = [c for c in cols_sorted if len(c) == 1 << log]
    return np.stack(own, axis=1).astype("<u4") if own else None


def hashlib_layers(cols):
    """layers[k]: (2^k, 8) uint32, every node by hashlib"""
    cs = tree_order([np.asarray(c) for c in cols])
    if not cs:
        return [np.frombuffer(hashlib.blake2s(b"").digest(), dtype="<u4").reshape(1, 8).astype(U32)]
    max_log = len(cs[0]).bit_length() - 1
    layers, prev = [None] * (max_log + 1), None
    for lg in range(max_log, -1, -1):
        own = _own(cs, lg)
        out = np.empty((1 << lg, 8), dtype=U32)
        for i in range(1 << lg):
            msg = b"" if prev is None else prev[2 * i].astype("<u4").tobytes() + prev[2 * i + 1].astype("<u4").tobytes()
            if own is not None:
                msg += own[i].tobytes()
            out[i] = np.frombuffer(hashlib.blake2s(msg).digest(), dtype="<u4")
        layers[lg] = prev = out
    return layers


def same_layer(got, want, what):
    got, want = np.asarray(got, dtype=U32), np.asarray(want, dtype=U32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(axis=1))
        i = int(bad[0])
        raise AssertionError("%s: %d of %d nodes differ, first at node %d: got %s want %s" % (
            what, len(bad), len(got), i, got[i].astype("<u4").tobytes().hex(), want[i].astype("<u4").tobytes().hex()))


def ref_layers(cols):
    from oracle.merkle import MerkleTree
    cols = [np.ascontiguousarray(c, dtype=U32) for c in cols]
    max_log = max(len(c) for c in cols).bit_length() - 1 if cols else 0
    if max_log <= PY_MAX_LOG:
        layers = hashlib_layers(cols)
        numpy_layers = MerkleTree(cols).layers
        assert len(numpy_layers) == len(layers)
        for lg in range(len(layers)):
            same_layer(numpy_layers[lg], layers[lg], "numpy oracle MerkleTree, layer %d" % lg)
        return layers
    if max_log >= C_MIN_LOG:
        return nc._c_oracle().merkle(cols).layers
    return MerkleTree(cols).layers


def ref_tree(cols, layers):
    """a MerkleTree over `layers` (for decommit), without hashing them again"""
    from oracle.merkle import MerkleTree
    t = MerkleTree.__new__(MerkleTree)
    t.columns = [np.ascontiguousarray(c, dtype=U32) for c in cols]
    t.sorted_columns = tree_order(t.columns)
    t.layers = layers
    return t


def sample_nodes(size, rng):
    """>= 64 nodes of a layer (all of a smaller one): 0, the last, seeded ones, and the nodes either side of the
    multiples of 64, 256 and 2048 below and above every seeded one"""
    if size <= 64:
        return list(range(size))
    drawn = {int(v) for v in rng.integers(0, size, size=64)}
    idx = {0, size - 1} | drawn
    for i in drawn:
        for m in (64, 256, 2048):
            for k in (i - i % m, i - i % m + m):
                idx.update(j for j in (k - 1, k) if 0 <= j < size)
    extra = iter(range(size))
    while len(idx) < 64:
        idx.add(next(extra))
    return sorted(idx)


def rehash_device_sample(dev_layers, cols, seed, what):
    """the device's node i of layer l == hashlib of the DEVICE's nodes 2i, 2i + 1 of layer l + 1 and the host columns"""
    cs = tree_order([np.asarray(c) for c in cols])
    max_log = len(dev_layers) - 1
    rng = np.random.default_rng(seed)
    for lg in range(max_log, -1, -1):
        own = _own(cs, lg)
        for i in sample_nodes(1 << lg, rng):
            msg = b"" if lg == max_log else dev_layers[lg + 1][2 * i:2 * i + 2].astype("<u4").tobytes()
            if own is not None:
                msg += own[i].tobytes()
            want = hashlib.blake2s(msg).digest()
            got = dev_layers[lg][i].astype("<u4").tobytes()
            assert got == want, "%s: layer %d node %d is not the hash of its children and columns: got %s want %s" % (
                what, lg, i, got.hex(), want.hex())


# ----------------------------------------------------------------------------- the planner, restated
def col_addresses(handles):
    """[(byte address, log)] of every column, commit order"""
    return [(h.device_ptr + (j * 4 << h.log_size), h.log_size) for h in handles for j in range(h.ncols)]


def arena_addresses(logs):
    """lmn_op_merkle_root: column after column from Arena::alloc_bytes (256-byte boundaries)"""
    out, off = [], 0
    for lg in logs:
        off = (off + 255) & ~255
        out.append((off, lg))
        off += 4 << lg
    return out


def plan(addresses, sub_env=None):
    """build_merkle_levels outside prove (no cuts, no fold) -> [(form, level, nfused, sub)]"""
    max_log = max(lg for _, lg in addresses)
    per_level = [[a for a, lg in addresses if lg == lv] for lv in range(max_log + 1)]    # commit order within a size

    def make_segs(lv):
        runs = []
        for a in per_level[lv]:
            if runs and a == runs[-1][0] + runs[-1][1] * (4 << lv):
                runs[-1][1] += 1
            elif len(runs) < MERKLE_MAX_SEG:
                runs.append([a, 1])
            else:
                return None
        return runs

    out, prev, level = [], False, max_log
    while level >= 0:
        ncols = len(per_level[level])
        runs = make_segs(level)
        if runs is None:
            out.append(("layer", level, 0, 0))
            prev, level = True, level - 1
            continue
        plain = 0
        while level - plain - 1 >= 0 and not per_level[level - plain - 1]:
            plain += 1
        leaf_run = not prev and ncols <= 16 and len(runs) == 1
        if level <= 10:
            nfused, sub = min(plain, 10), 0
            form = "small<%d>" % (1 if leaf_run else 2 if ncols == 0 else 0)
        else:
            nfused = min(plain, MERKLE_MAX_FUSED, level - 10)
            sub = max(0, min(MERKLE_MAX_SUB, nfused, level - 17))
            if sub_env is not None:
                sub = min(sub_env, nfused, MERKLE_MAX_SUB)
            nfused = min(nfused, sub + 8)
            if leaf_run:
                form = "fused<1,%d>" % next(nz for nz in (4, 8, 12, 15, 16) if ncols <= nz)
            elif ncols == 0:
                form = "fused<2>"
            else:
                form = "fused<0>x%d" % len(runs)
        out.append((form, level, nfused, sub))
        prev, level = True, level - nfused - 1
    return out


def plan_forms(p):
    return {f for f, _, _, _ in p} | {"sub=%d" % s for f, _, _, s in p if f.startswith("fused")}


# ----------------------------------------------------------------------------- handles
def layer_words(tree, lg):
    out = np.empty((1 << lg, 8), dtype=U32)
    tree.ctx._check(tree.ctx.lib.lib.lmn_tree_layer_to_cpu(tree.ctx.handle, tree.handle, lg, out.ctypes.data))
    return out


class Handles:
    """the handles of one commit, in commit order, with the host columns in the same order; `keep`: allocations that
    views alias or that only hold an address"""

    def __init__(self):
        self.commit, self.cols, self.keep = [], [], []

    def add(self, h, host):
        self.commit.append(h)
        self.cols.extend(np.ascontiguousarray(c, dtype=U32) for c in host)
        return h

    def free(self):
        for h in self.commit + self.keep:
            h.free()


def separate_handle(ctx, H, host):
    """a handle of its own that does NOT start where the previous column of the commit ends (allocators may hand out
    neighbouring blocks: such a block is kept as a spacer and another one is taken)"""
    for _ in range(8):
        h = ctx.col_from_cpu(host)
        if H.commit:
            p = H.commit[-1]
            if h.log_size == p.log_size and h.device_ptr == p.device_ptr + (p.ncols * 4 << p.log_size):
                H.keep.append(h)
                continue
        return H.add(h, host)
    raise AssertionError("no allocation apart from the previous handle in 8 tries")


def _junk(rng, log):
    return rng.integers(1, P, size=(1, 1 << log), dtype=U64).astype(U32)


def _split(n, k):
    return [n // k + (1 if i < n % k else 0) for i in range(k)]


RUN_VARIANTS = ("one handle", "2 handles", "3 handles", "4 handles", "5 handles", "9 handles", "adjacent views",
                "views with a gap", "handle and views interleaved")
RUN_COUNT = {"one handle": 1, "2 handles": 2, "3 handles": 3, "4 handles": 4, "5 handles": 5, "9 handles": 9,
             "adjacent views": 1, "views with a gap": 2, "handle and views interleaved": 3}


def build_level(ctx, H, a, variant, rng):
    """append the columns of `a` (ncols, 2^log) to the commit `H` as `variant` lays them out"""
    a = np.ascontiguousarray(a, dtype=U32)
    n, log = a.shape[0], a.shape[1].bit_length() - 1
    if variant.endswith("handles") or variant == "one handle":
        first = 0
        for k in _split(n, RUN_COUNT[variant]):
            separate_handle(ctx, H, a[first:first + k])
            first += k
    elif variant == "adjacent views":        # [0, n1) and [n1, n) of one allocation: the planner merges them into one run
        whole = ctx.col_from_cpu(a)
        H.keep.append(whole)
        n1 = max(1, n // 2)
        H.add(whole.view(0, n1), a[:n1])
        H.add(whole.view(n1, n - n1), a[n1:])
    elif variant == "views with a gap":      # a column that is not committed lies between the two views
        n1 = max(1, n // 2)
        whole = ctx.col_from_cpu(np.concatenate([a[:n1], _junk(rng, log), a[n1:]]))
        H.keep.append(whole)
        H.add(whole.view(0, n1), a[:n1])
        H.add(whole.view(n1 + 1, n - n1), a[n1:])
    elif variant == "handle and views interleaved":   # view of B's column 0 | handle A | view of B's column 2
        other = ctx.col_from_cpu(np.concatenate([a[:1], _junk(rng, log), a[n - 1:]]))
        H.keep.append(other)
        H.add(other.view(0, 1), a[:1])
        separate_handle(ctx, H, a[1:n - 1])
        H.add(other.view(2, 1), a[n - 1:])
    else:
        raise ValueError(variant)


# ----------------------------------------------------------------------------- one tree
def decommit_queries(logs, seed):
    rng = np.random.default_rng(seed)
    q = {}
    for lg in sorted(set(logs), reverse=True):
        n = 1 << lg
        q[lg] = sorted({0, n - 1} | {int(v) for v in rng.integers(0, n, size=3)})
    return q


def check_tree(ctx, H, what, expect=(), sub_env=None, want=None, seed=0, root_form=True):
    """commit H, compare everything with the reference (module docstring) -> the reference layers"""
    from level2_decommit_checks import assert_opening_equals_oracle
    cols = H.cols
    logs = [len(c).bit_length() - 1 for c in cols]
    max_log = max(logs)
    want = ref_layers(cols) if want is None else want
    root = want[0][0].astype("<u4").tobytes()
    p = plan(col_addresses(H.commit), sub_env)
    forms = plan_forms(p)
    for f in expect:
        assert f in forms, "%s: meant to reach %s, the planner takes %s" % (what, f, p)
    t0 = ctx.timings()
    tree = ctx.commit(H.commit)
    try:
        t1 = ctx.timings()
        got = (t1["merkle_launches"] - t0["merkle_launches"], t1["merkle_fused_launches"] - t0["merkle_fused_launches"])
        assert got == (len(p), sum(f.startswith("fused") for f, _, _, _ in p)), \
            "%s: (launches, fused launches) %s, the restated planner has %s" % (what, got, p)
        dev = [layer_words(tree, lg) for lg in range(max_log + 1)]
        for lg in range(max_log, -1, -1):          # leaves first: the first wrong layer is where the fault is
            same_layer(dev[lg], want[lg], "%s %s: layer %d" % (what, p, lg))
        assert tree.log_size == max_log, (what, tree.log_size)
        assert tree.root() == root, what
        if max_log <= PY_MAX_LOG:                  # the wrapper's own form of a layer
            for lg in range(max_log + 1):
                assert tree.layer(lg) == [r.astype("<u4").tobytes() for r in want[lg]], (what, lg)
        else:
            rehash_device_sample(dev, cols, seed + 1, what)
        t = types.SimpleNamespace(tree=tree, handles=H.commit, log_sizes=logs)
        assert_opening_equals_oracle(t, ref_tree(cols, want), decommit_queries(logs, seed + 2), what + ": decommit")
    finally:
        tree.free()
    if root_form:
        assert ctx.merkle_root(cols) == root, what + ": merkle_root"
    return want


def random_cols(rng, ncols, log, cls="random"):
    return words(cls, (ncols, 1 << log), rng).astype(U32)


def simple_tree(ctx, shape, what, expect=(), sub_env=None, seed=0, cls="random", root_form=True):
    """shape: [(ncols, log)] one handle each, commit order"""
    rng = np.random.default_rng(seed)
    H = Handles()
    try:
        for ncols, log in shape:
            separate_handle(ctx, H, random_cols(rng, ncols, log, cls))
        return check_tree(ctx, H, what, expect, sub_env, seed=seed, root_form=root_form)
    finally:
        H.free()


# ----------------------------------------------------------------------------- the axes
def leaf_form(ncols, log):
    if log <= 10:
        return "small<1>" if ncols <= 16 else "small<0>"
    return "fused<1,%d>" % next(nz for nz in (4, 8, 12, 15, 16) if ncols <= nz) if ncols <= 16 else "fused<0>x1"


def check_leaf_count(ctx, ncols, log, classes=("random",), sub_env=None, expect_sub=None):
    """a single-size tree of one handle (one run) on a dirtied context: stale words next to a short column must not
    pass for its zeros"""
    nc.dirty_context(ctx, np.random.default_rng(ncols))
    expect = [leaf_form(ncols, log)] + (["sub=%d" % expect_sub] if expect_sub is not None else [])
    for cls in classes:
        simple_tree(ctx, [(ncols, log)], "leaf of %d columns, 2^%d leaves, %s" % (ncols, log, cls), expect, sub_env,
                    seed=1000 * log + ncols, cls=cls)


def check_children_plus_columns(ctx, top_log, own_log, nown):
    """a 1-column level at top_log, then nown columns at own_log: children plus 1, 2, 15, 16, 17, 32 words"""
    form = "small<0>" if own_log <= 10 else "fused<0>x1"
    simple_tree(ctx, [(1, top_log), (nown, own_log)], "1 column at 2^%d over %d at 2^%d" % (top_log, nown, own_log), [form],
                seed=100 * top_log + 10 * own_log + nown)


def check_runs(ctx, log, with_children, ncols=9):
    """one logical level of `ncols` columns built in every RUN_VARIANTS way (under a 1-column level of 2^(log+1) when
    with_children): the same layers every time"""
    rng = np.random.default_rng(31 * log + with_children)
    a = random_cols(rng, ncols, log)
    top = random_cols(rng, 1, log + 1) if with_children else None
    want = None
    for v in RUN_VARIANTS:
        H = Handles()
        try:
            if top is not None:
                separate_handle(ctx, H, top)
            build_level(ctx, H, a, v, rng)
            nruns = RUN_COUNT[v]
            if nruns > MERKLE_MAX_SEG:
                form = "layer"
            elif log <= 10:
                form = "small<1>" if nruns == 1 and not with_children else "small<0>"
            else:
                form = "fused<1,12>" if nruns == 1 and not with_children else "fused<0>x%d" % nruns
            what = "%d columns at 2^%d as %s%s" % (ncols, log, v, ", with children" if with_children else "")
            want = check_tree(ctx, H, what, [form], want=want, seed=log, root_form=v == "one handle")
        finally:
            H.free()


def check_root_form_layouts(ctx):
    """lmn_op_merkle_root uploads column after column into the arena: columns shorter than 256 bytes are one run each, so
    five of them reach k_merkle_layer; unsorted input leaves the sorted level in two runs"""
    rng = np.random.default_rng(5)
    for logs, form in (([4] * 5, "layer"), ([5] * 9, "layer"), ([3] * 4, "small<0>"), ([7, 5, 5, 5, 5, 5, 5], "layer"),
                       ([6] * 9, "small<1>"), ([12, 12, 10, 12, 3], "fused<0>x2"), ([11] * 17, "fused<0>x1"),
                       ([11, 3, 11], "fused<0>x2")):
        cols = [random_cols(rng, 1, lg)[0] for lg in logs]
        p = plan(arena_addresses(logs))
        assert form in plan_forms(p), (logs, form, p)
        t0 = ctx.timings()
        got = ctx.merkle_root(cols)
        t1 = ctx.timings()
        assert got == ref_layers(cols)[0][0].astype("<u4").tobytes(), (logs, p)
        assert t1["merkle_launches"] - t0["merkle_launches"] == len(p), (logs, p)
    assert ctx.merkle_root([]) == hashlib.blake2s(b"").digest()


def check_single_size(ctx, log, ncols, sub_env=None, expect=()):
    simple_tree(ctx, [(ncols, log)], "%d columns of 2^%d%s" % (ncols, log, "" if sub_env is None else ", LMN_MERKLE_SUB=%d" % sub_env),
                list(expect) + [leaf_form(ncols, log)], sub_env, seed=log * 7 + ncols + 100 * (sub_env or 0))


def mixed_shapes(k):
    """(name, [(ncols, log)] commit order, forms) against the planner, tallest level 2^k (k >= 12)"""
    return [
        ("levels k, k-1", [(2, k - 1), (3, k)], ()),
        ("levels k, k-2", [(3, k), (2, k - 2)], ("fused<0>x1",) if k >= 13 else ()),
        ("levels k, 10", [(1, 10), (5, k)], ("small<0>",)),
        ("levels k, 11", [(5, k), (17, 11)], ("fused<0>x1",)),
        ("levels k, 0", [(2, 0), (9, k)], ("small<0>",)),
        ("levels k, 3, 2, 1, 0", [(1, 0), (2, 1), (13, k), (1, 2), (3, 3)], ("small<0>", "small<2>")),
        ("tallest level of 8 columns over a level with columns", [(8, k), (4, k - 1)], ()),
        ("tallest level of 2 columns over a level with 16", [(2, k), (16, k - 1)], ()),
    ]


def check_mixed(ctx, name, shape, forms, sub_env=None):
    simple_tree(ctx, shape, "%s %s" % (name, shape), forms, sub_env, seed=sum(n * lg for n, lg in shape))


def check_fused_run_end(ctx, top, cap, sub_env=None):
    """the fused launch from level `top` covers at most `cap` further levels (min(11, top - 10, sub + 8)).  Columns at
    level top - cap, where such a run ends, cut it one level short; columns at the level after it leave it whole.  The
    length of the first launch is asserted on the restated plan, whose launch counts check_tree compares."""
    for own in (top - cap, top - cap - 1):
        H = Handles()
        try:
            rng = np.random.default_rng(top * 100 + own)
            separate_handle(ctx, H, random_cols(rng, 4, top))
            separate_handle(ctx, H, random_cols(rng, 3, own))
            p = plan(col_addresses(H.commit), sub_env)
            assert p[0][1] == top and p[0][2] == (cap - 1 if own == top - cap else cap), (top, own, cap, p)
            check_tree(ctx, H, "4 columns at 2^%d, 3 at 2^%d" % (top, own), (), sub_env, seed=top + own,
                       root_form=sub_env is None)
        finally:
            H.free()


def check_refusals_leave_context_usable(ctx):
    """log 0 and 1 are accepted by both forms; what is refused is an empty commit and a null handle
    (LMN_ERR_INVALID_ARGUMENT), and the context goes on to a right answer"""
    from luminair_amd.backend import ERR_INVALID_ARGUMENT, LuminairBackendError
    try:
        ctx.commit([])
    except LuminairBackendError as e:
        assert e.code == ERR_INVALID_ARGUMENT, (e.code, str(e))
    else:
        raise AssertionError("an empty commit was accepted")
    big = np.zeros(2, dtype=U32)
    try:
        import ctypes as C
        root = (C.c_uint8 * 32)()
        ptrs = (C.c_void_p * 1)(big.ctypes.data)
        logs = (C.c_uint32 * 1)(27)
        ctx._check(ctx.lib.lib.lmn_op_merkle_root(ctx.handle, ptrs, logs, 1, root))
    except LuminairBackendError as e:
        assert e.code == ERR_INVALID_ARGUMENT, (e.code, str(e))
    else:
        raise AssertionError("a column of 2^27 words was accepted by merkle_root")
    simple_tree(ctx, [(2, 1), (1, 0)], "after the refusals", ["small<1>"])
