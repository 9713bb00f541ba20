"""The FRI commit loop layer by layer (`lmn_col_fri_commit` = phase_fri.cpp `fri_commit_layers`, the loop `prove` runs):
k_merkle_fused<3> (the line / circle fold inside the next layer's leaf hashing, with and without a joining quotient column),
k_merkle_fused<4> (the first tree's leaf level hashed by the launch of the level above it), k_fri_tail (with and without its
front fold, 1 to 9 layers), k_fold where the loop falls back to it, and the device-resident mix_root + draw between layers.
Run against the emulation build on CPU (tests/test_fri_commit_emu.py) and the HIP library on GPU (tests/test_gpu_fri_commit.py).

Reference - never the library under test.  `ref_commit` restates `fri_commit_phase` of oracle/prover.py without the degree
check that follows it.  Folds: plain Python integers up to 2^8 points (numeric_checks.ref_fold_line / ref_fold_circle; the numpy oracle must
give the same there, which pins it), the numpy oracle above, the C oracle from 2^17.  Trees: every node by hashlib.blake2s up
to 2^10 leaves (merkle_checks.hashlib_layers, pinning oracle.merkle.MerkleTree), numpy above, the C oracle from 2^17.  Channel:
oracle.channel in both draw encodings (pinned by the known-answer test).

What a case asserts (`check_case`): every root and alpha; every layer's values in full (the message names the layer, its
form, the first differing index and how many words differ); every tree level the loop wrote, in full; the set of levels it
did not write == `plan()`'s; every output word < P; the per-layer form codes == `plan()`; and the same inputs under
LMN_NO_FOLD_FUSION=1 and LMN_NO_JOIN_FUSION=1 give identical roots, alphas and layer values (and the forms `plan()` names for
those switches) - every case, the large GPU ones included: the reference is computed once per case.  `plan()` restates phase_fri.cpp's conditions and the `sub` / `below` thresholds of commit.cpp.

The transcript's value edges (REDRAW_CASES): start digests found by tools/find_redraw.cpp (tests/golden/transcript_redraw_seeds.json,
pinned against hashlib by tests/test_transcript_redraw_seeds.py) at which the draw behind a chosen tree goes round its loop a second
time (a word >= 2P; the exact words 0xFFFFFFFE and 0xFFFFFFFF, among words 0..3 and among words 4..7, which `draw_felt` never uses),
or accepts 0xFFFFFFFD (-> P - 1) or a word P (-> 0).  Random columns put the event at tree 0, whose root no alpha reaches - the
redrawn alpha is then used by every fold behind it; all-zero and constant columns fold to constants whatever alpha is, so every
root is known beforehand and the event can sit at an inner tree or at the first, a middle or the last layer of k_fri_tail - the
alphas are asserted directly and the layers behind the redraw show that the digest was carried on.  The reference runs on a
counting channel and must have met the event at that tree and nowhere else before the library is asked
(`check_redraw_reference`): a seed that a protocol change has made stale fails, it does not pass.  Two redraws in a row
(about 2^56 trials) are out of reach.

Two things the loop's construction rules out, so no case can hold them:
  * a tail of 10 layers: the tail starts at 2^10 at most and ends above the last layer of 2^(log_last_layer + log_blowup)
    values, and a context refuses log_blowup < 1 - 9 layers (2^10 .. 2^2) is the longest tail there is (TAIL_MAX_LAYERS;
    test_plan_tail_lengths asserts it over every configuration);
  * a joining column chosen, from the alphas, so that the joined layer is exactly 0: the first tree commits ALL the columns,
    the joining one included, so every alpha is a hash of that column and c = -(alpha^2 fold(prev)) / 2 has no solution that
    does not need alpha first (alpha^2 f0 + alpha^3 f1 + g0 + alpha g1 = 0 for an alpha not known when g is fixed forces
    f = g = 0).  The zero-landing join is therefore the all-zero class on the join shapes (the reference is asserted to be 0
    from the joined layer on before the kernel is asked), and pairs with a + b = 0 / a == b are run on the joining column
    as on every other.  Next to it, each term of the join alone at 0 with the other live (HALF_ZERO_CASES): cols[0] all zero
    under a random joining column (alpha^2 * prev = 0, the joining column's fold live) and a random cols[0] under an all-zero
    joining column (the fold term 0, alpha^2 * prev live); the reference is asserted to say so."""
import os
import zlib
from contextlib import contextmanager
from dataclasses import dataclass, field

import numpy as np

import merkle_checks as mc
import numeric_checks as nc
from numeric_checks import P, U64

U32 = np.uint32
# backend.FRI_* (include/luminair_hip.h LMN_FRI_*)
LAUNCH, IN_LEAVES, IN_LEAVES_JOIN, MATERIALISED, TAIL_FRONT, IN_TAIL = 1, 2, 3, 4, 5, 6
TREE_OWN, TREE_IN_TAIL = 0x100, 0x200
FIRST_TREE, FIRST_TREE_BELOW = 0x10000, 0x10001
ALL_FORMS = {LAUNCH, IN_LEAVES, IN_LEAVES_JOIN, MATERIALISED, TAIL_FRONT, IN_TAIL, TREE_OWN, TREE_IN_TAIL, FIRST_TREE,
             FIRST_TREE_BELOW}
FORM_NAMES = {LAUNCH: "fold launch", IN_LEAVES: "fold in the leaf launch", IN_LEAVES_JOIN: "fold + join in the leaf launch",
              MATERIALISED: "pending fold materialised", TAIL_FRONT: "tail front fold", IN_TAIL: "fold inside the tail",
              TREE_OWN: "own tree launches", TREE_IN_TAIL: "tree inside the tail", 0: "no tree"}
MERKLE_MAX_SUB, MERKLE_MAX_FUSED = 3, 11      # kernels.h
TAIL_MAX_LAYERS = 9
C_MIN_LOG = 17                                # the C oracle from 2^17 points / leaves
VALUE_CLASSES = ("zero", "pm1", "alt", "edge", "random", "sum0", "equal")


def form_name(f):
    return "%s, %s" % (FORM_NAMES[f & 0xff], FORM_NAMES[f & 0xf00])


# ----------------------------------------------------------------------------- the planner, restated
@dataclass
class Plan:
    first_form: int
    layer_logs: list
    layer_forms: list
    absent: list            # per tree: the levels the loop does not write
    n_tail: int
    first_launches: list = None     # the first tree's Merkle launches, leaves first: (the level a launch reads, levels it hashes above)

    def forms(self):
        out = {self.first_form}
        for f in self.layer_forms:
            out |= {f & 0xff, f & 0xf00} - {0}
        return out


def tree_absent(ncols, max_log, fold, sub_env, below_min_log, launches=None):
    """commit.cpp build_merkle_levels inside prove (with cuts) -> (levels not written, leaf level hashed from above);
    `launches`: a list that receives (the level a launch reads, the levels it hashes above that one), leaves first - a launch
    that reads a level <= 10 is k_merkle_small"""
    absent, below, prev, level = set(), False, False, max_log
    below_min_log = max(12, below_min_log)
    while level >= 0:
        nc_ = ncols.get(level, 0)
        if not fold and not prev and level == max_log and level >= below_min_log and 0 < nc_ <= 8 and ncols.get(level - 1, 0):
            below = True
            absent.add(level)
            level -= 1
            continue
        plain = 0
        while level - plain - 1 >= 0 and not ncols.get(level - plain - 1, 0):
            plain += 1
        if level <= 10:
            nfused = min(plain, 10)
        else:
            nfused = min(plain, MERKLE_MAX_FUSED, level - 10)
            sub = max(0, min(MERKLE_MAX_SUB, nfused, level - 17))
            if sub_env is not None:
                sub = min(sub_env, nfused, MERKLE_MAX_SUB)
            nfused = min(nfused, sub + 8)
            absent |= {level - l for l in range(sub)}
        if launches is not None:
            launches.append((level, nfused))
        prev, level = True, level - nfused - 1
    return absent, below


def plan(logs, last_log, fuse_folds=True, fuse_joins=True, sub_env=None, below_min_log=19):
    """phase_fri.cpp plan_fri_layout + fri_commit_layers for an unsharded context"""
    n, ls0 = len(logs), logs[0]
    assert all(a > b for a, b in zip(logs, logs[1:])) and ls0 - 1 >= last_log and logs[-1] - 1 >= last_log
    tail_log = min(10, ls0 - 1, logs[-1] - 1)
    if tail_log <= last_log:
        tail_log = -1
    first_launches = []
    first_absent, below = tree_absent({lg: 4 for lg in logs}, ls0, False, sub_env, below_min_log, first_launches)
    absent, forms, n_tail = [first_absent], [], 0
    layer_log, qi = ls0 - 1, 1
    pend, pend_join = fuse_folds, False
    produced = 0 if pend else LAUNCH
    while layer_log > last_log:
        if pend and layer_log <= 10:
            produced, pend = MATERIALISED, False
        if layer_log <= 10 and qi == n:
            assert layer_log == tail_log, (logs, last_log, layer_log, tail_log)
            n_tail = layer_log - last_log
            forms.append(produced | TREE_IN_TAIL)
            forms += [IN_TAIL | TREE_IN_TAIL] * (n_tail - 1)
            absent += [set() for _ in range(n_tail)]
            produced, layer_log = IN_TAIL, last_log
            break
        if pend:
            produced, pend = (IN_LEAVES_JOIN if pend_join else IN_LEAVES), False
            absent.append(tree_absent({layer_log: 4}, layer_log, True, sub_env, below_min_log)[0])
        else:
            absent.append(tree_absent({layer_log: 4}, layer_log, False, sub_env, below_min_log)[0])
        forms.append(produced | TREE_OWN)
        next_log = layer_log - 1
        joins = qi < n and logs[qi] - 1 == next_log
        if fuse_folds and next_log > 10 and (not joins or fuse_joins):
            pend, pend_join, produced = True, joins, 0
            qi += joins
        elif fuse_folds and not joins and qi == n and next_log == tail_log and next_log > last_log:
            produced = TAIL_FRONT
        else:
            produced = LAUNCH
        while qi < n and logs[qi] - 1 == next_log:
            qi += 1
        layer_log = next_log
    if pend:
        produced = MATERIALISED
    forms.append(produced)
    assert qi == n
    return Plan(FIRST_TREE_BELOW if below else FIRST_TREE, [ls0 - 1 - i for i in range(len(forms))], forms, absent, n_tail, first_launches)


# ----------------------------------------------------------------------------- reference
def _pin(got, want, what):
    nc.same(np.asarray(got).T, want, "numpy oracle " + what)


def ref_fold_line(src, alpha):
    """(4, 2^k) -> (4, 2^(k-1)), uint64"""
    from oracle.circle import Coset, LineDomain
    from oracle.field import QM31
    k = src.shape[1].bit_length() - 1
    if k >= C_MIN_LOG:
        return nc._c_oracle().fold_line(np.ascontiguousarray(src, dtype=U32), QM31(*alpha), LineDomain(Coset.half_odds(k))).astype(U64)
    want = nc.ref_fold_line(src.astype(U64), alpha)
    if k <= nc.PY_MAX_LOG:
        from oracle.prover import fold_line
        _pin(fold_line(src.T.astype(U64), QM31(*alpha), LineDomain(Coset.half_odds(k))), want, "fold_line 2^%d" % k)
    return want


def ref_fold_circle(dst, src, alpha):
    """dst * alpha^2 + fold(src); dst None = zeros"""
    from oracle.field import QM31
    k = src.shape[1].bit_length() - 1
    if k >= C_MIN_LOG:
        d = None if dst is None else np.ascontiguousarray(dst, dtype=U32)
        return nc._c_oracle().fold_circle_into_line(d, np.ascontiguousarray(src, dtype=U32), QM31(*alpha), k).astype(U64)
    if dst is None:
        dst = np.zeros((4, src.shape[1] // 2), dtype=U64)
    want = nc.ref_fold_circle(dst.astype(U64), src.astype(U64), alpha)
    if k <= nc.PY_MAX_LOG:
        from oracle.prover import fold_circle_into_line
        _pin(fold_circle_into_line(dst.T.astype(U64), src.T.astype(U64), QM31(*alpha), k), want, "fold_circle_into_line 2^%d" % k)
    return want


@dataclass
class Ref:
    roots: list = field(default_factory=list)
    alphas: list = field(default_factory=list)
    trees: list = field(default_factory=list)     # [tree][level] -> (2^level, 8)
    layers: list = field(default_factory=list)    # (4, 2^log) uint64, the last layer last


def ref_commit(cols, digest, variant, last_log, channel=None):
    """oracle/prover.py fri_commit_phase, on (4, 2^log) columns of strictly decreasing sizes, without the degree check;
    `channel`: the (counting) channel to run it on"""
    from oracle.channel import Blake2sChannel
    ch = Blake2sChannel(variant) if channel is None else channel
    ch.digest = digest
    R = Ref()

    def commit(columns):
        layers = mc.ref_layers(columns)
        R.trees.append(layers)
        root = layers[0][0].astype("<u4").tobytes()
        ch.mix_root(root)
        R.roots.append(root)
        a = tuple(int(v) for v in ch.draw_felt().v)
        R.alphas.append(a)
        return a
    logs = [c.shape[1].bit_length() - 1 for c in cols]
    alpha = commit([c[k].astype(U32) for c in cols for k in range(4)])
    layer, layer_log, qi = ref_fold_circle(None, cols[0], alpha), logs[0] - 1, 1
    assert layer_log >= last_log
    while layer_log > last_log:
        R.layers.append(layer)
        alpha = commit([layer[k].astype(U32) for k in range(4)])
        layer = ref_fold_line(layer, alpha)
        layer_log -= 1
        while qi < len(cols) and logs[qi] - 1 == layer_log:
            layer = ref_fold_circle(layer, cols[qi], alpha)
            qi += 1
    assert qi == len(cols), "unconsumed columns"
    R.layers.append(layer)
    return R


# ----------------------------------------------------------------------------- inputs
def column(cls, log, rng):
    """(4, 2^log) uint32 in a value class; sum0: pairs (a, P - a), f0 = 0; equal: pairs (a, a), f1 = 0"""
    n = 1 << log
    if cls == "const":          # one non-zero QM31 everywhere: every fold of it is constant whatever alpha is
        return np.repeat(rng.integers(1, P, size=(4, 1), dtype=U64), n, axis=1).astype(U32)
    if cls in ("sum0", "equal"):
        a = nc.words("random", (4, n // 2), rng)
        c = np.empty((4, n), dtype=U64)
        c[:, 0::2] = a
        c[:, 1::2] = (U64(P) - a) % U64(P) if cls == "sum0" else a
        return c.astype(U32)
    return nc.words(cls, (4, n), rng).astype(U32)


@dataclass(frozen=True)
class Case:
    name: str
    logs: tuple
    lll: int = 0            # log_last_layer
    lb: int = 1             # log_blowup
    u32: bool = False       # LMN_PV_DRAW_CTR_U32
    sub: int = None         # LMN_MERKLE_SUB
    below: int = None       # LMN_MERKLE_BELOW_MIN_LOG
    cls: object = "random"  # a value class for every column, or one per column
    search: str = None      # REDRAW_CASES: the search (REDRAW_SEARCHES) whose record gives the start digest ...
    layer: int = None       # ... and the tree at which the event happens

    @property
    def last_log(self):
        return self.lll + self.lb

    def plan(self, fuse_folds=True, fuse_joins=True):
        return plan(list(self.logs), self.last_log, fuse_folds, fuse_joins, self.sub, 19 if self.below is None else self.below)

    @property
    def id(self):
        return self.name.replace(" ", "_")


def _c(name, logs, **kw):
    return Case(name, tuple(logs), **kw)


# The matrix of the CPU suite (all <= 2^14), also run on the GPU.  Default configuration: last layer 2^1.
SHAPE_CASES = [
    # ls0 - 1 in {3, 9, 10, 11, 12}: first layer materialised / fused, tail from the first layer / behind it
    _c("first layer 3 tail of 2", [4]),
    _c("first layer 9 tail of 8", [10], u32=True),
    _c("first layer 10 tail of 9", [11]),
    _c("first layer 11 tail front", [12]),
    _c("first layer 12 two fused folds", [13], u32=True),
    # tail lengths 1, 2 (above), 9 (above); no tail
    _c("tail of 1 blowup 2", [4], lb=2),
    _c("tail of 1 last layer 3", [6], lll=3, u32=True),
    _c("no tail last layer 11 pending at the end", [13], lll=10),
    _c("no tail last layer 12 blowup 2", [14], lll=10, lb=2, u32=True),
    _c("no tail join below the tail start", [9, 5], lll=3),
    _c("loop never runs below 10", [5], lll=3),
    _c("loop never runs above 10", [12], lll=10),
    _c("loop never runs blowup 3", [14], lll=10, lb=3, u32=True),
    _c("blowup 3 last layer 0", [13], lb=3),
    _c("blowup 2 last layer 3 join", [12, 8], lll=3, lb=2),
    # joins
    _c("join at 12 fused", [14, 13]),
    _c("join at 11 fused", [13, 12], u32=True),
    _c("join at 10 tail starts there", [13, 11]),
    _c("join at 9 layer 10 on its own", [12, 10]),
    _c("join at 5", [12, 6], u32=True),
    _c("join into the last layer", [5, 2]),
    _c("join into the last layer 11", [14, 12], lll=10),
    _c("two joins consecutive", [14, 13, 12], u32=True),
    _c("three joins", [14, 12, 11, 6]),
    _c("joins at 10 and 9", [13, 11, 10]),
    _c("small joins every layer", [7, 6, 5, 4, 3]),
    # the first tree with columns at ls0 and ls0 - 1: leaf level hashed by the launch above it
    _c("below at 12", [12, 11], below=12),
    _c("below at 14 with a fused join", [14, 13], below=12, u32=True),
    _c("below at 13 sub 2", [13, 12, 9], below=12, sub=2),
    _c("not below: threshold 14", [13, 12], below=14),
] + [_c("sub %d at 14" % s, [14], sub=s, u32=bool(s & 1)) for s in (0, 1, 2, 3)] + [
    _c("sub 3 at 14 with joins", [14, 13, 11], sub=3),
]
# one term of a join at 0, the other live: (cols[0], joining columns ...)
HALF_ZERO_CASES = [_c("zero first column random join fused", [13, 12], cls=("zero", "random")),
                   _c("random first column zero join fused", [13, 12], cls=("random", "zero")),
                   _c("zero first column random small joins", [8, 7, 5], cls=("zero", "random", "random")),
                   _c("random first column zero small joins", [8, 7, 5], cls=("random", "zero", "zero"))]
CLASS_CASES = [_c("%s fused join front tail" % cls, [13, 12], cls=cls) for cls in VALUE_CLASSES] + \
              [_c("%s tail only" % cls, [9], cls=cls) for cls in VALUE_CLASSES] + \
              [_c("%s small joins" % cls, [8, 7, 5], cls=cls) for cls in ("zero", "sum0", "equal", "edge")] + HALF_ZERO_CASES
CASES = SHAPE_CASES + CLASS_CASES

# The transcript's value edges (tests/transcript_seeds.py): one search of tools/find_redraw.cpp each, one record - a start
# digest - per listed tree.  Random columns: the event at tree 0, whose root no alpha reaches; the redrawn alpha is used by
# every fold behind it.  "zero" / "const" columns fold to a constant whatever alpha is, so every root is fixed and the event
# can be placed at any tree: [11] = the first tree, then a tail of 9 (trees 1 .. 9); [12] = the first tree, layer 2^11 as an
# inner tree of its own (tree 1), then the tail behind its front fold (tree 2 = its first layer).  value: the exact word;
# lo, hi: the word indices the event may lie at (a redraw: no rejected word outside them).
def _s(name, logs, event, layers=(0,), value="any", lo=0, hi=7, **kw):
    return dict(name=name, logs=tuple(logs), event=event, layers=tuple(layers), value=value, lo=lo, hi=hi, u32=kw.pop("u32", False),
                cls=kw.pop("cls", "random"))


REDRAW_SEARCHES = [
    _s("redraw tree 0 small FFFFFFFE in words 0 to 3", [10], "redraw", value="FFFFFFFE", hi=3),
    _s("redraw tree 0 small FFFFFFFF in words 4 to 7 u32", [10], "redraw", value="FFFFFFFF", lo=4, u32=True),
    _s("redraw tree 0 large FFFFFFFF in words 0 to 3", [12], "redraw", value="FFFFFFFF", hi=3),
    _s("redraw tree 0 large FFFFFFFE in words 4 to 7 u32", [12], "redraw", value="FFFFFFFE", lo=4, u32=True),
    _s("accept edge tree 0 small", [10], "accept-edge", hi=3),
    _s("accept edge tree 0 large u32", [12], "accept-edge", hi=3, u32=True),
    _s("reduce edge tree 0 large", [12], "reduce-edge", hi=3),
    _s("reduce edge tree 0 small u32", [10], "reduce-edge", hi=3, u32=True),
    _s("redraw zero tail", [11], "redraw", layers=(1, 5, 9), cls="zero"),
    _s("redraw const tail u32", [11], "redraw", layers=(1, 5, 9), cls="const", u32=True),
    _s("redraw const inner and front tail", [12], "redraw", layers=(1, 2), cls="const"),
    _s("redraw zero inner and front tail u32", [12], "redraw", layers=(1, 2), cls="zero", u32=True),
]
REDRAW_CASES = [_c("%s tree %d" % (s["name"], t), s["logs"], u32=s["u32"], cls=s["cls"], search=s["name"], layer=t)
                for s in REDRAW_SEARCHES for t in s["layers"]]
SEARCH_OF = {s["name"]: s for s in REDRAW_SEARCHES}
DRAW_SITES = {"k_merkle_small, the whole first tree", "k_merkle_small, the top of the first tree", "k_merkle_small, inner tree", "k_fri_tail, first layer",
              "k_fri_tail, first layer behind the front fold", "k_fri_tail, middle layer", "k_fri_tail, last layer"}


def draw_site(case, fuse_folds=True):
    """which statement of the draw loop the case's event reaches, from plan() alone"""
    pl, t = case.plan(fuse_folds), case.layer
    if t == 0:
        # the launch that reaches the root mixes it and draws: k_merkle_small if it reads a level <= 10 and hashes up to level
        # 0 (anything else would leave the root to the single-lane k_chan_mix_root_draw)
        level, above = pl.first_launches[-1]
        assert pl.first_form == FIRST_TREE and level <= 10 and level - above == 0, (case.name, pl.first_launches)
        if len(pl.first_launches) == 1:
            assert level == case.logs[0], (case.name, pl.first_launches)
            return "k_merkle_small, the whole first tree"
        assert pl.first_launches[0][0] == case.logs[0] > 10, (case.name, pl.first_launches)
        return "k_merkle_small, the top of the first tree"      # behind the fused launches of the levels above 10
    f = pl.layer_forms[t - 1]
    if f & TREE_OWN:
        return "k_merkle_small, inner tree"
    assert f & TREE_IN_TAIL, (case.name, hex(f))
    k = t - 1 - next(i for i, g in enumerate(pl.layer_forms) if g & TREE_IN_TAIL)
    if k == 0:
        return "k_fri_tail, first layer" + (" behind the front fold" if f & 0xff == TAIL_FRONT else "")
    return "k_fri_tail, %s layer" % ("last" if k == pl.n_tail - 1 else "middle")


def check_redraw_cases_reach_every_draw(cases):
    """Between them the redraws reach every statement of the draw loop an unsharded context can, in both encodings per kernel.
    Every tree's top is hashed by k_merkle_small (step kind 0: chan_mix_root_draw_block) or lies in k_fri_tail (the same
    function, the digest carried in registers).  The single-lane k_chan_mix_root_draw is out of reach here: commit.cpp
    launches it only when no k_merkle_small launch reaches the root with the channel - the root level itself scattered over
    more runs of columns than a launch takes (columns of one value: no FRI column is), or the tree of a sharded context with
    one shard, whose root is hashed before the gather.  `lmn_col_fri_commit` refuses a sharded context."""
    redraws = [c for c in cases if SEARCH_OF[c.search]["event"] == "redraw"]
    sites = {draw_site(c) for c in redraws}
    assert sites == DRAW_SITES, sorted(DRAW_SITES ^ sites)
    for kernel in ("k_merkle_small", "k_fri_tail"):
        assert {c.u32 for c in redraws if draw_site(c).startswith(kernel)} == {False, True}, kernel
    # LMN_NO_FOLD_FUSION=1 takes the front fold out of the tail: the same seeds meet the tail behind a fold launch
    assert "k_fri_tail, first layer" in {draw_site(c, False) for c in redraws if "front" in draw_site(c)}
    assert {SEARCH_OF[c.search]["event"] for c in cases} == {"redraw", "accept-edge", "reduce-edge"}
    values = {(SEARCH_OF[c.search]["value"], SEARCH_OF[c.search]["lo"] >= 4) for c in redraws}
    assert {("FFFFFFFE", False), ("FFFFFFFF", False), ("FFFFFFFE", True), ("FFFFFFFF", True)} <= values, values


def case_columns(case, seed=0):
    """-> (columns, the generator behind them): a redraw case's columns are its search's"""
    rng = np.random.default_rng(seed + zlib.crc32((case.search or case.name).encode()))
    classes = [case.cls] * len(case.logs) if isinstance(case.cls, str) else list(case.cls)
    assert len(classes) == len(case.logs), case.name
    return [column(cls, lg, rng) for cls, lg in zip(classes, case.logs)], classes, rng


def check_redraw_reference(case, rec, chan, ref):
    """the reference met the event where the record says, and nowhere else, before the library is asked: a seed that a
    protocol change has made stale fails here"""
    import transcript_seeds as ts
    s, n = SEARCH_OF[case.search], len(ref.roots)
    given = n if case.cls in ("zero", "const") else 1
    assert [r.hex() for r in ref.roots[:given]] == rec["roots"], "%s: the searcher was given other roots than the reference's" % case.name
    assert rec["event"] == s["event"] and rec["encoding"] == (37 if case.u32 else 64) and rec["layer"] == case.layer, case.name
    assert s["lo"] <= rec["word_index"] <= s["hi"] and s["value"] in ("any", rec["word_value"][2:]), (case.name, rec)
    ts.check_chain(rec, chan, n, case.name)
    a = ref.alphas[case.layer]
    if rec["event"] == "accept-edge":
        assert a[rec["word_index"]] == P - 1, (case.name, a)
    elif rec["event"] == "reduce-edge":
        assert a[rec["word_index"]] == 0, (case.name, a)
    else:   # the alpha is that of the second draw
        w = ts.draw_words(chan.digest_after[case.layer], 1, rec["encoding"])
        assert a == tuple(x % P for x in w[:4]) and a != tuple(x % P for x in ts.draw_words(chan.digest_after[case.layer], 0, rec["encoding"])[:4])
    if case.cls == "const":
        assert all(l.any() and (l == l[:, :1]).all() for l in ref.layers), case.name


def check_matrix_reaches_every_form(cases):
    """a condition on plan() alone"""
    default = set()
    for c in cases:
        default |= c.plan().forms()
    assert default == ALL_FORMS, "forms no case reaches without a switch: %s" % sorted(ALL_FORMS - default)
    tails = {c.plan().n_tail for c in cases}
    assert {0, 1, 2, TAIL_MAX_LAYERS} <= tails, tails


def check_plan_tail_lengths():
    """no configuration a context accepts has a tail of more than TAIL_MAX_LAYERS layers"""
    longest = 0
    for lb in (1, 2, 3):
        for lll in range(0, 11):
            for ls0 in range(lll + lb + 1, 16):
                longest = max(longest, plan([ls0], lll + lb).n_tail)
    assert longest == TAIL_MAX_LAYERS, longest


# ----------------------------------------------------------------------------- one case
@contextmanager
def environment(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Contexts:
    """one context per (log_last_layer, log_blowup, draw encoding)"""

    def __init__(self, lib):
        self.lib, self.ctxs = lib, {}

    def get(self, case):
        from luminair_amd import backend
        key = (case.lll, case.lb, case.u32)
        if key not in self.ctxs:
            cfg = self.lib.default_config()
            cfg.log_last_layer, cfg.log_blowup = case.lll, case.lb
            cfg.protocol_variant = backend.PV_DRAW_CTR_U32 if case.u32 else 0
            self.ctxs[key] = backend.Context(0, cfg, self.lib)
        return self.ctxs[key]

    def close(self):
        for c in self.ctxs.values():
            c.close()
        self.ctxs = {}


def same_values(got, want, what):
    got, want = np.asarray(got).astype(U64), np.asarray(want).astype(U64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        k, i = (int(v) for v in bad[0])
        raise AssertionError("%s: %d of %d words differ, first at index %d (coordinate %d): got %d want %d" % (
            what, len(bad), got.size, i, k, got[k, i], want[k, i]))


def compare(case, got, ref, pl, tag):
    what = "%s %s (%s)" % (case.name, list(case.logs), tag)
    n = len(ref.roots)
    assert len(got.roots) == n and got.layer_logs == pl.layer_logs, (what, len(got.roots), n, got.layer_logs)
    assert got.first_tree_form == pl.first_form, "%s: first tree form %#x, plan() has %#x" % (what, got.first_tree_form, pl.first_form)
    assert got.layer_forms == pl.layer_forms, "%s: layer forms %s, plan() has %s" % (
        what, [hex(f) for f in got.layer_forms], [hex(f) for f in pl.layer_forms])
    # in the loop's own order: the first place that differs is where the fault is
    for t in range(n):
        lg = got.layer_logs[t]
        where = "%s: tree %d (%s)" % (what, t, "first tree" if t == 0 else "layer 2^%d, %s" % (got.layer_logs[t - 1], form_name(got.layer_forms[t - 1])))
        assert got.tree_logs[t] == len(ref.trees[t]) - 1, (where, got.tree_logs[t])
        missing = {l for l, lv in enumerate(got.tree_levels[t]) if lv is None}
        assert missing == pl.absent[t], "%s: levels not written %s, plan() has %s" % (where, sorted(missing), sorted(pl.absent[t]))
        for l in range(got.tree_logs[t], -1, -1):
            if got.tree_levels[t][l] is not None:
                mc.same_layer(got.tree_levels[t][l], ref.trees[t][l], "%s level %d" % (where, l))
        assert got.roots[t] == ref.roots[t], "%s: root %s want %s" % (where, got.roots[t].hex(), ref.roots[t].hex())
        nc.canonical_q(got.alphas[t], where + " alpha")
        assert got.alphas[t] == ref.alphas[t], "%s: alpha %s want %s" % (where, got.alphas[t], ref.alphas[t])
        where = "%s: layer 2^%d (%s)" % (what, lg, form_name(got.layer_forms[t]))
        nc.canonical(got.layer_values[t], where)
        same_values(got.layer_values[t], ref.layers[t], where)


def check_case(ctxs, case, seed=0):
    """-> the reference (for callers that assert more)"""
    ctx = ctxs.get(case)
    cols, classes, rng = case_columns(case, seed)
    digest = bytes(int(v) for v in rng.integers(0, 256, size=32))
    from oracle.channel import ProtocolVariant
    variant, chan = ProtocolVariant.DRAW_CTR_U32 if case.u32 else ProtocolVariant.KAT, None
    if case.search:
        import transcript_seeds as ts
        rec = ts.chain_record(case.search, case.layer)
        digest, chan = bytes.fromhex(rec["digest"]), ts.CountingChannel(variant)
    ref = ref_commit(cols, digest, variant, case.last_log, chan)
    if case.search:
        check_redraw_reference(case, rec, chan, ref)
    if case.cls == "zero":      # the zero-landing join: the reference says so before the kernel is asked
        assert not any(l.any() for l in ref.layers), case.name
    elif classes[0] == "zero":  # alpha^2 * prev = 0 at the first join, the joining column's fold live
        j = case.logs[0] - case.logs[1]
        assert not any(l.any() for l in ref.layers[:j]) and ref.layers[j].any(), case.name
    elif set(classes[1:]) == {"zero"}:      # the joining column's fold is 0, alpha^2 * prev live
        j = case.logs[0] - case.logs[1]
        assert not ref_fold_circle(None, cols[1], ref.alphas[j]).any() and ref.layers[j].any(), case.name
    handles = [ctx.col_from_cpu(c) for c in cols]
    try:
        runs = [("default", {}, case.plan()),
                ("LMN_NO_FOLD_FUSION=1", {"LMN_NO_FOLD_FUSION": 1}, case.plan(fuse_folds=False)),
                ("LMN_NO_JOIN_FUSION=1", {"LMN_NO_JOIN_FUSION": 1}, case.plan(fuse_joins=False))]
        first = None
        for tag, env, pl in runs:
            base = {"LMN_MERKLE_SUB": case.sub, "LMN_MERKLE_BELOW_MIN_LOG": case.below, "LMN_NO_FOLD_FUSION": None,
                    "LMN_NO_JOIN_FUSION": None, "LMN_MERKLE_FULL": None}
            with environment(**{**base, **env}):
                got = ctx.fri_commit(handles, digest)
            compare(case, got, ref, pl, tag)
            if first is None:
                first = got
            else:       # identical to the default run, whatever the reference says
                assert got.roots == first.roots and got.alphas == first.alphas, (case.name, tag)
                for a, b in zip(got.layer_values, first.layer_values):
                    assert np.array_equal(a, b), (case.name, tag)
        for h, c in zip(handles, cols):     # the loop writes none of its inputs
            assert np.array_equal(h.to_cpu(), c), case.name + ": an input column changed"
    finally:
        for h in handles:
            h.free()
    return ref


# ----------------------------------------------------------------------------- refusals
def check_refusals(ctxs):
    """LMN_ERR_INVALID_ARGUMENT with a text naming the argument; context and handles stay usable"""
    from luminair_amd.backend import ERR_INVALID_ARGUMENT, LuminairBackendError
    case = _c("after the refusals", [6, 4], lll=1)      # last layer 2^2
    ctx = ctxs.get(case)
    rng = np.random.default_rng(3)
    digest = bytes(32)

    def col(ncols, log):
        return ctx.col_from_cpu(nc.words("random", (ncols, 1 << log), rng).astype(U32))
    a6, a5, a3, a2, t6, b2 = col(4, 6), col(4, 5), col(4, 3), col(4, 2), col(3, 6), col(4, 2)
    v2 = t6.view(0, 2)
    try:
        for cols, word in (([t6], "cols[0]"), ([a6, v2], "cols[1]"), ([a5, a6], "cols[1]"), ([a6, a6], "cols[1]"),
                           ([a2], "cols[0]"), ([a6, b2], "cols[1]"), ([], "cols")):
            try:
                ctx.fri_commit(cols, digest)
            except LuminairBackendError as e:
                assert e.code == ERR_INVALID_ARGUMENT and "fri_commit" in str(e) and word in str(e), (word, e.code, str(e))
            else:
                raise AssertionError("accepted: %s" % word)
        import ctypes as C
        from luminair_amd.backend import LmnFriCommitResult
        L, res = ctx.lib.lib, LmnFriCommitResult()
        arr = (C.c_void_p * 1)(a6.handle)
        assert L.lmn_col_fri_commit(ctx.handle, arr, 1, None, C.byref(res)) == ERR_INVALID_ARGUMENT
        assert L.lmn_col_fri_commit(ctx.handle, arr, 1, (C.c_uint8 * 32)(), None) == ERR_INVALID_ARGUMENT
        assert L.lmn_col_fri_commit(None, arr, 1, (C.c_uint8 * 32)(), C.byref(res)) == ERR_INVALID_ARGUMENT
        assert L.lmn_col_fri_commit(ctx.handle, None, 1, (C.c_uint8 * 32)(), C.byref(res)) == ERR_INVALID_ARGUMENT
        assert res.n_trees == 0 and not res.roots and not res.values and not res.levels
        # a first line layer exactly the last layer, and a column that joins exactly the last layer, are accepted
        got = ctx.fri_commit([a3], digest)
        assert got.layer_logs == [2] and len(got.roots) == 1
        got = ctx.fri_commit([a6, a3], digest)
        assert got.layer_logs == [5, 4, 3, 2] and got.layer_forms[-1] == LAUNCH
    finally:
        for h in (v2, a6, a5, a3, a2, t6, b2):
            h.free()
    check_case(ctxs, case)


def check_sharded_context_refused(ctxs):
    """a context with a shard set refuses the call and works again once the shard is cleared"""
    from luminair_amd.backend import ERR_INVALID_ARGUMENT, LuminairBackendError
    case = _c("after the shard is cleared", [5])
    ctx = ctxs.get(case)
    h = ctx.col_from_cpu(np.zeros((4, 32), dtype=U32))
    ctx.set_shard(0, 1, lambda *a: None)
    try:
        try:
            ctx.fri_commit([h], bytes(32))
        except LuminairBackendError as e:
            assert e.code == ERR_INVALID_ARGUMENT and "fri_commit" in str(e) and "shard" in str(e), (e.code, str(e))
        else:
            raise AssertionError("a sharded context accepted fri_commit")
    finally:
        ctx.clear_shard()
        h.free()
    check_case(ctxs, case)


# ----------------------------------------------------------------------------- the searcher's inputs
def search_roots(name):
    """the roots tools/find_redraw.cpp is given: all of them for constant columns (no alpha moves them), the first tree's
    for random ones"""
    from oracle.channel import ProtocolVariant
    case = next(c for c in REDRAW_CASES if c.search == name)
    cols, _, _ = case_columns(case)
    ref = ref_commit(cols, bytes(32), ProtocolVariant.DRAW_CTR_U32 if case.u32 else ProtocolVariant.KAT, case.last_log)
    return [r.hex() for r in (ref.roots if case.cls in ("zero", "const") else ref.roots[:1])]


def search_command(s, threads=8, seed=1):
    return 'tools/bin/find_redraw chain "%s" %d %s %s %s %d %d %d %d %s' % (
        s["name"], 37 if s["u32"] else 64, s["event"], ",".join(str(t) for t in s["layers"]), s["value"], s["lo"], s["hi"], threads,
        seed, " ".join(search_roots(s["name"])))


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:2] == ["roots"] and len(sys.argv) == 3:
        print(" ".join(search_roots(sys.argv[2])))
    elif sys.argv[1:] == ["commands"]:
        for s_ in REDRAW_SEARCHES:
            print(search_command(s_))
    else:
        sys.exit("usage: fri_checks.py roots <search name> | commands")
