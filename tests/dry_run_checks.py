"""Cases and references of the device dry run (`lmn_eval_*`, `lmn_tensor_range`, `DeviceGraph.dry_run_device`), run on the
emulation build (tests/test_dry_run_emu.py) and on the HIP libraries (tests/test_gpu_dry_run.py).

Two references:
 - plain Python integers, restated here: the Fixed<12> rules of include/luminair_hip.h (`py_value`, `py_reduce`) and the
   range by `min()` / `max()`;
 - the existing trace producers: for the same operands `lmn_eval_*`'s output equals `lmn_trace_*`'s out_dev word for word,
   and the refused count equals the number of rows whose output-value column holds the non-canonical word P.
Up to 2^8 elements both are asserted, above that the trace producer and numpy int64.

Every call writes into an arena filled with 0xA5 bytes: the output, the two range words and the counter lie between guard
words that must not change, and the counter starts at 0xA5A5A5A5 (a call adds to it and never resets it)."""
import math

import numpy as np

import trace_checks as tc
from luminair_amd import backend

P, S, R = tc.P, tc.S, tc.R
ADD, MUL, RECIP, SIN, SUM, MAX, SQRT, REM, EXP2, LOG2, LT, INPUTS, CONTIG = 0, 1, 2, 3, 5, 6, 7, 8, 9, 11, 13, 15, 16
ELEMENTWISE = (ADD, MUL, REM, LT, RECIP, SQRT, CONTIG, INPUTS)
BINARY = (ADD, MUL, REM, LT)
OUT_COL = {ADD: 11, MUL: 11, REM: 11, LT: 11, RECIP: 8, SQRT: 8, CONTIG: 8, INPUTS: 5, SUM: 8, MAX: 8}
COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000, (1 << 16) + 3)
FILL = 0xA5A5A5A5
GUARD = 64          # words
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
LUT_RANGES = [(-100, -50), (0, 10), (200, 210)]


def fits(v):
    return -R <= v <= R


def py_value(kind, a, b=0):
    """(output value, accepted) of one element: the contract of include/luminair_hip.h in Python integers"""
    if kind == ADD:
        ok = fits(a) and fits(b) and fits(a + b)
        return (a + b if ok else 0), ok
    if kind == MUL:
        o = (a * b) // S
        ok = fits(a) and fits(b) and fits(o)
        return (o if ok else 0), ok
    if kind == REM:
        ok = 0 <= a <= R and 0 < b <= R
        return (a % b if ok else 0), ok
    if kind == LT:
        ok = fits(a) and fits(b)
        return (S if ok and a < b else 0), ok
    if kind == RECIP:
        ok = 0 < a <= R
        return (S * S // a if ok else 0), ok
    if kind == SQRT:
        ok = 0 <= a <= R
        return (math.isqrt(a * S) if ok else 0), ok
    ok = fits(a)                     # Contiguous, Inputs
    return (a if ok else 0), ok


def py_reduce(groups, maximum):
    """(outputs, refused) of a reduction: an input outside the range is refused where it stands, the last step also
    when the group result is outside it - and only then 0 is written; running sums may leave the range"""
    outs, refused = [], 0
    for xs in groups:
        xs = [int(v) for v in xs]
        res = max(xs) if maximum else sum(xs)
        refused += sum(1 for v in xs[:-1] if not fits(v))
        ok = fits(xs[-1]) and fits(res)
        refused += 0 if ok else 1
        outs.append(res if ok else 0)
    return outs, refused


def positions(n):
    """element 0, element n - 1, the last lane of the first wave, the first lane of the last workgroup"""
    return [0, n - 1, min(63, n - 1), (n - 1) // 256 * 256]


# per kind: operands whose outputs are (in between, the smallest, the largest); +-(2^30-1) where the kind reaches them
EXTREMES = {ADD: ((5, 7), (-R, 0), (R, 0)), MUL: ((3 * S, 2 * S), (-R, S), (R, S)), REM: ((7, 5), (5, 5), (R - 1, R)),
            LT: ((1, 2), (2, 1), (1, 2)), RECIP: ((S, 0), (R, 0), (1, 0)), SQRT: ((S, 0), (0, 0), (R, 0)),
            CONTIG: ((3, 0), (-R, 0), (R, 0)), INPUTS: ((3, 0), (-R, 0), (R, 0))}


class Arena:
    """out[0 .. n), two range words and a counter between guards, everything 0xA5 before the call"""

    def __init__(self, ctx, n, counter=None):
        self.ctx, self.n = ctx, n
        self.o_out = GUARD
        self.o_mm = GUARD + n + GUARD + (n & 1)          # even: the two words are one 8-byte slot
        self.o_ctr = self.o_mm + 2 + GUARD
        self.words = self.o_ctr + 1 + GUARD
        self.buf = ctx.upload(np.full(self.words, FILL, dtype=np.uint32))
        self.out = self.buf.view(self.o_out * 4, n * 4)
        self.minmax = self.buf.view(self.o_mm * 4, 8)
        self.own_counter = counter is None
        self.counter = self.buf.view(self.o_ctr * 4, 4) if counter is None else counter

    def result(self, what):
        """(out int64[n], (min, max), counter word) after the guards were checked; frees the arena"""
        w = self.ctx.download(self.buf)
        self.buf.free()
        keep = np.ones(self.words, dtype=bool)
        keep[self.o_out:self.o_out + self.n] = False
        keep[self.o_mm:self.o_mm + 2] = False
        if self.own_counter:
            keep[self.o_ctr] = False
        assert np.all(w[keep] == FILL), "%s: %d words outside out / range / counter changed" % (what, int((w[keep] != FILL).sum()))
        out = w[self.o_out:self.o_out + self.n].view(np.int32).astype(np.int64)
        mm = w[self.o_mm:self.o_mm + 2].view(np.int32)
        return out, (int(mm[0]), int(mm[1])), int(w[self.o_ctr])


def _i32(v):
    return np.asarray(v, dtype=np.int64).astype(np.int32)


def check_eval(ctx, kind, lhs, rhs=None, lhs_view=None, rhs_view=None, n=None, what="", elems=None):
    """one lmn_eval_elementwise_v call against both references.  lhs / rhs: the operand BUFFERS; elems: the element
    values (a, b) in output order when views are used.  Returns (out, refused)."""
    n = n if n is not None else len(lhs)
    what = "kind %d n=%d %s" % (kind, n, what)
    if kind not in BINARY:
        rhs = rhs_view = None
    dl = ctx.upload(_i32(lhs))
    dr = ctx.upload(_i32(rhs)) if rhs is not None else None
    ar = Arena(ctx, n)
    ctx.eval_elementwise(kind, dl, dr, n, lhs_view=lhs_view, rhs_view=rhs_view, out=ar.out, minmax=ar.minmax,
                         refused=ar.counter)
    out, mm, ctr = ar.result(what)
    refused = (ctr - FILL) % 2 ** 32
    for b in (dl, dr):
        if b is not None:
            b.free()
    # the trace producer on the same operands
    rows, t_out, _ = tc._run(ctx, kind, list(lhs), list(rhs) if rhs is not None else None, lhs_view=lhs_view,
                             rhs_view=rhs_view, n=n)
    assert np.array_equal(out, t_out), "%s: output differs from the trace producer's out_dev" % what
    assert refused == int((rows[:, OUT_COL[kind]] == P).sum()), "%s: refused count %d" % (what, refused)
    assert mm == (int(t_out.min()), int(t_out.max())), "%s: range %r, numpy %r" % (what, mm, (t_out.min(), t_out.max()))
    if n <= 256:
        if elems is None:
            elems = list(zip(lhs, rhs)) if rhs is not None else [(a, 0) for a in lhs]
        want = [py_value(kind, int(a), int(b)) for a, b in elems]
        assert [int(v) for v in out] == [o for o, _ in want], "%s: output differs from the Python integers" % what
        assert refused == sum(1 for _, ok in want if not ok), what
        assert mm == (min(o for o, _ in want), max(o for o, _ in want)), what
    return out, refused, mm


def check_counts(ctx, kind):
    """every element count, the smallest and the largest output placed at each of the four positions in turn"""
    base, lo, hi = EXTREMES[kind]
    for n in COUNTS:
        pos = positions(n)
        for i, p in enumerate(pos):
            ops = [base] * n
            q = pos[(i + 1) % 4]
            if q != p:
                ops[q] = hi
            ops[p] = lo
            out, refused, mm = check_eval(ctx, kind, [a for a, _ in ops], [b for _, b in ops],
                                          what="min at %d max at %d" % (p, q))
            assert refused == 0 and mm[0] == py_value(kind, *lo)[0], (kind, n, p, mm)
            if q != p:
                assert mm[1] == py_value(kind, *hi)[0], (kind, n, q, mm)


def check_range_cases(ctx, n=257):
    """all-equal, all-negative, +-(2^30-1), min = max = 0 - through Add, Contiguous, Inputs and lmn_tensor_range"""
    cases = {"all-equal": [7] * n, "all-negative": [-5 - (i % 11) for i in range(n)], "extremes": [R, -R] + [0] * (n - 2),
             "zeros": [0] * n}
    for name, vals in cases.items():
        for kind in (ADD, CONTIG, INPUTS):
            _, _, mm = check_eval(ctx, kind, vals, [0] * n, what=name)
            assert mm == (min(vals), max(vals)), (name, kind, mm)
        assert tensor_range(ctx, vals, name) == (min(vals), max(vals)), name


def tensor_range(ctx, vals, what=""):
    d = ctx.upload(_i32(vals))
    ar = Arena(ctx, 0)
    ctx.tensor_range(d, len(vals), ar.minmax)
    _, mm, ctr = ar.result("tensor_range " + what)
    d.free()
    assert ctr == FILL
    return mm


def check_tensor_range_counts(ctx):
    """raw buffers (no contract): the int32 extremes at each position"""
    for n in COUNTS:
        pos = positions(n)
        for i, p in enumerate(pos):
            vals = [3] * n
            q = pos[(i + 1) % 4]
            if q != p:
                vals[q] = INT32_MAX
            vals[p] = INT32_MIN
            assert tensor_range(ctx, vals, "n=%d" % n) == (min(vals), max(vals)), (n, p, q)
        assert tensor_range(ctx, [-9] * n) == (-9, -9)


# ---- views
def view_cases(n):
    """(name, buffer size, shape, strides, offset): a stride-0 expanded dimension, a slice with an offset, a permutation"""
    if n == 1000:
        return [("expanded", 100 + 4, (10, 100), (0, 1), 4), ("slice", 20 * 60, (20, 50), (60, 1), 5),
                ("permuted", 1000, (50, 20), (1, 50), 0)]
    assert n == 257
    return [("expanded", 9, (257,), (0,), 3), ("slice", 2 * 257 + 3, (257,), (2,), 3), ("permuted", 257, (257, 1), (1, 257), 0)]


def operand_values(kind, rng, m):
    """m in-contract operand pairs of one kind, negative values where the kind takes them"""
    if kind in (REM, RECIP, SQRT):
        return rng.integers(1, 1 << 20, size=m), rng.integers(1, 1 << 20, size=m)
    return rng.integers(-(1 << 20), 1 << 20, size=m), rng.integers(-(1 << 20), 1 << 20, size=m)


def check_views(ctx, kind):
    rng = np.random.default_rng(100 + kind)
    for n in (257, 1000):
        for name, size, shape, strides, offset in view_cases(n):
            a, b = operand_values(kind, rng, size)
            full, _ = operand_values(kind, rng, n)
            idx = tc.view_index(shape, strides, offset)
            v = backend.LmnView.make(shape, strides, offset)
            # the view on the left operand, then on the right one (binary kinds)
            check_eval(ctx, kind, a, full if kind in BINARY else None, lhs_view=v, n=n, what="lhs " + name,
                       elems=list(zip(a[idx], full)))
            if kind in BINARY:
                check_eval(ctx, kind, full, b, rhs_view=v, n=n, what="rhs " + name, elems=list(zip(full, b[idx])))


# ---- refusals
REFUSED_OPERANDS = {RECIP: [(0, 0), (-5, 0)], SQRT: [(-1, 0)], REM: [(-7, 3), (7, 0)], ADD: [(R, R)], MUL: [(R, 2 * S)],
                    CONTIG: [(R + 1, 0)], INPUTS: [(-R - 1, 0)], LT: [(R + 1, 0)]}
ACCEPTED_POSITIVE = {RECIP: (S, 0), SQRT: (S, 0), REM: (7, 5), ADD: (5, 7), MUL: (3 * S, 2 * S), CONTIG: (3, 0), INPUTS: (3, 0),
                     LT: (1, 2)}


def check_refusals(ctx, kind, n=1000):
    """refused elements at the four positions, one workgroup refused entirely, none refused: the counter, the zeros in
    the output, and 0 taking part in the range (every accepted output here is positive)"""
    good = ACCEPTED_POSITIVE[kind]
    assert py_value(kind, *good)[0] > 0
    for bad in REFUSED_OPERANDS[kind]:
        assert not py_value(kind, *bad)[1]
        for name, where in (("positions", positions(n)), ("workgroup 1", list(range(256, 512))), ("none", [])):
            ops = [good] * n
            for p in where:
                ops[p] = bad
            out, refused, mm = check_eval(ctx, kind, [a for a, _ in ops], [b for _, b in ops], what="refused: " + name)
            assert refused == len(set(where)), (kind, name, refused)
            assert all(out[p] == 0 for p in where) and int((out == 0).sum()) == len(set(where))
            assert mm == ((0 if where else py_value(kind, *good)[0]), py_value(kind, *good)[0]), (kind, name, mm)


def check_counter_accumulates(ctx):
    """two calls on one counter: it is never reset"""
    ctr = ctx.upload(np.array([FILL], dtype=np.uint32))
    for vals, k in (([0, 5, 0, 7, -1], 3), ([4, 0, 9], 1)):
        d = ctx.upload(_i32(vals))
        ar = Arena(ctx, len(vals), counter=ctr)
        ctx.eval_elementwise(RECIP, d, None, len(vals), out=ar.out, minmax=ar.minmax, refused=ar.counter)
        out, _, _ = ar.result("accumulate")
        assert int((out == 0).sum()) == k
        d.free()
    assert int(ctx.download(ctr)[0]) == (FILL + 4) % 2 ** 32
    # NULL range words and NULL counter are accepted
    d = ctx.upload(_i32([0, 4096]))
    o = ctx.eval_elementwise(RECIP, d, None, 2)
    assert list(ctx.download(o, np.int32)) == [0, 4096]
    for b in (d, o, ctr):
        b.free()


# ---- LUT ops
def lut_signed(w):
    return int(w) - P if int(w) > P // 2 else int(w)


def check_eval_lut(ctx, kind, name, inputs, ranges, col1, view=None, n=None, what="", elems=None):
    n = n if n is not None else len(inputs)
    what = "%s n=%d %s" % (name, n, what)
    d, dc = ctx.upload(_i32(inputs)), ctx.upload(col1)
    ar = Arena(ctx, n)
    ctx.eval_lut(kind, d, n, dc, ranges, view=view, out=ar.out, minmax=ar.minmax, refused=ar.counter)
    out, mm, ctr = ar.result(what)
    refused = (ctr - FILL) % 2 ** 32
    elems = [int(v) for v in (inputs if elems is None else elems)]
    base, index = 0, {}
    for lo, hi in ranges:                      # LookupLayout::find_index
        for v in range(lo, hi + 1):
            index[v] = base + v - lo
        base += hi - lo + 1
    want = np.array([lut_signed(col1[index[v]]) if v in index else 0 for v in elems], dtype=np.int64)
    assert np.array_equal(out, want), "%s: output differs from the LUT column" % what
    assert refused == sum(1 for v in elems if v not in index), what
    assert mm == (int(want.min()), int(want.max())), (what, mm)
    if refused == 0:                           # inside the ranges the trace producer is a second reference
        info = dict(node_id=2, input_id=0, num_consumers=1)
        mult = ctx.upload(np.zeros(len(col1), dtype=np.uint32))
        rb, ob = ctx.trace_lut(kind, d, n, lut_col1=dc, mult=mult, view=view, ranges=ranges, **info)
        assert np.array_equal(ctx.download(ob, np.int32).astype(np.int64), out), "%s: trace producer" % what
        for b in (mult, rb, ob):
            b.free()
    d.free()
    dc.free()
    return refused, mm


def check_lut_counts(ctx):
    lib = ctx.lib
    col0, col1 = lib.lut_from_ranges("sin", LUT_RANGES)
    valid = [v for lo, hi in LUT_RANGES for v in range(lo, hi + 1)]
    outs = {v: lut_signed(col1[i]) for i, v in enumerate(valid)}
    lo_in, hi_in = min(valid, key=outs.get), max(valid, key=outs.get)
    base = next(v for v in valid if outs[lo_in] < outs[v] < outs[hi_in])
    for n in COUNTS:
        pos = positions(n)
        for i, p in enumerate(pos):
            vals = [base] * n
            q = pos[(i + 1) % 4]
            if q != p:
                vals[q] = hi_in
            vals[p] = lo_in
            refused, mm = check_eval_lut(ctx, SIN, "sin", vals, LUT_RANGES, col1, what="min at %d" % p)
            assert refused == 0 and mm[0] == outs[lo_in] and (q == p or mm[1] == outs[hi_in])
    # below, between and above the ranges: counted, 0 written, no error return
    vals = [base] * 1000
    for p, v in zip(positions(1000), (-101, 11, 211, 199)):
        vals[p] = v
    refused, mm = check_eval_lut(ctx, SIN, "sin", vals, LUT_RANGES, col1, what="outside the ranges")
    assert refused == 4 and mm[0] <= 0 <= mm[1]
    # views, and the two other functions over one range
    rng = np.random.default_rng(5)
    for n in (257, 1000):
        for name, size, shape, strides, offset in view_cases(n):
            buf = rng.choice(valid, size=size)
            idx = tc.view_index(shape, strides, offset)
            check_eval_lut(ctx, SIN, "sin", buf, LUT_RANGES, col1, view=backend.LmnView.make(shape, strides, offset), n=n,
                           what=name, elems=buf[idx])
    for kind, name, rg in ((EXP2, "exp2", [(-300, 500)]), (LOG2, "log2", [(1, 900)])):
        c1 = lib.lut_from_ranges(name, rg)[1]
        check_eval_lut(ctx, kind, name, rng.integers(rg[0][0], rg[0][1] + 1, size=257), rg, c1)


# ---- reduce
REDUCE_SHAPES = [(1, 1, 1), (1, 5, 1), (3, 1, 4), (5, 64, 7), (2, 300, 3), (1, 1, 300), (4, 3, 1000), (1, 70000, 1)]


def check_reduce(ctx, t, maximum, what=""):
    """t: (front, dim, back) int64 against the trace producer, and against Python integers up to 2^8 elements"""
    front, dim, back = t.shape
    what = "%s (%d, %d, %d) %s" % ("max" if maximum else "sum", front, dim, back, what)
    d = ctx.upload(_i32(t.reshape(-1)))
    ar = Arena(ctx, front * back)
    ctx.eval_reduce(d, front, dim, back, maximum=maximum, out=ar.out, minmax=ar.minmax, refused=ar.counter)
    out, mm, ctr = ar.result(what)
    refused = (ctr - FILL) % 2 ** 32
    rb, ob = ctx.trace_sum_reduce(d, front, dim, back, node_id=21, input_id=20, num_consumers=1, maximum=maximum)
    rows = ctx.download(rb).reshape(-1, tc.NCOLS[MAX if maximum else SUM])
    t_out = ctx.download(ob, np.int32).astype(np.int64)
    for b in (d, rb, ob):
        b.free()
    assert np.array_equal(out, t_out), "%s: output differs from the trace producer's" % what
    assert refused == int((rows[:, OUT_COL[SUM]] == P).sum()), "%s: refused %d" % (what, refused)
    assert mm == (int(t_out.min()), int(t_out.max())), (what, mm)
    if t.size <= 256:
        want, want_refused = py_reduce(t.transpose(0, 2, 1).reshape(front * back, dim).tolist(), maximum)
        assert [int(v) for v in out] == want and refused == want_refused, what
        assert mm == (min(want), max(want)), what
    return out, refused


def check_reduce_shape(ctx, shape, maximum):
    front, dim, back = shape
    rng = np.random.default_rng(front * 1000003 + dim * 1009 + back)
    t = rng.integers(-(1 << 20), 1 << 20, size=shape).astype(np.int64)
    _, refused = check_reduce(ctx, t, maximum, "random")
    assert refused == 0
    # running sums that pass +-P while the results stay inside the range (accepted); with more than two groups one
    # result outside it and one input outside it (refused and counted)
    g = tc.wrapping_groups(rng, front * back, dim)
    t = g.reshape(front, back, dim).transpose(0, 2, 1).copy()
    out, refused = check_reduce(ctx, t, maximum, "wrapping")
    marked = front * back > 2 and dim > 1
    if not maximum:
        assert (refused >= 2 and out[1] == 0) if marked else refused == 0, (shape, refused)
    if dim >= 2 and not maximum:
        # the whole first half at +R, the second at -R: the running sum reaches dim/2 * (2^30-1), the result is 0 or R
        t = np.empty(shape, dtype=np.int64)
        t[:, :dim // 2, :] = R
        t[:, dim // 2:, :] = -R
        out, refused = check_reduce(ctx, t, False, "half +R half -R")
        assert refused == 0 and set(int(v) for v in out) == {-R if dim % 2 else 0}
        t[:, dim // 2:, :] = R                          # every result outside the range: refused, 0 written
        out, refused = check_reduce(ctx, t, False, "all +R")
        assert refused == front * back and not out.any()


def check_reduce_split(lib):
    """the issue's shapes lie on both sides of the host's split, and the split only depends on `back` growing"""
    split = {s: lib.eval_reduce_split(s[1], s[2]) for s in REDUCE_SHAPES}
    assert set(split.values()) == {0, 1}, split
    for a in REDUCE_SHAPES:
        for b in REDUCE_SHAPES:
            if a[2] <= b[2]:
                # one lane per output element needs `back` consecutive words per step: more of them never hurts
                assert not (split[a] == 0 and split[b] == 1), ("lane-per-output at back=%d but wave-per-group at back=%d"
                                                               % (a[2], b[2]))
    assert any(split[s] == 1 and s[1] > 256 for s in REDUCE_SHAPES)          # a group longer than a workgroup, by one wave
    for mapping in (0, 1):
        assert any(split[s] == mapping and s[0] * s[2] > 256 for s in REDUCE_SHAPES) or mapping == 1   # several workgroups
        assert any(split[s] == mapping and s[1] > 1 for s in REDUCE_SHAPES)
    return split


# ---- argument refusals
def check_argument_refusals(ctx):
    a = ctx.upload(_i32(range(12)))
    col = ctx.upload(np.zeros(16, dtype=np.uint32))
    out = ctx.alloc(64)

    def refused(names, fn):
        try:
            fn()
        except backend.LuminairBackendError as e:
            assert e.code == backend.ERR_INVALID_ARGUMENT, e
            assert any(nm in str(e) for nm in names), "the text %r names none of %r" % (str(e), names)
            return
        raise AssertionError("accepted: %r" % (names,))
    v = backend.LmnView.make
    refused(["lhs_dev"], lambda: ctx.eval_elementwise(ADD, None, a, 12, out=out))
    refused(["rhs_dev"], lambda: ctx.eval_elementwise(ADD, a, None, 12, out=out))
    refused(["out_dev"], lambda: ctx.eval_elementwise(ADD, a, a, 12, out=backend.DeviceBuffer(ctx, 0, 48, owned=False)))
    refused(["n is 0", " n "], lambda: ctx.eval_elementwise(ADD, a, a, 0, out=out))
    refused(["lhs_view"], lambda: ctx.eval_elementwise(ADD, a, a, 12, lhs_view=v((3, 5), (5, 1)), out=out))
    refused(["rhs_view"], lambda: ctx.eval_elementwise(ADD, a, a, 12, rhs_view=v((3, 5), (5, 1)), out=out))
    refused(["kind"], lambda: ctx.eval_elementwise(SIN, a, a, 12, out=out))
    refused(["input_dev"], lambda: ctx.eval_reduce(None, 1, 12, 1, out=out))
    refused(["dim"], lambda: ctx.eval_reduce(a, 1, 0, 12, out=out))
    refused(["front"], lambda: ctx.eval_reduce(a, 0, 12, 1, out=out))
    refused(["back"], lambda: ctx.eval_reduce(a, 12, 1, 0, out=out))
    refused(["input_dev"], lambda: ctx.eval_lut(SIN, None, 12, col, [(0, 15)], out=out))
    refused(["lut_col1_dev"], lambda: ctx.eval_lut(SIN, a, 12, None, [(0, 15)], out=out))
    refused(["n_ranges"], lambda: ctx.eval_lut(SIN, a, 12, col, [(20 * k, 20 * k + 1) for k in range(17)], out=out))
    refused(["n_ranges"], lambda: ctx.eval_lut(SIN, a, 12, col, [], out=out))
    refused(["ranges"], lambda: ctx.eval_lut(SIN, a, 12, col, [(5, 9), (0, 3)], out=out))
    refused(["view"], lambda: ctx.eval_lut(SIN, a, 12, col, [(0, 15)], view=v((5,), (1,)), out=out))
    refused(["n is 0"], lambda: ctx.eval_lut(SIN, a, 0, col, [(0, 15)], out=out))
    refused(["kind"], lambda: ctx.eval_lut(ADD, a, 12, col, [(0, 15)], out=out))
    refused(["buf_dev"], lambda: ctx.tensor_range(None, 12, out))
    refused(["minmax_dev"], lambda: ctx.tensor_range(a, 12, backend.DeviceBuffer(ctx, 0, 8, owned=False)))
    refused(["n is 0"], lambda: ctx.tensor_range(a, 0, out))
    # the context is usable afterwards
    o = ctx.eval_elementwise(ADD, a, a, 12, out=out)
    assert list(ctx.download(o.view(0, 48), np.int32)) == [2 * i for i in range(12)]
    for b in (a, col, out):
        b.free()


# ---- graph level
def py_padded_range(name, lo, hi):
    """the rule of gen_circuit_settings: 10 % of the span, round to nearest, log2 clipped at 1"""
    lo_f, hi_f = lo / 4096.0, hi / 4096.0
    delta = (hi_f - lo_f) * 0.10
    rnd = lambda x: int(math.floor(abs(x) * 4096.0 + 0.5)) * (1 if x >= 0 else -1)
    lo, hi = rnd(lo_f - delta), rnd(hi_f + delta)
    return (max(lo, 1) if name == "log2" else lo), hi


def py_graph(g, lib):
    """exact node values in Python integers, LUT outputs read from lmn_lut_from_ranges columns of each node's own padded
    range; -> ({node id: [values]}, {lut name: coalesced ranges}, whether a LessThan node exists)"""
    vals, per_fn = {}, {"sin": [], "exp2": [], "log2": []}
    names = {SIN: "sin", EXP2: "exp2", LOG2: "log2"}

    def view(v):
        base = vals[v.base.node_id]
        return [base[i] for i in tc.view_index(v.shape, v.strides, v.offset)]
    for n in g.nodes:
        k = n.kind
        if k == INPUTS:
            out = [py_value(INPUTS, int(x))[0] for x in n.host.reshape(-1)]
        elif k in BINARY:
            out = [py_value(k, a, b)[0] for a, b in zip(view(n.inputs[0]), view(n.inputs[1]))]
        elif k in (RECIP, SQRT, CONTIG):
            out = [py_value(k, a)[0] for a in view(n.inputs[0])]
        elif k in (SUM, MAX):
            a = n.inputs[0].base
            x = np.moveaxis(np.array(vals[a.node_id], dtype=object).reshape(a.shape), n.axis, -1).reshape(-1, a.shape[n.axis])
            out, _ = py_reduce(x.tolist(), k == MAX)
        else:
            name = names[k]
            buf = vals[n.inputs[0].base.node_id]               # the BUFFER, not the view
            lo, hi = py_padded_range(name, min(buf), max(buf))
            per_fn[name].append((lo, hi))
            col1 = lib.lut_from_ranges(name, [(lo, hi)])[1]
            out = [lut_signed(col1[a - lo]) for a in view(n.inputs[0])]
        vals[n.out.node_id] = [int(v) for v in out]
    ranges = {}
    for name, rg in per_fn.items():
        if rg:
            rg = sorted(rg)
            merged = [list(rg[0])]
            for lo, hi in rg[1:]:
                if lo <= merged[-1][1] + 1:
                    merged[-1][1] = max(merged[-1][1], hi)
                else:
                    merged.append([lo, hi])
            ranges[name] = [tuple(r) for r in merged]
    return vals, ranges, any(n.kind == LT for n in g.nodes)


def settings_ranges(settings):
    return {name: [tuple(r) for r in lk.layout.ranges] for name, lk in (settings.layouts or {}).items()}


def check_graph_settings(ctx, g, what, host_agrees=True):
    """gen_circuit_settings(device=True) == the Python restatement; every dry-run tensor == its exact values; and ==
    the host path where numpy's rounding agrees with the LUT columns"""
    vals, ranges, has_lt = py_graph(g, ctx.lib)
    settings = g.gen_circuit_settings(device=True)
    assert settings_ranges(settings) == ranges, (what, settings_ranges(settings), ranges)
    assert (settings.range_check is not None) == has_lt, what
    for n in g.nodes:
        assert [int(v) for v in g.read(n.out).reshape(-1)] == vals[n.out.node_id], "%s: node %d" % (what, n.out.node_id)
    g.release_dry_run()
    assert all(n.out.buf is None for n in g.nodes)
    host = g.gen_circuit_settings()
    if host_agrees:
        assert settings_ranges(host) == ranges and (host.range_check is not None) == has_lt, what
    return settings, host


def mirror_graph(ctx):
    """the graph of test_gen_circuit_settings_mirror (tests/test_producer_scenarios.py), seed 3"""
    from luminair_amd.graph import DeviceGraph
    rng = np.random.default_rng(3)
    g = DeviceGraph(ctx)
    x = g.input(rng.integers(-900, -600, size=(3, 4)))
    y = g.input(rng.integers(700, 950, size=(3, 4)))
    e = g.exp2(g.add(g.sin(x), g.sin(y)))
    out = g.output(g.less_than(e, g.input(rng.integers(0, 8192, size=(3, 4)))))
    return g, out


def check_scenario_graphs(lib, device=0):
    """every graph of tests/producer_scenarios.py (seed 11, as test_producer_scenarios.py runs them) and the mirror
    graph (seed 3): on these inputs numpy's rounding of the host formula agrees with the LUT columns - checked on the
    emulation build - so the host path's settings are asserted equal too"""
    import producer_scenarios as ps
    from luminair_amd.graph import DeviceGraph
    cfg = lib.default_config()
    cfg.protocol_variant = backend.VARIANT_PINNED
    ctx = backend.Context(device, cfg, lib)
    try:
        for build in ps.EXPANSIONS + ps.OPS:
            g = DeviceGraph(ctx)
            for o in build(g, np.random.default_rng(11)):
                g.output(o)
            check_graph_settings(ctx, g, build.__name__)
        check_graph_settings(ctx, mirror_graph(ctx)[0], "mirror")
    finally:
        ctx.close()


def check_view_not_buffer(ctx):
    """a LUT node that reads a slice: its range comes from the whole source buffer, as `buffer.min_max()` does"""
    from luminair_amd.graph import DeviceGraph
    g = DeviceGraph(ctx)
    x = g.input(np.array([[-3000, 10, 20, 30], [40, 50, 60, 5000]]))
    g.output(g.sin(g.slice(x, (None, (1, 3)))))
    settings, _ = check_graph_settings(ctx, g, "slice of a wider buffer")
    assert settings_ranges(settings)["sin"] == [py_padded_range("sin", -3000, 5000)]


def check_tie_graph(ctx):
    """exp2 at -13.0: the host formula computes 2^-13 * 4096 = 0.5 exactly and numpy rounds the tie to 0, the LUT
    generator's column holds 1.  The device dry run reads the column, so the next LUT node's range starts from 1."""
    from luminair_amd.graph import DeviceGraph
    g = DeviceGraph(ctx)
    x = g.input(np.array([-13 * S, 0, S]))
    e = g.exp2(x)
    g.output(g.sin(e))
    col1 = ctx.lib.lut_from_ranges("exp2", [py_padded_range("exp2", -13 * S, S)])[1]
    assert lut_signed(col1[-13 * S - py_padded_range("exp2", -13 * S, S)[0]]) == 1      # the generator's rounding
    assert np.rint(np.exp2(-13.0) * S) == 0                                             # numpy's
    vals, ranges, _ = py_graph(g, ctx.lib)
    assert vals[e.node_id] == [1, S, 2 * S]
    settings, host = check_graph_settings(ctx, g, "tie", host_agrees=False)
    assert settings_ranges(settings)["sin"] == [py_padded_range("sin", 1, 2 * S)]
    assert settings_ranges(host)["sin"] == [py_padded_range("sin", 0, 2 * S)] != settings_ranges(settings)["sin"]


def check_full_mirror(lib, device=0):
    """device settings -> gen_trace -> fill_multiplicities -> prove -> verify; the proof's bytes equal the proof made
    with host-derived settings; every dry-run tensor equals the tensor gen_trace leaves"""
    import luminair_amd
    cfg = lib.default_config()
    cfg.protocol_variant = backend.VARIANT_PINNED
    ctx = backend.Context(device, cfg, lib)
    try:
        proofs = []
        for on_device in (True, False):
            g, out = mirror_graph(ctx)
            settings = g.gen_circuit_settings(device=on_device)
            dry = {n.out.node_id: g.read(n.out).copy() for n in g.nodes} if on_device else None
            tables, luts, bufs = g.gen_trace()
            assert not g._dry_bufs
            if dry is not None:
                for n in g.nodes:
                    assert np.array_equal(g.read(n.out), dry[n.out.node_id]), "node %d" % n.out.node_id
            g.fill_multiplicities(settings, tables)
            proof = ctx.prove_tables(tables, settings.lut_columns(lib))
            luminair_amd.verify(luminair_amd.LuminairProof(proof), settings, backend.VARIANT_PINNED, library=lib)
            proofs.append((proof, settings.to_bincode()))
            for b in bufs:
                b.free()
        assert proofs[0] == proofs[1], "proof or settings differ between the device and the host dry run"
    finally:
        ctx.close()


def check_refused_graph(ctx):
    """a Recip of 0 (twice) raises with the count; the context takes the next graph"""
    from luminair_amd.graph import DeviceGraph
    g = DeviceGraph(ctx)
    g.output(g.exp2(g.recip(g.input(np.array([4096, 0, 8192, 0])))))
    try:
        g.gen_circuit_settings(device=True)
    except ValueError as e:
        assert "2 elements refused" in str(e), e
    else:
        raise AssertionError("a Recip of 0 was accepted")
    assert not g._dry_bufs
    check_graph_settings(ctx, mirror_graph(ctx)[0], "after a refused graph")


NEW_EXPORTS = ["lmn_eval_elementwise_v", "lmn_eval_reduce", "lmn_eval_reduce_split", "lmn_eval_lut_ranges", "lmn_tensor_range"]


def check_exports(lib):
    for name in NEW_EXPORTS:
        assert name in backend.EXPORTS
        getattr(lib.lib, name)
