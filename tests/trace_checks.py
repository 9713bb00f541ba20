"""Value and shape edges of the device trace producers (`lmn_trace_*`), run against the emulation build on CPU
(tests/test_trace_edges_emu.py) and the HIP library on GPU (tests/test_gpu_trace_edges.py, also through the batch
library's second compile of the kernels).

The reference is a plain restatement, in Python integers, of each kind's row layout and of the producers' contract
(include/luminair_hip.h, next to lmn_trace_elementwise): values in [-(2^30-1), 2^30-1], every row word the exact value
mod P, Recip input > 0, Sqrt input >= 0, Rem lhs >= 0 and rhs > 0; an element outside the contract carries the
non-canonical word P in its row's output-value column, zeros in the other derived words, and 0 in the output tensor.
It does not use luminair_amd/synthetic.py; `check_synthetic_agrees` checks synthetic.py against it inside the contract."""
import math

import numpy as np

P = (1 << 31) - 1
S = 4096
R = (1 << 30) - 1          # largest magnitude of a Fixed<12> value under the contract
MARK = P                   # the non-canonical word of a refused element

ADD, MUL, RECIP, SUM, MAX, SQRT, REM, LT, RC, INPUTS, CONTIG = 0, 1, 2, 5, 6, 7, 8, 13, 14, 15, 16
BINARY = (ADD, MUL, REM, LT)
NCOLS = {ADD: 15, MUL: 16, RECIP: 13, SQRT: 13, REM: 16, LT: 22, INPUTS: 7, CONTIG: 11, SUM: 14, MAX: 15}

# value edges: 0, +-1, the scale boundary, both ends of the range and just past them, the int32 extremes
EDGES = [0, 1, -1, 4095, -4095, 4096, -4096, 4097, -4097, R, -R, R + 1, -R - 1, 2 ** 31 - 1, -2 ** 31]
# Mul pairs around |lhs * rhs| = 2^30 * 4096 (out = +-R is the last value inside), negative operands (floor), and the
# issue's own cases
MUL_PAIRS = [(R, 4096), (R, 4097), (-R, 4096), (-R, 4097), (4096, -R), (1 << 21, (1 << 21) - 1), (1 << 21, 1 << 21),
             (-(1 << 21), 1 << 21), (-(1 << 21), (1 << 21) - 1), (-1, 1), (-5, 3), (-4097, 4096), (-4097, -4097),
             (-(1 << 22), 1 << 22), (3 << 20, 3 << 20), (1 << 30, 1 << 30)]
RECIP_VALUES = [1, 2, 4095, 4096, 4097, S * S, S * S + 1, R, 0, -1, -5000, -R, R + 1, -2 ** 31]
SQRT_VALUES = [0, 1, 4095, 4096, 4097, R, -1, -R, R + 1, -2 ** 31] + \
    [v for k in (1, 3, 100, 511) for v in (k * k * S - 1, k * k * S, k * k * S + 1)]   # v*4096 = (k*4096)^2 and +-4096
REM_PAIRS = [(0, 1), (1, 1), (5, 5), (3, 7), (7, 3), (R, 1), (R, R), (R - 1, R), (R, 4096), (4095, 4096), (4097, 4096),
             (-7, 3), (7, -3), (-7, -3), (7, 0), (0, 0), (-1, R), (R + 1, 3), (3, R + 1), (-2 ** 31, 5)]


def m31(v):
    return v % P


def fits(v):
    return -R <= v <= R


# ---- the value words of one element, per kind: (words, output value)
def v_add(a, b):
    o = a + b
    ok = fits(a) and fits(b) and fits(o)
    return [m31(a), m31(b), m31(o) if ok else MARK], o if ok else 0


def v_mul(a, b):
    prod = a * b
    o = prod // S                           # floor, also for negative products
    ok = fits(a) and fits(b) and fits(o)
    return [m31(a), m31(b), m31(o) if ok else MARK, prod - o * S if ok else 0], o if ok else 0


def v_rem(a, b):
    ok = 0 <= a <= R and 0 < b <= R
    q, r = divmod(a, b) if ok else (0, 0)
    return [m31(a), m31(b), r if ok else MARK, q], r


def v_lt(a, b):
    if not (fits(a) and fits(b)):
        return [m31(a), m31(b), MARK] + [0] * 6, 0
    lt = a < b
    diff = b - a + (0 if lt else P)
    return [m31(a), m31(b), S if lt else 0, m31(diff), 0 if lt else 1] + [diff >> (8 * k) & 255 for k in range(4)], \
        (S if lt else 0)


def v_recip(a):
    ok = 0 < a <= R
    o = S * S // a if ok else 0
    return [m31(a), o if ok else MARK, S * S - a * o if ok else 0, S], o


def v_sqrt(a):
    ok = 0 <= a <= R
    o = math.isqrt(a * S) if ok else 0
    return [m31(a), o if ok else MARK, a * S - o * o if ok else 0, S], o


def v_unary_copy(a):      # Contiguous (element-wise view rule): input word, output word
    ok = fits(a)
    return [m31(a), m31(a) if ok else MARK], a if ok else 0


def v_inputs(a):
    ok = fits(a)
    return [m31(a) if ok else MARK], a if ok else 0


VALUE = {ADD: v_add, MUL: v_mul, REM: v_rem, LT: v_lt, RECIP: v_recip, SQRT: v_sqrt, CONTIG: v_unary_copy,
         INPUTS: v_inputs}


def ref_elementwise(kind, lhs, rhs, node=2, ids=(0, 1), mults=(-1, -1), consumers=1, final=False):
    """(rows (n, ncols) uint32, out int64, range-check multiplicities[256] for LessThan) of one lmn_trace_elementwise
    call on the element values lhs / rhs (already read through their views)."""
    lhs = [int(v) for v in lhs]
    rhs = [int(v) for v in rhs] if kind in BINARY else [0] * len(lhs)
    n = len(lhs)
    om = 0 if final else m31(consumers)
    lm, rm = m31(mults[0]), m31(mults[1])
    cache, vals, outs = {}, [], []
    for ab in zip(lhs, rhs):
        if ab not in cache:
            cache[ab] = VALUE[kind](*ab) if kind in BINARY else VALUE[kind](ab[0])
        w, o = cache[ab]
        vals.append(w)
        outs.append(o)
    vals = np.array(vals, dtype=np.int64).reshape(n, -1)
    idx = np.arange(n, dtype=np.int64)
    last = (idx == n - 1).astype(np.int64)
    full = lambda v: np.full(n, v, dtype=np.int64)
    if kind == INPUTS:
        cols = [full(node), idx, last, full(node), idx + 1, vals[:, 0], full(om)]
    elif kind in BINARY:
        cols = [full(node), full(ids[0]), full(ids[1]), idx, last, full(node), full(ids[0]), full(ids[1]), idx + 1]
        cols += list(vals.T) + [full(lm), full(rm), full(om)] + ([full(1)] if kind == LT else [])
    else:
        cols = [full(node), full(ids[0]), idx, last, full(node), full(ids[0]), idx + 1] + list(vals.T) + [full(lm), full(om)]
    rows = np.stack(cols, axis=1)
    assert rows.shape[1] == NCOLS[kind] and rows.min() >= 0 and rows.max() <= P
    rc = np.zeros(256, dtype=np.int64)
    if kind == LT:
        ok = vals[:, 2] != MARK
        for c in range(5, 9):
            rc += np.bincount(vals[ok, c], minlength=256)
    return rows.astype(np.uint32), np.array(outs, dtype=np.int64), rc


def ref_reduce(groups, maximum, node=2, input_id=0, input_mult=-1, consumers=1, final=False):
    """(rows, out) of lmn_trace_sum_reduce / lmn_trace_max_reduce for groups (n_out lists of dim values, output order)."""
    om = 0 if final else m31(consumers)
    rows, outs = [], []
    n_out = len(groups)
    for g, xs in enumerate(groups):
        acc = xs[0] if maximum else 0
        for k, x in enumerate(int(v) for v in xs):
            nxt = max(acc, x) if maximum else acc + x
            last = k == len(xs) - 1
            ok = fits(x) and (not last or fits(nxt))
            ow = MARK if not ok else m31(nxt) if last else 0
            row = [node, input_id, g, int(g == n_out - 1), node, input_id, g + 1, m31(x), ow, m31(acc), m31(nxt), int(last)]
            row += ([int(x > acc)] if maximum else []) + [m31(input_mult), om if last else 0]
            rows.append(row)
            if last:
                outs.append(nxt if ok else 0)
            acc = nxt
    return np.array(rows, dtype=np.int64).astype(np.uint32), np.array(outs, dtype=np.int64)


def view_index(shape, strides, offset=0):
    """element indices of a view, row-major over its shape"""
    idx = np.full(shape, offset, dtype=np.int64)
    for ax, (d, st) in enumerate(zip(shape, strides)):
        shp = [1] * len(shape)
        shp[ax] = d
        idx = idx + (np.arange(d, dtype=np.int64) * st).reshape(shp)
    return idx.reshape(-1)


# ---- device side
def _run(ctx, kind, lhs, rhs, node=2, ids=(0, 1), mults=(-1, -1), consumers=1, final=False, lhs_view=None,
         rhs_view=None, n=None, rows=None, row_offset=0, rc=None):
    """one lmn_trace_elementwise(_v) / lmn_trace_less_than call on int32 host arrays; returns (rows, out, rc)"""
    for v in (lhs, rhs):
        assert v is None or -2 ** 31 <= min(v) and max(v) < 2 ** 31, "test values must be int32"
    dl = ctx.upload(np.asarray(lhs, dtype=np.int64).astype(np.int32))
    dr = ctx.upload(np.asarray(rhs, dtype=np.int64).astype(np.int32)) if rhs is not None else None
    n = n if n is not None else len(lhs)
    nid = list(ids[:2 if kind in BINARY else 1])
    nm = list(mults[:2 if kind in BINARY else 1])
    bufs = [dl] + ([dr] if dr is not None else [])
    if kind == LT:
        own_rc = rc is None
        rc = rc if rc is not None else ctx.upload(np.zeros(256, dtype=np.uint32))
        rb, ob = ctx.trace_less_than(dl, dr, n, node_id=node, input_ids=nid, num_consumers=consumers, range_check_mult=rc,
                                     is_final_output=final, input_mults=nm, rows=rows, row_offset=row_offset,
                                     lhs_view=lhs_view, rhs_view=rhs_view)
        if own_rc:
            bufs.append(rc)
    else:
        rb, ob = ctx.trace_elementwise(kind, dl, dr, n, node_id=node, input_ids=nid, num_consumers=consumers,
                                       is_final_output=final, input_mults=nm, rows=rows, row_offset=row_offset,
                                       lhs_view=lhs_view, rhs_view=rhs_view)
    got_rows = ctx.download(rb).reshape(-1, NCOLS[kind])
    got_out = ctx.download(ob, np.int32).astype(np.int64)
    got_rc = ctx.download(rc).astype(np.int64) if kind == LT else None
    bufs.append(ob)
    if rows is None:
        bufs.append(rb)
    for b in bufs:
        b.free()
    return got_rows, got_out, got_rc


def _assert_rows(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        r, c = bad[0]
        raise AssertionError("%s: %d words differ, first at row %d column %d: device %d, reference %d"
                             % (what, len(bad), r, c, got[r, c], want[r, c]))


def check_elementwise(ctx, kind, lhs, rhs=None, what="", **kw):
    """device rows / output / range-check multiplicities == the reference, for one launch"""
    rows, out, rc = _run(ctx, kind, lhs, rhs, **{k: v for k, v in kw.items() if k in ("node", "ids", "mults", "consumers",
                                                                                       "final")})
    want_rows, want_out, want_rc = ref_elementwise(kind, lhs, rhs, **kw)
    _assert_rows(rows, want_rows, "kind %d %s" % (kind, what))
    assert np.array_equal(out, want_out), "kind %d %s: output tensor" % (kind, what)
    if kind == LT:
        assert np.array_equal(rc, want_rc), "LessThan %s: range-check multiplicities" % what
    return want_rows


def edge_operands(kind):
    """(lhs, rhs) covering every edge of one kind"""
    if kind in (ADD, LT):
        pairs = [(a, b) for a in EDGES for b in EDGES]
    elif kind == MUL:
        pairs = [(a, b) for a in EDGES for b in EDGES] + MUL_PAIRS
    elif kind == REM:
        pairs = REM_PAIRS + [(a, b) for a in EDGES for b in EDGES if not (0 <= a <= R and 0 < b <= R)][:40]
    else:
        vals = {RECIP: RECIP_VALUES, SQRT: SQRT_VALUES}.get(kind, EDGES)
        return list(vals), None
    return [a for a, _ in pairs], [b for _, b in pairs]


def check_value_edges(ctx):
    """every elementwise kind at every value edge, one launch per kind: in-contract rows exact, the others marked"""
    for kind in (ADD, MUL, REM, LT, RECIP, SQRT, CONTIG, INPUTS):
        lhs, rhs = edge_operands(kind)
        check_elementwise(ctx, kind, lhs, rhs, what="value edges", mults=(-1, 3), consumers=2)


# the issue's table: one named element each, with the word the reference expects
NAMED_CASES = {
    "add_2^30+2^30": [(ADD, [1 << 30], [1 << 30])],
    # the product -2^32 is refused; where the contract allows that value (a running sum: 4 * -(2^30-1) - 4) its word is
    # -2^32 mod P = P - 2
    "mul_-2^22*2^22": [(MUL, [-(1 << 22)], [1 << 22]), (SUM, [[-R] * 4 + [-4, R, R, R, R - 2]], None)],
    "mul_3*2^20*3*2^20": [(MUL, [3 << 20], [3 << 20])],
    "sum_reduce_600x2^22": [(SUM, [[1 << 22] * 600], None)],
    "recip_-5000": [(RECIP, [-5000], None)],
    "rem_-7%3": [(REM, [-7], [3])],
    "sqrt_-1": [(SQRT, [-1], None)],
    "recip_0": [(RECIP, [0], None)],
}


def check_named_case(ctx, name):
    for kind, lhs, rhs in NAMED_CASES[name]:
        if kind == SUM:
            check_reduce(ctx, np.array(lhs, dtype=np.int64).reshape(1, -1, 1), False)
        else:
            check_elementwise(ctx, kind, lhs, rhs, what=name)


def _tiled(vals, n):
    return [vals[i % len(vals)] for i in range(n)]


def check_shapes(ctx, sizes=(1, 255, 256, 257, (1 << 18) + 5)):
    """lengths around TPB = 256 and one past 2^18, edge values cycling through them (the refused ones included)"""
    for n in sizes:
        for kind in (ADD, MUL, REM, LT, RECIP, SQRT, CONTIG, INPUTS):
            lhs, rhs = edge_operands(kind)
            # a different phase per size, so that the block boundaries fall on different values
            lhs = _tiled(lhs[n % len(lhs):] + lhs[:n % len(lhs)], n)
            rhs = _tiled(rhs[n % len(rhs):] + rhs[:n % len(rhs)], n) if rhs is not None else None
            check_elementwise(ctx, kind, lhs, rhs, what="n=%d" % n, node=7, ids=(5, 6), mults=(-1, 0), final=n % 2 == 1)


def check_less_than_multiplicities(ctx, n=(1 << 18) + 3):
    """every element on the same four limbs (equal operands: diff = P, limbs ff ff ff 7f; and lhs < rhs with one
    limb value): the 256-entry atomics must count n per limb exactly; then a second launch accumulates into the table"""
    rc = ctx.upload(np.zeros(256, dtype=np.uint32))
    rows, _, got = _run(ctx, LT, [5] * n, [5] * n, rc=rc)
    want = np.zeros(256, dtype=np.int64)
    want[255], want[127] = 3 * n, n
    assert np.array_equal(got, want)
    _assert_rows(rows, ref_elementwise(LT, [5] * n, [5] * n)[0], "LessThan equal operands")
    rows, _, got = _run(ctx, LT, [-R] * n, [-R + 0x01010101] * n, rc=rc)   # diff 0x01010101: limb 1 four times
    want[1] += 4 * n
    assert np.array_equal(got, want)
    rows, _, got = _run(ctx, LT, [R, -R, R + 1, 3] * 64, [-R, R, 0, 3] * 64, rc=rc)   # extreme pairs, one refused
    _, _, r = ref_elementwise(LT, [R, -R, R + 1, 3] * 64, [-R, R, 0, 3] * 64)
    assert np.array_equal(got, want + r)
    rc.free()


def wrapping_groups(rng, n_groups, dim, marked=True):
    """groups whose running sums pass +-P while most final sums stay in range: k values of magnitude near R and their
    negatives, shuffled, plus one value in range for odd dims.  With `marked`, one group ends outside the range and one
    holds an input outside it."""
    groups = []
    for gi in range(n_groups):
        # a run of one sign first (positive and negative groups alternate): the running sum climbs past +-P, then returns
        half = (1 - 2 * (gi % 2)) * rng.integers(R - 5000, R + 1, size=dim // 2)
        groups.append(np.concatenate([half, rng.permutation(-half)] + ([rng.integers(-R, R + 1, size=1)] if dim % 2 else [])))
    groups = np.array(groups, dtype=np.int64).reshape(n_groups, dim)
    if marked and n_groups > 2 and dim > 1:
        groups[1, :] = R                         # the result leaves the range
        groups[2, dim // 2] = -(2 ** 31)         # one input outside the range
    return groups


def check_reduce(ctx, t, maximum, node=21, input_id=20, consumers=1, rows=None, row_offset=0):
    """t: (front, dim, back) int64.  Device rows / output of the reduction of dim == the reference."""
    front, dim, back = t.shape
    dt = ctx.upload(t.reshape(-1).astype(np.int32))
    rb, ob = ctx.trace_sum_reduce(dt, front, dim, back, node_id=node, input_id=input_id, num_consumers=consumers,
                                  maximum=maximum, rows=rows, row_offset=row_offset)
    nc = NCOLS[MAX if maximum else SUM]
    got = ctx.download(rb).reshape(-1, nc)[row_offset:row_offset + t.size]
    groups = t.transpose(0, 2, 1).reshape(front * back, dim)
    want, want_out = ref_reduce(groups.tolist(), maximum, node=node, input_id=input_id, consumers=consumers)
    _assert_rows(got, want, "%s (%d, %d, %d)" % ("max" if maximum else "sum", front, dim, back))
    assert np.array_equal(ctx.download(ob, np.int32).astype(np.int64), want_out)
    for b in (dt, ob) + ((rb,) if rows is None else ()):
        b.free()
    return want


def check_reduce_shapes(ctx, seed=3):
    """group lengths 1, 255, 256, 257 and 3*256+7 (a group across four blocks: the cooperative carry-in), back > 1
    (strided groups), front*back around a block boundary; running sums past +-P, marked groups"""
    rng = np.random.default_rng(seed)
    for front, dim, back in ((257, 1, 1), (3, 1, 85), (2, 255, 3), (1, 256, 2), (3, 257, 1), (1, 3 * 256 + 7, 2),
                             (5, 3, 17), (2, 128, 1), (1, 2, 129)):
        groups = wrapping_groups(rng, front * back, dim)
        t = groups.reshape(front, back, dim).transpose(0, 2, 1).copy()
        for maximum in (False, True):
            check_reduce(ctx, t, maximum)


def check_views(ctx, seed=4):
    """lmn_trace_elementwise_v: expanded dimensions (stride 0), a slice with an offset, a 4-d permutation, broadcast on
    either operand - rows == the reference on the gathered elements"""
    from luminair_amd.backend import LmnView
    rng = np.random.default_rng(seed)
    edge = np.array(EDGES[:11], dtype=np.int64)             # the in-range edges
    base = rng.choice(edge, size=2 * 3 * 4 * 5 + 7)
    other = rng.choice(edge, size=len(base))
    cases = [
        ("expanded", (4, 3, 5), (5, 0, 1), 0, (4, 3, 5), (15, 5, 1), 0),
        ("slice+offset", (3, 4), (10, 2), 7, (3, 4), (4, 1), 3),
        ("permute 4-d", (5, 2, 4, 3), (1, 60, 15, 5), 0, (5, 2, 4, 3), (24, 12, 3, 1), 0),
        ("broadcast lhs", (6, 7), (0, 1), 2, (6, 7), (7, 1), 0),
        ("broadcast rhs", (6, 7), (7, 1), 0, (6, 7), (1, 0), 5),
    ]
    for name, ls, lst, lo, rs, rst, ro in cases:
        lv, rv = LmnView.make(ls, lst, lo), LmnView.make(rs, rst, ro)
        a = base[view_index(ls, lst, lo)]
        b = other[view_index(rs, rst, ro)]
        n = len(a)
        for kind in (ADD, MUL, LT):
            rows, out, _ = _run(ctx, kind, base, other, node=9, ids=(3, 4), lhs_view=lv, rhs_view=rv, n=n)
            want_rows, want_out, _ = ref_elementwise(kind, a, b, node=9, ids=(3, 4))
            _assert_rows(rows, want_rows, "%s kind %d" % (name, kind))
            assert np.array_equal(out, want_out), name
        for kind in (RECIP, SQRT, CONTIG):      # unary kinds read the lhs view; refused elements included
            rows, out, _ = _run(ctx, kind, base, None, node=9, ids=(3,), lhs_view=lv, n=n)
            want_rows, want_out, _ = ref_elementwise(kind, a, None, node=9, ids=(3,))
            _assert_rows(rows, want_rows, "%s kind %d" % (name, kind))
            assert np.array_equal(out, want_out), name


def ref_contiguous_buffer(phys, out_vals, node, input_id, input_mult, consumers):
    """LuminairContiguous in the reference's row rule: max(in, out) rows pairing the idx-th buffer element (0 past its
    end) with the idx-th output element (wrapping), is_last on the buffer's last element"""
    phys, out_vals = [int(v) for v in phys], [int(v) for v in out_vals]
    n = max(len(phys), len(out_vals))
    rows, outs = [], [0] * len(out_vals)
    for i in range(n):
        x = phys[i] if i < len(phys) else 0
        y = out_vals[i % len(out_vals)]
        ok = fits(x) and fits(y)
        rows.append([node, input_id, i, int(i == len(phys) - 1), node, input_id, i + 1, m31(x), m31(y) if ok else MARK,
                     m31(input_mult), m31(consumers)])
        if i < len(out_vals):
            outs[i] = y if ok else 0
    return np.array(rows, dtype=np.int64).astype(np.uint32), np.array(outs, dtype=np.int64)


def check_contiguous(ctx, seed=6):
    """lmn_trace_contiguous with in_size > out_size (a slice) and in_size < out_size (an expansion), edge values in the
    buffer (one outside the range)"""
    from luminair_amd.backend import LmnView
    rng = np.random.default_rng(seed)
    for in_size, shape, strides, offset in ((300, (7, 9), (20, 2), 11), (40, (3, 40), (0, 1), 0), (257, (257,), (1,), 0),
                                            (6, (4, 256), (0, 0), 5)):
        phys = rng.choice(np.array(EDGES[:11] + [R + 1], dtype=np.int64), size=in_size)
        out_size = int(np.prod(shape))
        view = LmnView.make(shape, strides, offset)
        dp = ctx.upload(phys.astype(np.int32))
        rb, ob = ctx.trace_contiguous(dp, in_size, out_size, node_id=4, input_id=2, num_consumers=3, view=view)
        want_rows, want_out = ref_contiguous_buffer(phys, phys[view_index(shape, strides, offset)], 4, 2, -1, 3)
        _assert_rows(ctx.download(rb).reshape(-1, 11), want_rows, "contiguous in %d out %d" % (in_size, out_size))
        assert np.array_equal(ctx.download(ob, np.int32).astype(np.int64), want_out)
        for b in (dp, rb, ob):
            b.free()


def check_lut_edges(ctx, n=(1 << 18) + 5):
    """LUT inputs exactly at lo and hi of each of several ranges (LookupLayout::find_index), and all n inputs on one
    LUT row (its multiplicity must be n); an input outside every range fails the call and leaves the context usable"""
    from luminair_amd.backend import LuminairBackendError
    ranges = [(-R, -R + 9), (-4097, -4095), (0, 0), (4095, 4097), (R - 9, R)]
    lens = [b - a + 1 for a, b in ranges]
    L = 1 << max(4, (sum(lens) - 1).bit_length())
    rng = np.random.default_rng(8)
    col1 = rng.integers(0, P, size=L).astype(np.uint32)
    col1[:3] = [0, P - 1, (P >> 1) + 1]         # words that read back as 0, -1 and the most negative value
    dcol = ctx.upload(col1)

    def run(inputs):
        mult = ctx.upload(np.zeros(L, dtype=np.uint32))
        di = ctx.upload(np.asarray(inputs, dtype=np.int64).astype(np.int32))
        rb, ob = ctx.alloc(len(inputs) * 12 * 4), ctx.alloc(len(inputs) * 4)
        try:
            ctx.trace_lut(9, di, len(inputs), node_id=6, input_id=5, num_consumers=2, lut_col1=dcol, mult=mult,
                          ranges=ranges, rows=rb, out=ob)
            return (ctx.download(rb).reshape(-1, 12), ctx.download(ob, np.int32).astype(np.int64),
                    ctx.download(mult).astype(np.int64))
        finally:
            for b in (di, mult, rb, ob):
                b.free()

    def li(a):
        base = 0
        for (lo, hi), ln in zip(ranges, lens):
            if lo <= a <= hi:
                return base + a - lo
            base += ln
        raise AssertionError(a)

    ends = [v for a, b in ranges for v in (a, b)]
    inputs = _tiled(ends, 1000)
    rows, out, mult = run(inputs)
    k = len(inputs)
    words = [int(col1[li(a)]) for a in inputs]
    want = np.array([[6, 5, i, int(i == k - 1), 6, 5, i + 1, m31(a), w, m31(-1), 2, 1]
                     for i, (a, w) in enumerate(zip(inputs, words))], dtype=np.int64)
    _assert_rows(rows, want.astype(np.uint32), "LUT range ends")
    assert np.array_equal(out, [w - P if w > P >> 1 else w for w in words])
    want_mult = np.zeros(L, dtype=np.int64)
    for a in inputs:
        want_mult[li(a)] += 1
    assert np.array_equal(mult, want_mult)
    for a in (ranges[0][0], ranges[2][0], ranges[4][1]):
        rows, out, mult = run([a] * n)
        assert mult[li(a)] == n and mult.sum() == n
        assert np.all(rows[:, 8] == col1[li(a)]) and np.all(rows[:, 7] == m31(a))
    for bad in (ranges[0][0] - 1, ranges[4][1] + 1, -2 ** 31, 1):
        try:
            run([0, bad, 0])
        except LuminairBackendError as e:
            assert e.code == -6
        else:
            raise AssertionError("LUT input %d outside every range was accepted" % bad)
    rows, _, mult = run([0, 0])                   # the context's range verdict was reset
    assert mult[li(0)] == 2
    dcol.free()


def check_row_offset_appends(ctx, n1=257, n2=300):
    """a second node of the same kind appends at row_offset: both blocks exact, the first untouched"""
    for kind in (ADD, MUL, REM, LT, RECIP, SQRT, CONTIG, INPUTS):
        lhs, rhs = edge_operands(kind)
        l1, l2 = _tiled(lhs, n1), _tiled(lhs[::-1], n2)
        r1 = _tiled(rhs, n1) if rhs is not None else None
        r2 = _tiled(rhs[::-1], n2) if rhs is not None else None
        rows = ctx.alloc((n1 + n2) * NCOLS[kind] * 4)
        _run(ctx, kind, l1, r1, node=3, ids=(1, 2), rows=rows)
        _run(ctx, kind, l2, r2, node=4, ids=(3, 2), mults=(-1, 0), consumers=0, final=True, rows=rows, row_offset=n1)
        got = ctx.download(rows).reshape(n1 + n2, NCOLS[kind])
        _assert_rows(got[:n1], ref_elementwise(kind, l1, r1, node=3, ids=(1, 2))[0], "first node, kind %d" % kind)
        _assert_rows(got[n1:], ref_elementwise(kind, l2, r2, node=4, ids=(3, 2), mults=(-1, 0), final=True)[0],
                     "appended node, kind %d" % kind)
        rows.free()
    rng = np.random.default_rng(12)
    t1 = wrapping_groups(rng, 3, 257).reshape(3, 257, 1)
    t2 = wrapping_groups(rng, 4, 5, marked=False).reshape(2, 5, 2)
    for maximum in (False, True):
        rows = ctx.alloc((t1.size + t2.size) * NCOLS[MAX if maximum else SUM] * 4)
        first = check_reduce(ctx, t1, maximum, rows=rows)
        check_reduce(ctx, t2, maximum, node=22, input_id=21, consumers=2, rows=rows, row_offset=t1.size)
        _assert_rows(ctx.download(rows).reshape(-1, NCOLS[MAX if maximum else SUM])[:t1.size], first, "reduce first node")
        rows.free()


def check_marked_rows_refused(lib, device=0, c_oracle=None):
    """A table holding a marked row is refused by lmn_prove (non-canonical word: the same table with a canonical word in
    its place is not refused for that reason); the same context then proves a good pie - made on the device from
    edge-but-valid values - to the C oracle's bytes."""
    from luminair_amd import backend
    from luminair_amd.backend import LuminairBackendError
    from oracle.cbackend import CKernels
    from oracle.channel import ProtocolVariant
    from oracle.proof import to_bincode
    from oracle.prover import prove
    c_oracle = c_oracle or CKernels()
    cfg = lib.default_config()
    cfg.protocol_variant = backend.VARIANT_PINNED
    ctx = backend.Context(device, cfg, lib)
    for kind, lhs, rhs in ((ADD, [R, 1, -R], [0, R, 1]), (MUL, [R, -R, 4096], [4096, 4097, -R]),
                           (RECIP, [1, 0, S * S + 1], None), (SQRT, [R, -1, 0], None), (REM, [R, -7, 5], [R, 3, 5]),
                           (LT, [R, -2 ** 31, -R], [-R, 0, R]), (INPUTS, [-R, -R - 1, R], None),
                           (CONTIG, [R + 1, 0, -R], None)):
        dl = ctx.upload(np.array(lhs, dtype=np.int64).astype(np.int32))
        dr = ctx.upload(np.array(rhs, dtype=np.int64).astype(np.int32)) if rhs is not None else None
        rc = ctx.upload(np.zeros(256, dtype=np.uint32))
        if kind == LT:
            rb, ob = ctx.trace_less_than(dl, dr, 3, node_id=2, input_ids=(0, 1), num_consumers=1, range_check_mult=rc)
        else:
            rb, ob = ctx.trace_elementwise(kind, dl, dr, 3, node_id=2, input_ids=(0, 1), num_consumers=1)
        got = ctx.download(rb).reshape(3, NCOLS[kind])
        _assert_rows(got, ref_elementwise(kind, lhs, rhs)[0], "marked launch, kind %d" % kind)
        assert (got == MARK).sum() == 1, kind
        extra = [(RC, ctx.download(rc).reshape(-1, 1), 256)] if kind == LT else []
        try:
            ctx.prove_tables(sorted([(kind, rb, 3)] + extra, key=lambda t: t[0]))
        except LuminairBackendError as e:
            assert e.code == backend.ERR_INVALID_ARGUMENT, (kind, e.code)
        else:
            raise AssertionError("lmn_prove accepted a table with a marked row (kind %d)" % kind)
        fixed = np.where(got == MARK, 0, got).astype(np.uint32)
        try:
            ctx.prove_tables(sorted([(kind, fixed, 3)] + extra, key=lambda t: t[0]))
        except LuminairBackendError as e:      # the patched row breaks a constraint, and nothing else is wrong
            assert e.code == backend.ERR_CONSTRAINTS, (kind, e.code)
        for b in (dl, dr, rc, rb, ob):
            if b is not None:
                b.free()
    # a good pie on the same context: Add / Mul / Recip rows of in-contract edges, generated on the device
    lhs, rhs = edge_operands(ADD)
    keep = [(a, b) for a, b in zip(lhs, rhs) if fits(a) and fits(b) and fits(a + b)]
    add_l, add_r = [a for a, _ in keep], [b for _, b in keep]
    lhs, rhs = edge_operands(MUL)
    keep = [(a, b) for a, b in zip(lhs, rhs) if v_mul(a, b)[0][2] != MARK]
    mul_l, mul_r = [a for a, _ in keep], [b for _, b in keep]
    rec = [a for a in RECIP_VALUES if 0 < a <= R]
    tabs, bufs = [], []
    for kind, l, r in ((ADD, add_l, add_r), (MUL, mul_l, mul_r), (RECIP, rec, None)):
        dl = ctx.upload(np.array(l, dtype=np.int64).astype(np.int32))
        dr = ctx.upload(np.array(r, dtype=np.int64).astype(np.int32)) if r is not None else None
        rb, ob = ctx.trace_elementwise(kind, dl, dr, len(l), node_id=2 + kind, input_ids=(0, 1), num_consumers=1,
                                       input_mults=(0, 0))
        tabs.append((kind, rb, len(l)))
        bufs += [b for b in (dl, dr, rb, ob) if b is not None]
    want_tabs = [(k, ref_elementwise(k, l, r, node=2 + k, mults=(0, 0))[0])
                 for k, l, r in ((ADD, add_l, add_r), (MUL, mul_l, mul_r), (RECIP, rec, None))]
    got = ctx.prove_tables(tabs)
    assert got == ctx.prove_tables([(k, r, len(r)) for k, r in want_tabs])
    assert got == to_bincode(prove([(k, r.astype(np.uint64)) for k, r in want_tabs], variant=ProtocolVariant.PINNED,
                                   kernels=c_oracle))
    for b in bufs:
        b.free()
    ctx.close()


def check_synthetic_agrees():
    """luminair_amd.synthetic (the host generators the other tests use) == this reference inside the contract, its
    to_m31 exact for any int64, and its generators refuse what the device refuses"""
    from luminair_amd import synthetic as syn
    vals = np.array([0, 1, -1, P, -P, P + 1, -P - 1, 2 ** 32, -2 ** 32, 2 ** 62, -2 ** 62, 2 ** 63 - 1, -2 ** 63],
                    dtype=np.int64)
    assert syn.to_m31(vals).tolist() == [int(v) % P for v in vals]
    inside = lambda kind, l, r: [i for i in range(len(l))
                                 if MARK not in ref_elementwise(kind, [l[i]], None if r is None else [r[i]])[0][0]]
    gens = {ADD: lambda l, r: syn.add_rows(l, r, 2, 0, 1, (-1, -1, 1)), MUL: lambda l, r: syn.mul_rows(l, r, 2, 0, 1, (-1, -1, 1)),
            REM: lambda l, r: syn.rem_rows(l, r, 2, 0, 1, (-1, -1, 1)), RECIP: lambda l, r: syn.recip_rows(l, 2, 0, (-1, 1)),
            SQRT: lambda l, r: syn.sqrt_rows(l, 2, 0, (-1, 1)), CONTIG: lambda l, r: syn.contiguous_rows(l, 2, 0, -1, 1),
            INPUTS: lambda l, r: syn.inputs_rows(l, 2, 1), LT: lambda l, r: syn.less_than_rows(l, r, 2, 0, 1, (-1, -1, 1))}
    for kind, gen in gens.items():
        lhs, rhs = edge_operands(kind)
        keep = inside(kind, lhs, rhs)
        l = np.array([lhs[i] for i in keep], dtype=np.int64)
        r = np.array([rhs[i] for i in keep], dtype=np.int64) if rhs is not None else None
        got = gen(l, r)
        want_rows, _, want_rc = ref_elementwise(kind, l, r)
        if kind == LT:
            got, counts = got
            assert np.array_equal(counts, want_rc)
        _assert_rows(got, want_rows, "synthetic kind %d" % kind)
    rng = np.random.default_rng(5)
    for maximum in (False, True):
        groups = wrapping_groups(rng, 6, 257, marked=False)
        gen = syn.max_reduce_rows if maximum else syn.sum_reduce_rows
        _assert_rows(gen(groups, 2, 0, -1, 1), ref_reduce(groups.tolist(), maximum)[0], "synthetic reduce")
    for fn, args in ((syn.recip_rows, ([4, 0],)), (syn.recip_rows, ([-5000],)), (syn.sqrt_rows, ([4, -1],)),
                     (syn.rem_rows, ([-7], [3])), (syn.rem_rows, ([7], [0])), (syn.rem_rows, ([7], [-3]))):
        try:
            fn(*args)
        except ValueError:
            continue
        raise AssertionError("%s accepted %r" % (fn.__name__, args))


def edge_graph(ctx):
    """A DeviceGraph of edge-but-valid values: inputs at the range ends, SumReduce whose running sums wrap past P, negative
    Mul operands (floor), Recip / Sqrt / Rem / LessThan / MaxReduce at their edges.  Returns the graph."""
    from luminair_amd.graph import DeviceGraph
    g = DeviceGraph(ctx)
    a = np.array([[R, R, R, -R, -R, -R, 5, -7],
                  [R, -R, R, -R, R, -R, R, -R],
                  [-R, -R, -R, R, R, R, -4097, 4095]], dtype=np.int64)
    b = np.array([[4096, -4096, 1, -1, 0, 2048, -2048, -4097],
                  [-4096, -4096, 4096, 4096, -1, -1, 1, 1],
                  [4096, 4096, -4096, 4096, -4096, 4096, 4097, -4097]], dtype=np.int64)
    assert np.abs(np.cumsum(a, axis=1)).max() > P
    ta, tb = g.input(a), g.input(b)
    s = g.sum_reduce(ta, axis=1)                               # running sums pass +-P, the results are -2, 0, -2
    m = g.mul(ta, tb)                                          # negative operands, |out| up to R
    sm = g.sum_reduce(m, axis=1)
    c = g.input(np.array([R - 2, -R + 3, 17], dtype=np.int64))
    g.output(g.add(g.add(s, c), sm))
    g.output(g.max_reduce(ta, axis=1))
    g.output(g.less_than(m, ta))
    g.output(g.recip(g.input(np.array([1, S * S, S * S + 1, R], dtype=np.int64))))
    g.output(g.sqrt(g.input(np.array([0, R, S, 1, 9 * S - 1], dtype=np.int64))))
    g.output(g.rem(g.input(np.array([0, 5, R, 7, R], dtype=np.int64)), g.input(np.array([1, 5, 3, R, R], dtype=np.int64))))
    g.output(g.contiguous(g.expand(g.input(np.array([-R, R, 0], dtype=np.int64)), 0, 2)))
    return g


def check_edge_graph_end_to_end(lib, device=0):
    """edge_graph on the device: every table equals the host mirror's rows (tests/host_graph.py), the proof verifies and
    equals ctx.prove_tables of the host rows byte for byte"""
    from luminair_amd import backend
    from host_graph import host_tables
    cfg = lib.default_config()
    cfg.protocol_variant = backend.VARIANT_PINNED
    ctx = backend.Context(device, cfg, lib)
    g = edge_graph(ctx)
    tables, luts, bufs = g.gen_trace()
    want, vals = host_tables(g)
    assert [k for k, _, _ in tables] == sorted(want)
    for k, buf, n in tables:
        _assert_rows(ctx.download(buf)[:n * want[k].shape[1]].reshape(n, -1), want[k], "graph table %d" % k)
    proof = ctx.prove_tables(tables, luts)
    lib.verify(proof, backend.VARIANT_PINNED)
    assert proof == ctx.prove_tables([(k, want[k], len(want[k])) for k in sorted(want)], luts)
    for b in bufs:
        b.free()
    ctx.close()


def check_host_mirror_refuses(ctx):
    """tests/host_graph.py refuses what the device marks: a value leaving the range, an op's precondition"""
    from luminair_amd.graph import DeviceGraph
    from host_graph import host_tables
    cases = [lambda g: g.add(g.input(np.array([R])), g.input(np.array([1]))),
             lambda g: g.mul(g.input(np.array([-(1 << 22)])), g.input(np.array([1 << 22]))),
             lambda g: g.sum_reduce(g.input(np.array([[1 << 22] * 600])), axis=1),
             lambda g: g.recip(g.input(np.array([-5000]))),
             lambda g: g.recip(g.input(np.array([0]))),
             lambda g: g.sqrt(g.input(np.array([-1]))),
             lambda g: g.rem(g.input(np.array([-7])), g.input(np.array([3]))),
             lambda g: g.input(np.array([R + 1]))]
    for make in cases:
        g = DeviceGraph(ctx)
        g.output(make(g))
        try:
            host_tables(g)
        except ValueError:
            continue
        raise AssertionError("host mirror accepted a graph outside the contract")
