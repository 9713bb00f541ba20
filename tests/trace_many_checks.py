"""The many-member trace producers (`lmn_trace_many_*`: one launch fills a node's rows for n_members pies), run against the
emulation build on CPU (tests/test_trace_many_emu.py) and the HIP libraries on GPU (tests/test_gpu_trace_many.py, also
through the batch library's own compile of the kernels).

Every check uses two yardsticks, neither of which is the code under test: the plain Python-integer reference of
tests/trace_checks.py applied per member, and the existing single-member producer called on member m's operands - with
word-for-word equality of rows, output tensor and multiplicity tables.  Buffers are laid out with a gap behind every member
(rows, outputs, tables) that is pre-filled with a sentinel and must come back untouched."""
import numpy as np

import trace_checks as tc
from trace_checks import (ADD, BINARY, CONTIG, INPUTS, LT, MARK, MAX, MUL, NCOLS, P, R, RECIP, REM, SQRT, SUM, ref_contiguous_buffer,
                          ref_elementwise, ref_reduce, view_index)

SENT = 0xDEADBEEF                       # rows, tables, counters' neighbours
SENT_I32 = -0x21524111                  # the same word as an int32 (output tensors)
KINDS = (ADD, MUL, REM, LT, RECIP, SQRT, CONTIG, INPUTS)
MEMBERS = (1, 2, 3, 65)                 # 65: a grid.y larger than a wave and than a tile
SIZES = (1, 255, 256, 257, 513)         # a full, a partial and a next block of TPB = 256 rows
MARK_COL = {ADD: 11, MUL: 11, REM: 11, LT: 11, RECIP: 8, SQRT: 8, CONTIG: 8, INPUTS: 5, SUM: 8, MAX: 8}
ERR_INVALID = -6
ERR_EMPTY = -1


def _i32(v):
    return np.asarray(v, dtype=np.int64).astype(np.int32)


def _sent(ctx, words):
    return ctx.upload(np.full(words, SENT, dtype=np.uint32))


def _pack(ctx, members, stride, shared):
    """per-member operand lists -> one int32 device buffer, `stride` elements apart (the gaps hold values outside the
    contract: nothing may read them); a shared operand is one list"""
    if members is None:
        return None
    if shared:
        return ctx.upload(_i32(members))
    buf = np.full(len(members) * stride, -2 ** 31, dtype=np.int64)
    for m, vals in enumerate(members):
        buf[m * stride:m * stride + len(vals)] = vals
    return ctx.upload(_i32(buf))


def member_operands(kind, n, m, dirty):
    """(lhs, rhs) of n elements for member m: the value edges of the kind in a phase of its own; a clean member holds only
    elements inside the contract, a dirty one every edge (the refused ones included)"""
    lhs, rhs = tc.edge_operands(kind)
    pairs = list(zip(lhs, rhs if rhs is not None else [0] * len(lhs)))
    if not dirty:
        pairs = [ab for ab in pairs if MARK not in ref_elementwise(kind, [ab[0]], [ab[1]] if kind in BINARY else None)[0][0]]
    ph = (7 * m + n) % len(pairs)
    pairs = pairs[ph:] + pairs[:ph]
    sel = [pairs[i % len(pairs)] for i in range(n)]
    return [a for a, _ in sel], ([b for _, b in sel] if kind in BINARY else None)


def run_elementwise(ctx, kind, lhs, rhs, M, n, lhs_shared=False, rhs_shared=False, lhs_view=None, rhs_view=None, gap=3,
                    rows=None, rows_stride=None, row_offset=0, out_shared=False, node=2, ids=(0, 1), mults=(-1, -1), consumers=1,
                    final=False):
    """one lmn_trace_many_elementwise_v call.  lhs / rhs: per-member lists of buffer values (one list when shared).
    Returns a dict: rows (M, n, nc), row_gap (the words behind each member's rows), out, out_gap, rc, rc_gap, refused."""
    nc = NCOLS[kind]
    binary = kind in BINARY
    ls = 0 if lhs_shared else max(len(v) for v in lhs) + gap
    rs = 0 if (rhs_shared or not binary) else max(len(v) for v in rhs) + gap
    dl, dr = _pack(ctx, lhs, ls, lhs_shared), _pack(ctx, rhs if binary else None, rs, rhs_shared)
    own_rows = rows is None
    rows_stride = rows_stride if rows_stride is not None else row_offset + n + 2
    if own_rows:
        rows = _sent(ctx, M * rows_stride * nc)
    os_ = 0 if out_shared else n + 1
    out = ctx.upload(np.full(n + 1 if out_shared else M * os_, SENT_I32, dtype=np.int32))
    rc_stride = 256 + 16
    rc = None
    if kind == LT:
        t = np.full((M, rc_stride), SENT, dtype=np.uint32)
        t[:, :256] = 0
        rc = ctx.upload(t)
    refused = ctx.upload(np.array([0] * M + [SENT], dtype=np.uint32))
    nid = list(ids[:2 if binary else 1])
    nm = list(mults[:2 if binary else 1])
    bufs = [b for b in (dl, dr, out, rc, refused) if b is not None] + ([rows] if own_rows else [])
    try:
        ctx.trace_many_elementwise(kind, dl, dr, n, M, node_id=node, input_ids=nid, num_consumers=consumers, rows=rows,
                                   rows_stride=rows_stride, out=out, out_stride=os_, lhs_stride=ls, rhs_stride=rs,
                                   is_final_output=final, input_mults=nm, row_offset=row_offset, lhs_view=lhs_view,
                                   rhs_view=rhs_view, range_check_mult=rc, range_check_mult_stride=rc_stride if rc is not None else 0,
                                   refused=refused)
        got = ctx.download(rows).reshape(M, rows_stride, nc)
        res = dict(rows=got[:, row_offset:row_offset + n], row_gap=got[:, row_offset + n:], table=got)
        o = ctx.download(out, np.int32).astype(np.int64)
        if out_shared:
            res.update(out=o[:n], out_gap=o[n:])
        else:
            o = o.reshape(M, os_)
            res.update(out=o[:, :n], out_gap=o[:, n:])
        if rc is not None:
            t = ctx.download(rc).reshape(M, rc_stride)
            res.update(rc=t[:, :256].astype(np.int64), rc_gap=t[:, 256:])
        cnt = ctx.download(refused)
        assert cnt[M] == SENT, "the word behind the refused counters was written"
        res["refused"] = [int(c) for c in cnt[:M]]
        return res
    finally:
        for b in bufs:
            b.free()


def _assert_member(ctx, kind, res, m, a, b, what, single=True, **kw):
    """member m's rows / output / table against the Python reference and the single-member producer on the element
    values a / b (already read through their views)"""
    want_rows, want_out, want_rc = ref_elementwise(kind, a, b, **kw)
    tc._assert_rows(res["rows"][m], want_rows, "%s member %d" % (what, m))
    assert np.array_equal(res["out"][m], want_out), "%s member %d: output tensor" % (what, m)
    n_marked = int((want_rows[:, MARK_COL[kind]] == MARK).sum())
    assert res["refused"][m] == n_marked, "%s member %d: refused %d, reference %d" % (what, m, res["refused"][m], n_marked)
    if kind == LT:
        assert np.array_equal(res["rc"][m], want_rc), "%s member %d: range-check multiplicities" % (what, m)
        assert res["rc"][m].sum() == 4 * (len(a) - n_marked)
    if single:
        s_rows, s_out, s_rc = tc._run(ctx, kind, a, b, **kw)
        assert np.array_equal(res["rows"][m], s_rows), "%s member %d: rows differ from the single form's" % (what, m)
        assert np.array_equal(res["out"][m], s_out), "%s member %d: output differs from the single form's" % (what, m)
        if kind == LT:
            assert np.array_equal(res["rc"][m], s_rc), "%s member %d: table differs from the single form's" % (what, m)
    return n_marked


def _assert_gaps(res, what):
    assert np.all(res["row_gap"] == SENT), "%s: rows behind a member's last row were written" % what
    assert np.all(res["out_gap"] == SENT_I32), "%s: output words behind a member's tensor were written" % what
    if "rc_gap" in res:
        assert np.all(res["rc_gap"] == SENT), "%s: words between the range-check tables were written" % what


def check_kind(ctx, kind, members=MEMBERS, sizes=SIZES):
    """one elementwise kind at every (members, elements per member): value edges spread over the members, odd members
    (and a lone member) hold refused elements and their neighbours do not"""
    for M in members:
        for n in sizes:
            dirty = [m % 2 == 1 or M == 1 for m in range(M)]
            ops = [member_operands(kind, n, m, dirty[m]) for m in range(M)]
            lhs, rhs = [o[0] for o in ops], ([o[1] for o in ops] if kind in BINARY else None)
            what = "kind %d, %d members of %d" % (kind, M, n)
            kw = dict(node=7, ids=(5, 6), mults=(-1, 3), consumers=2, final=n % 2 == 0)
            res = run_elementwise(ctx, kind, lhs, rhs, M, n, **kw)
            _assert_gaps(res, what)
            for m in range(M):
                marked = _assert_member(ctx, kind, res, m, lhs[m], rhs[m] if rhs else None, what, **kw)
                if not dirty[m]:     # marks only in the offending members' rows
                    assert marked == 0 and not np.any(res["rows"][m] == MARK), "%s: a mark in clean member %d" % (what, m)
            if n >= 255:
                assert any(res["refused"][m] for m in range(M) if dirty[m]), what


def check_shared(ctx, n=257, M=3):
    """left operand shared, right operand shared, both shared (per-member and shared output); out stride 0 with a
    per-member operand is refused"""
    from luminair_amd.backend import LuminairBackendError
    for kind in (ADD, MUL, LT, REM):
        ops = [member_operands(kind, n, m, m == 1) for m in range(M)]
        lhs, rhs = [o[0] for o in ops], [o[1] for o in ops]
        what = "kind %d" % kind
        res = run_elementwise(ctx, kind, lhs[0], rhs, M, n, lhs_shared=True)
        _assert_gaps(res, what + " lhs shared")
        for m in range(M):
            _assert_member(ctx, kind, res, m, lhs[0], rhs[m], what + " lhs shared")
        res = run_elementwise(ctx, kind, lhs, rhs[1], M, n, rhs_shared=True)
        _assert_gaps(res, what + " rhs shared")
        for m in range(M):
            _assert_member(ctx, kind, res, m, lhs[m], rhs[1], what + " rhs shared")
        res = run_elementwise(ctx, kind, lhs[1], rhs[1], M, n, lhs_shared=True, rhs_shared=True)
        _assert_gaps(res, what + " both shared")
        for m in range(M):
            _assert_member(ctx, kind, res, m, lhs[1], rhs[1], what + " both shared", single=m == 0)
        # one shared output tensor, stored by member 0: every member's rows are the same rows
        res = run_elementwise(ctx, kind, lhs[1], rhs[1], M, n, lhs_shared=True, rhs_shared=True, out_shared=True)
        want_rows, want_out, want_rc = ref_elementwise(kind, lhs[1], rhs[1])
        assert np.all(res["row_gap"] == SENT) and np.all(res["out_gap"] == SENT_I32)
        assert np.array_equal(res["out"], want_out), what + ": shared output tensor"
        for m in range(M):
            tc._assert_rows(res["rows"][m], want_rows, what + " shared output, member %d" % m)
            assert res["refused"][m] == int((want_rows[:, 11] == MARK).sum())
            if kind == LT:
                assert np.array_equal(res["rc"][m], want_rc)
        for ls, rs in ((False, True), (True, False), (False, False)):
            try:
                run_elementwise(ctx, kind, lhs[0] if ls else lhs, rhs[0] if rs else rhs, M, n, lhs_shared=ls, rhs_shared=rs,
                                out_shared=True)
            except LuminairBackendError as e:
                assert e.code == ERR_INVALID and "out_member_stride" in str(e), e
            else:
                raise AssertionError("out stride 0 with a per-member operand was accepted (kind %d)" % kind)
    for kind in (RECIP, SQRT, CONTIG, INPUTS):      # unary: the one operand shared, per-member and shared output
        a = member_operands(kind, n, 1, True)[0]
        for out_shared in (False, True):
            res = run_elementwise(ctx, kind, a, None, M, n, lhs_shared=True, out_shared=out_shared)
            want_rows, want_out, _ = ref_elementwise(kind, a, None)
            for m in range(M):
                tc._assert_rows(res["rows"][m], want_rows, "unary kind %d shared, member %d" % (kind, m))
                assert np.array_equal(res["out"] if out_shared else res["out"][m], want_out)
        try:
            run_elementwise(ctx, kind, [a] * M, None, M, n, out_shared=True)
        except LuminairBackendError as e:
            assert e.code == ERR_INVALID
        else:
            raise AssertionError("out stride 0 with a per-member operand was accepted (kind %d)" % kind)


def check_views(ctx, seed=4, M=3):
    """a view per operand - expanded dimension, slice with offset, permutation, broadcast - combined with a member stride
    larger than the viewed buffer"""
    from luminair_amd.backend import LmnView
    rng = np.random.default_rng(seed)
    edge = np.array(tc.EDGES[:11] + [R + 1], dtype=np.int64)     # the in-range edges and one value outside
    size = 2 * 3 * 4 * 5 + 7
    base = [rng.choice(edge[:11] if m != 1 else edge, size=size) for m in range(M)]
    other = [rng.choice(edge[:11], size=size) for m in range(M)]
    cases = [
        ("expanded", (4, 3, 5), (5, 0, 1), 0, (4, 3, 5), (15, 5, 1), 0),
        ("slice+offset", (3, 4), (10, 2), 7, (3, 4), (4, 1), 3),
        ("permute 4-d", (5, 2, 4, 3), (1, 60, 15, 5), 0, (5, 2, 4, 3), (24, 12, 3, 1), 0),
        ("broadcast lhs", (6, 7), (0, 1), 2, (6, 7), (7, 1), 0),
        ("broadcast rhs", (6, 7), (7, 1), 0, (6, 7), (1, 0), 5),
    ]
    for name, ls, lst, lo, rs, rst, ro in cases:
        lv, rv = LmnView.make(ls, lst, lo), LmnView.make(rs, rst, ro)
        li, ri = view_index(ls, lst, lo), view_index(rs, rst, ro)
        n = len(li)
        for kind in (ADD, MUL, LT, RECIP, SQRT, CONTIG):
            binary = kind in BINARY
            kw = dict(node=9, ids=(3, 4))
            res = run_elementwise(ctx, kind, [list(b) for b in base], [list(o) for o in other] if binary else None, M, n,
                                  lhs_view=lv, rhs_view=rv if binary else None, gap=13, **kw)
            _assert_gaps(res, name)
            for m in range(M):
                a, b = base[m][li], (other[m][ri] if binary else None)
                _assert_member(ctx, kind, res, m, a, b, "%s kind %d" % (name, kind), **kw)
        # the single form through the same views on member 2's buffers (the reference gathers; this one reads the views)
        rows, out, _ = tc._run(ctx, ADD, base[2], other[2], node=9, ids=(3, 4), lhs_view=lv, rhs_view=rv, n=n)
        res = run_elementwise(ctx, ADD, [list(b) for b in base], [list(o) for o in other], M, n, lhs_view=lv, rhs_view=rv,
                              gap=13, node=9, ids=(3, 4))
        assert np.array_equal(res["rows"][2], rows) and np.array_equal(res["out"][2], out), name


def check_row_offsets(ctx, n1=257, n2=300, stride=600, M=3):
    """two nodes of one kind appended at row_offset 0 and n1 in a table of member stride 600: both blocks exact per member,
    the rows between a member's last row and the next member's first untouched"""
    for kind in KINDS:
        nc = NCOLS[kind]
        rows = _sent(ctx, M * stride * nc)
        o1 = [member_operands(kind, n1, m, m == 1) for m in range(M)]
        o2 = [member_operands(kind, n2, m + 5, m == 2) for m in range(M)]
        kw1 = dict(node=3, ids=(1, 2))
        kw2 = dict(node=4, ids=(3, 2), mults=(-1, 0), consumers=0, final=True)
        binary = kind in BINARY
        r1 = run_elementwise(ctx, kind, [o[0] for o in o1], [o[1] for o in o1] if binary else None, M, n1, rows=rows,
                             rows_stride=stride, **kw1)
        r2 = run_elementwise(ctx, kind, [o[0] for o in o2], [o[1] for o in o2] if binary else None, M, n2, rows=rows,
                             rows_stride=stride, row_offset=n1, **kw2)
        assert np.all(r1["table"][:, n1:] == SENT), "kind %d: the first node wrote behind its rows" % kind
        for m in range(M):
            _assert_member(ctx, kind, r1, m, o1[m][0], o1[m][1], "first node, kind %d" % kind, **kw1)
            _assert_member(ctx, kind, r2, m, o2[m][0], o2[m][1], "appended node, kind %d" % kind, **kw2)
            tc._assert_rows(r2["table"][m, :n1], ref_elementwise(kind, o1[m][0], o1[m][1], **kw1)[0],
                            "first node after the append, kind %d member %d" % (kind, m))
        assert np.all(r2["table"][:, n1 + n2:] == SENT), "kind %d: rows between the members were written" % kind
        rows.free()


REDUCE_SHAPES = ((1, 1, 1), (2, 300, 3), (3, 7, 64), (1, 513, 1), (5, 256, 1))


def check_reduce(ctx, shapes=REDUCE_SHAPES, members=(1, 3), seed=3):
    """SumReduce / MaxReduce per member: groups straddling a block boundary (the cooperative carry-in reads the member's own
    input) and ending exactly at one; running sums that leave the value range, marked groups, in ONE member only"""
    rng = np.random.default_rng(seed)
    for front, dim, back in shapes:
        for M in members + ((65,) if (front, dim, back) == (3, 7, 64) else ()):
            wild = M // 2                       # the member whose running sums pass +-P and whose groups are marked
            ts = []
            for m in range(M):
                if m == wild:
                    g = tc.wrapping_groups(rng, front * back, dim)
                else:
                    g = rng.integers(-4096, 4097, size=(front * back, dim)).astype(np.int64) + 1000 * (m + 1)
                ts.append(g.reshape(front, back, dim).transpose(0, 2, 1).copy())
            n_rows, n_out = front * dim * back, front * back
            for maximum in (False, True):
                kind = MAX if maximum else SUM
                nc = NCOLS[kind]
                what = "%s (%d, %d, %d) x %d" % ("max" if maximum else "sum", front, dim, back, M)
                in_stride, rows_stride, out_stride = n_rows + 5, n_rows + 2, n_out + 1
                di = _pack(ctx, [t.reshape(-1) for t in ts], in_stride, False)
                rows = _sent(ctx, M * rows_stride * nc)
                out = ctx.upload(np.full(M * out_stride, SENT_I32, dtype=np.int32))
                refused = ctx.upload(np.array([0] * M + [SENT], dtype=np.uint32))
                ctx.trace_many_reduce(di, front, dim, back, M, node_id=21, input_id=20, num_consumers=2, rows=rows,
                                      rows_stride=rows_stride, out=out, out_stride=out_stride, inp_stride=in_stride,
                                      maximum=maximum, refused=refused)
                got = ctx.download(rows).reshape(M, rows_stride, nc)
                o = ctx.download(out, np.int32).astype(np.int64).reshape(M, out_stride)
                cnt = ctx.download(refused)
                assert cnt[M] == SENT and np.all(got[:, n_rows:] == SENT) and np.all(o[:, n_out:] == SENT_I32), what
                for m in range(M):
                    groups = ts[m].transpose(0, 2, 1).reshape(n_out, dim)
                    want, want_out = ref_reduce(groups.tolist(), maximum, node=21, input_id=20, consumers=2)
                    tc._assert_rows(got[m, :n_rows], want, "%s member %d" % (what, m))
                    assert np.array_equal(o[m, :n_out], want_out), what
                    marked = int((want[:, 8] == MARK).sum())
                    assert cnt[m] == marked, "%s member %d: refused %d, reference %d" % (what, m, cnt[m], marked)
                    if m != wild:
                        assert marked == 0
                    if m in (0, wild, M - 1):        # the single form on the member's own tensor
                        dt = ctx.upload(_i32(ts[m].reshape(-1)))
                        rb, ob = ctx.trace_sum_reduce(dt, front, dim, back, node_id=21, input_id=20, num_consumers=2,
                                                      maximum=maximum)
                        assert np.array_equal(ctx.download(rb).reshape(-1, nc), got[m, :n_rows]), what
                        assert np.array_equal(ctx.download(ob, np.int32).astype(np.int64), o[m, :n_out]), what
                        for b in (dt, rb, ob):
                            b.free()
                for b in (di, rows, out, refused):
                    b.free()


def check_lut(ctx, members=(1, 3, 65), sizes=(1, 257, 513)):
    """Exp2 rows over two ranges with inputs on both ends of each; one member has inputs outside every range - its rows are
    marked and counted, it adds nothing to its table; every member's table is its own histogram"""
    ranges = [(-4097, -4000), (-3, 300)]
    lens = [b - a + 1 for a, b in ranges]
    L = 512
    rng = np.random.default_rng(8)
    col1 = rng.integers(0, P, size=L).astype(np.uint32)
    col1[:3] = [0, P - 1, (P >> 1) + 1]
    dcol = ctx.upload(col1)
    ends = [v for a, b in ranges for v in (a, b)]
    outside = [ranges[0][0] - 1, ranges[0][1] + 1, ranges[1][0] - 1, ranges[1][1] + 1, -2 ** 31, 2 ** 31 - 1]

    def li(a):
        base = 0
        for (lo, hi), ln in zip(ranges, lens):
            if lo <= a <= hi:
                return base + a - lo
            base += ln
        return -1

    for M in members:
        for n in sizes:
            bad_m = M // 2
            ins = []
            for m in range(M):
                inside = ends + [int(v) for v in rng.integers(ranges[1][0], ranges[1][1] + 1, size=5)]
                pool = inside + outside if m == bad_m else inside
                ins.append([pool[(i + 3 * m) % len(pool)] for i in range(n)])
            if n == 1:
                ins[bad_m] = [outside[0]]
            what = "LUT %d members of %d" % (M, n)
            in_stride, rows_stride, out_stride, mult_stride = n + 4, n + 2, n + 1, L + 8
            di = _pack(ctx, ins, in_stride, False)
            rows = _sent(ctx, M * rows_stride * 12)
            out = ctx.upload(np.full(M * out_stride, SENT_I32, dtype=np.int32))
            t = np.full((M, mult_stride), SENT, dtype=np.uint32)
            t[:, :L] = 0
            mult = ctx.upload(t)
            refused = ctx.upload(np.array([0] * M + [SENT], dtype=np.uint32))
            ctx.trace_many_lut(9, di, n, M, node_id=6, input_id=5, num_consumers=2, lut_col1=dcol, ranges=ranges, mult=mult,
                               mult_stride=mult_stride, rows=rows, rows_stride=rows_stride, out=out, out_stride=out_stride,
                               inp_stride=in_stride, refused=refused)
            got = ctx.download(rows).reshape(M, rows_stride, 12)
            o = ctx.download(out, np.int32).astype(np.int64).reshape(M, out_stride)
            mt = ctx.download(mult).reshape(M, mult_stride)
            cnt = ctx.download(refused)
            assert cnt[M] == SENT and np.all(got[:, n:] == SENT) and np.all(o[:, n:] == SENT_I32), what
            assert np.all(mt[:, L:] == SENT), what + ": words between the multiplicity tables were written"
            for m in range(M):
                words = [int(col1[li(a)]) if li(a) >= 0 else MARK for a in ins[m]]
                want = np.array([[6, 5, i, int(i == n - 1), 6, 5, i + 1, a % P, w, (-1) % P, 2, 1]
                                 for i, (a, w) in enumerate(zip(ins[m], words))], dtype=np.int64).astype(np.uint32)
                tc._assert_rows(got[m, :n], want, "%s member %d" % (what, m))
                assert np.array_equal(o[m, :n], [0 if w == MARK else w - P if w > P >> 1 else w for w in words]), what
                hist = np.zeros(L, dtype=np.int64)
                for a in ins[m]:
                    if li(a) >= 0:
                        hist[li(a)] += 1
                assert np.array_equal(mt[m, :L], hist), "%s member %d: multiplicities" % (what, m)
                n_bad = sum(1 for a in ins[m] if li(a) < 0)
                assert cnt[m] == n_bad and (n_bad > 0) == (m == bad_m), (what, m, cnt[m], n_bad)
                if m != bad_m and m in (0, M - 1):       # the single form (it fails the call for the other member)
                    ds, dm = ctx.upload(_i32(ins[m])), ctx.upload(np.zeros(L, dtype=np.uint32))
                    rb, ob = ctx.trace_lut(9, ds, n, node_id=6, input_id=5, num_consumers=2, lut_col1=dcol, mult=dm,
                                           ranges=ranges)
                    assert np.array_equal(ctx.download(rb).reshape(-1, 12), got[m, :n]), what
                    assert np.array_equal(ctx.download(ob, np.int32).astype(np.int64), o[m, :n]), what
                    assert np.array_equal(ctx.download(dm), mt[m, :L]), what
                    for b in (ds, dm, rb, ob):
                        b.free()
            for b in (di, rows, out, mult, refused):
                b.free()
    # the single-range case is one range
    n, M = 40, 2
    ins = [[-3 + (i + m) % 304 for i in range(n)] for m in range(M)]
    di, rows, out = _pack(ctx, ins, n, False), _sent(ctx, M * n * 12), ctx.alloc(M * n * 4)
    mult = ctx.upload(np.zeros(M * L, dtype=np.uint32))
    ctx.trace_many_lut(9, di, n, M, node_id=6, input_id=5, num_consumers=2, lut_col1=dcol, ranges=[(-3, 300)], mult=mult,
                       mult_stride=L, rows=rows, rows_stride=n, out=out, out_stride=n, inp_stride=n)
    got = ctx.download(rows).reshape(M, n, 12)
    for m in range(M):
        assert [int(w) for w in got[m, :, 8]] == [int(col1[a + 3]) for a in ins[m]]
    for b in (di, rows, out, mult, dcol):
        b.free()


def check_contiguous(ctx, seed=6, M=3):
    """the reference's buffer rule per member, in_size > out_size (a slice) and in_size < out_size (an expansion); one member
    holds a value outside the range"""
    from luminair_amd.backend import LmnView
    rng = np.random.default_rng(seed)
    for in_size, shape, strides, offset in ((300, (7, 9), (20, 2), 11), (40, (3, 40), (0, 1), 0), (257, (257,), (1,), 0),
                                            (6, (4, 256), (0, 0), 5)):
        out_size = int(np.prod(shape))
        n_rows = max(in_size, out_size)
        what = "contiguous in %d out %d" % (in_size, out_size)
        phys = [rng.choice(np.array(tc.EDGES[:11] + ([R + 1] if m == 1 else []), dtype=np.int64), size=in_size)
                for m in range(M)]
        phys[1][5] = R + 1
        view = LmnView.make(shape, strides, offset)
        in_stride, rows_stride, out_stride = in_size + 5, n_rows + 2, out_size + 1
        di = _pack(ctx, phys, in_stride, False)
        rows = _sent(ctx, M * rows_stride * 11)
        out = ctx.upload(np.full(M * out_stride, SENT_I32, dtype=np.int32))
        refused = ctx.upload(np.array([0] * M + [SENT], dtype=np.uint32))
        ctx.trace_many_contiguous(di, in_size, out_size, M, node_id=4, input_id=2, num_consumers=3, rows=rows,
                                  rows_stride=rows_stride, out=out, out_stride=out_stride, inp_stride=in_stride, view=view,
                                  refused=refused)
        got = ctx.download(rows).reshape(M, rows_stride, 11)
        o = ctx.download(out, np.int32).astype(np.int64).reshape(M, out_stride)
        cnt = ctx.download(refused)
        assert cnt[M] == SENT and np.all(got[:, n_rows:] == SENT) and np.all(o[:, out_size:] == SENT_I32), what
        for m in range(M):
            want_rows, want_out = ref_contiguous_buffer(phys[m], phys[m][view_index(shape, strides, offset)], 4, 2, -1, 3)
            tc._assert_rows(got[m, :n_rows], want_rows, "%s member %d" % (what, m))
            assert np.array_equal(o[m, :out_size], want_out), what
            marked = int((want_rows[:, 8] == MARK).sum())
            assert cnt[m] == marked and (marked > 0) == (m == 1), (what, m, cnt[m], marked)
            dp = ctx.upload(_i32(phys[m]))
            rb, ob = ctx.trace_contiguous(dp, in_size, out_size, node_id=4, input_id=2, num_consumers=3, view=view)
            assert np.array_equal(ctx.download(rb).reshape(-1, 11), got[m, :n_rows]), what
            assert np.array_equal(ctx.download(ob, np.int32).astype(np.int64), o[m, :out_size]), what
            for b in (dp, rb, ob):
                b.free()
        for b in (di, rows, out, refused):
            b.free()


def check_argument_errors(ctx):
    """every refusal of the header returns its code before any launch and leaves sentinel-filled buffers untouched;
    n_members = 0 is LMN_OK and touches nothing"""
    import ctypes as C
    from luminair_amd import backend as B
    from luminair_amd.backend import LmnView, LuminairBackendError
    n, M, L = 20, 3, 64
    ops = ctx.upload(_i32(list(range(1, 200))))
    rows = _sent(ctx, M * 40 * 22)
    out = ctx.upload(np.full(M * 40, SENT_I32, dtype=np.int32))
    tabs = _sent(ctx, M * 300)
    refused = _sent(ctx, M)
    col1 = ctx.upload(np.arange(L, dtype=np.uint32))

    def untouched(what):
        assert np.all(ctx.download(rows) == SENT) and np.all(ctx.download(out, np.int32) == SENT_I32), what
        assert np.all(ctx.download(tabs) == SENT) and np.all(ctx.download(refused) == SENT), what

    def refused_call(what, names, fn, code=ERR_INVALID, **kw):
        try:
            fn(**kw)
        except LuminairBackendError as e:
            assert e.code == code, (what, e.code)
            assert any(nm in str(e) for nm in names), "%s: lmn_last_error does not name the argument: %s" % (what, e)
        else:
            raise AssertionError("%s was accepted" % what)
        untouched(what)

    ew = dict(kind=ADD, lhs=ops, rhs=ops, n=n, n_members=M, node_id=2, input_ids=(0, 1), num_consumers=1, rows=rows,
              rows_stride=40, out=out, out_stride=40, lhs_stride=n, rhs_stride=n, refused=refused)
    call = ctx.trace_many_elementwise
    refused_call("n_members > LMN_TRACE_MANY_MAX", ["n_members"], call, **dict(ew, n_members=B.TRACE_MANY_MAX + 1))
    refused_call("rows stride < n", ["rows_member_stride"], call, **dict(ew, rows_stride=n - 1))
    refused_call("rows stride < row_offset + n", ["rows_member_stride"], call, **dict(ew, row_offset=21))
    refused_call("out stride < n", ["out_member_stride"], call, **dict(ew, out_stride=n - 1))
    refused_call("out stride 0, per-member operand", ["out_member_stride"], call, **dict(ew, out_stride=0))
    refused_call("out stride 0, one operand per member", ["out_member_stride"], call, **dict(ew, out_stride=0, lhs_stride=0))
    lt = dict(ew, kind=LT, range_check_mult=tabs, range_check_mult_stride=300)
    refused_call("range-check stride < 256", ["range_check_mult_member_stride"], call, **dict(lt, range_check_mult_stride=255))
    refused_call("range-check stride 0", ["range_check_mult_member_stride"], call, **dict(lt, range_check_mult_stride=0))
    refused_call("LessThan without its table", ["range-check", "range_check"], call, **dict(lt, range_check_mult=None))
    refused_call("null lhs", ["lhs_dev"], call, **dict(ew, lhs=None))
    refused_call("null rhs of a binary kind", ["right operand", "rhs"], call, **dict(ew, rhs=None))
    refused_call("null rows", ["rows_dev"], call, **dict(ew, rows=None))
    refused_call("not an elementwise kind", ["kind"], call, **dict(ew, kind=SUM))
    refused_call("view shape product != n", ["view"], call, **dict(ew, lhs_view=LmnView.make((3, 5), (5, 1))))
    bad_view = LmnView.make((n,), (1,))
    bad_view.ndim = 5
    refused_call("view with 5 dimensions", ["view"], call, **dict(ew, rhs_view=bad_view))
    refused_call("n = 0 (the single form's EmptyTrace)", ["EmptyTrace"], call, code=ERR_EMPTY, **dict(ew, n=0))
    refused_call("n >= 2^31", ["too large"], call, **dict(ew, n=1 << 31, rows_stride=1 << 32, out_stride=1 << 32))

    cg = dict(inp=ops, in_size=30, out_size=n, n_members=M, node_id=2, input_id=0, num_consumers=1, rows=rows, rows_stride=40,
              out=out, out_stride=40, inp_stride=30, refused=refused, view=LmnView.make((n,), (1,), 3))
    call = ctx.trace_many_contiguous
    refused_call("contiguous: n_members", ["n_members"], call, **dict(cg, n_members=B.TRACE_MANY_MAX + 1))
    refused_call("contiguous: rows stride < max(in, out)", ["rows_member_stride"], call, **dict(cg, rows_stride=29))
    refused_call("contiguous: out stride < out_size", ["out_member_stride"], call, **dict(cg, out_stride=n - 1))
    refused_call("contiguous: out stride 0", ["out_member_stride"], call, **dict(cg, out_stride=0))
    refused_call("contiguous: null input", ["input_dev"], call, **dict(cg, inp=None))
    refused_call("contiguous: null rows", ["rows_dev"], call, **dict(cg, rows=None))
    refused_call("contiguous: the view leaves the buffer", ["view"], call, **dict(cg, view=LmnView.make((n,), (2,), 0)))
    refused_call("contiguous: out > in without a view", ["view"], call, **dict(cg, view=None, in_size=10))
    refused_call("contiguous: empty", ["EmptyTrace"], call, code=ERR_EMPTY, **dict(cg, out_size=0, view=None))

    rd = dict(inp=ops, front=2, dim=5, back=2, n_members=M, node_id=2, input_id=0, num_consumers=1, rows=rows, rows_stride=40,
              out=out, out_stride=4, inp_stride=20, refused=refused)
    call = ctx.trace_many_reduce
    for maximum in (False, True):
        r = dict(rd, maximum=maximum)
        refused_call("reduce: n_members", ["n_members"], call, **dict(r, n_members=B.TRACE_MANY_MAX + 1))
        refused_call("reduce: rows stride", ["rows_member_stride"], call, **dict(r, rows_stride=19))
        refused_call("reduce: out stride < front * back", ["out_member_stride"], call, **dict(r, out_stride=3))
        refused_call("reduce: out stride 0", ["out_member_stride"], call, **dict(r, out_stride=0))
        refused_call("reduce: null input", ["input_dev"], call, **dict(r, inp=None))
        refused_call("reduce: null rows", ["rows_dev"], call, **dict(r, rows=None))
        refused_call("reduce: dim = 0", ["EmptyTrace"], call, code=ERR_EMPTY, **dict(r, dim=0))
        refused_call("reduce: too large", ["too large"], call, **dict(r, front=1 << 20, dim=1 << 11, rows_stride=1 << 32,
                                                                        out_stride=1 << 21))

    lu = dict(kind=9, inp=ops, n=n, n_members=M, node_id=2, input_id=0, num_consumers=1, lut_col1=col1, ranges=[(1, 30), (40, 60)],
              mult=tabs, mult_stride=300, rows=rows, rows_stride=40, out=out, out_stride=40, inp_stride=n, refused=refused)
    call = ctx.trace_many_lut
    refused_call("lut: n_members", ["n_members"], call, **dict(lu, n_members=B.TRACE_MANY_MAX + 1))
    refused_call("lut: rows stride", ["rows_member_stride"], call, **dict(lu, rows_stride=n - 1))
    refused_call("lut: out stride", ["out_member_stride"], call, **dict(lu, out_stride=n - 1))
    refused_call("lut: out stride 0", ["out_member_stride"], call, **dict(lu, out_stride=0))
    refused_call("lut: mult stride < the ranges' rows", ["mult_member_stride"], call, **dict(lu, mult_stride=50))
    refused_call("lut: mult stride 0", ["mult_member_stride"], call, **dict(lu, mult_stride=0))
    refused_call("lut: null input", ["input_dev"], call, **dict(lu, inp=None))
    refused_call("lut: null lut_col1", ["lut_col1_dev"], call, **dict(lu, lut_col1=None))
    refused_call("lut: null mult", ["mult_dev"], call, **dict(lu, mult=None))
    refused_call("lut: null rows", ["rows_dev"], call, **dict(lu, rows=None))
    refused_call("lut: not a LUT kind", ["kind"], call, **dict(lu, kind=ADD))
    refused_call("lut: 17 ranges", ["ranges"], call, **dict(lu, ranges=[(3 * k, 3 * k + 1) for k in range(17)]))
    refused_call("lut: no range", ["ranges"], call, **dict(lu, ranges=[]))
    refused_call("lut: overlapping ranges", ["ranges"], call, **dict(lu, ranges=[(1, 30), (30, 60)]))
    refused_call("lut: view shape", ["view"], call, **dict(lu, view=LmnView.make((3, 5), (5, 1))))
    refused_call("lut: n = 0", ["EmptyTrace"], call, code=ERR_EMPTY, **dict(lu, n=0))

    # null info: the wrappers always pass one, so straight through the C ABI
    lib = ctx.lib.lib
    rc = lib.lmn_trace_many_reduce(ctx.handle, 0, ops.ptr, 20, 2, 5, 2, None, M, rows.ptr, 0, 40, out.ptr, 4, refused.ptr)
    assert rc == ERR_INVALID and b"info" in lib.lmn_last_error(ctx.handle)
    rc = lib.lmn_trace_many_elementwise_v(ctx.handle, ADD, ops.ptr, None, n, ops.ptr, None, n, n, None, M, rows.ptr, 0, 40,
                                          out.ptr, 40, None, 0, refused.ptr)
    assert rc == ERR_INVALID and b"info" in lib.lmn_last_error(ctx.handle)
    untouched("null info")

    # n_members = 0: LMN_OK, nothing touched - whatever else the call holds
    ctx.trace_many_elementwise(**dict(ew, n_members=0))
    ctx.trace_many_elementwise(**dict(ew, n_members=0, rows=None, lhs=None, rows_stride=0))
    ctx.trace_many_contiguous(**dict(cg, n_members=0))
    ctx.trace_many_reduce(**dict(rd, n_members=0))
    ctx.trace_many_lut(**dict(lu, n_members=0))
    untouched("n_members = 0")
    # and the context still works: the same call, accepted
    ctx.trace_many_elementwise(**ew)
    got = ctx.download(rows).reshape(-1, 15)[:M * 40].reshape(M, 40, 15)
    for m in range(M):
        vals = list(range(1 + m * n, 1 + (m + 1) * n))
        tc._assert_rows(got[m, :n], ref_elementwise(ADD, vals, vals)[0], "after the refusals, member %d" % m)
    assert [int(c) for c in ctx.download(refused)] == [SENT] * M
    for b in (ops, rows, out, tabs, refused, col1):
        b.free()


# ---- whole graphs
def mlp_graph(ctx, x0, widths=(2, 8, 8, 1), seed=42, lut_half_range=8 * 4096, per_member=False):
    """the shape of level2_checks.device_mlp (BASELINE config 4: a tanh MLP through an Exp2 LUT) with the input x0 - per
    member when asked - and shared weights.  Returns (graph, input tensor, output tensor, numpy forward pass of x0)."""
    from luminair_amd.graph import DeviceGraph
    S = 4096
    rng = np.random.default_rng(seed)
    g = DeviceGraph(ctx)
    g.set_lut("exp2", -lut_half_range, lut_half_range)
    cs = int(round(-2.0 / np.log(2.0) * S))
    c_scale, c_one, c_two, c_neg1 = g.constant(cs), g.constant(S), g.constant(2 * S), g.constant(-S)
    x_in = g.input(np.asarray(x0), per_member=per_member)
    h, ref = x_in, np.asarray(x0).astype(np.int64)
    for li_, (n_in, n_out) in enumerate(zip(widths[:-1], widths[1:])):
        w = rng.integers(-600, 600, size=(n_out, n_in))
        b = rng.integers(-512, 512, size=n_out)
        y = g.add(g.sum_reduce(g.mul(g.expand(h, 0, n_out), g.input(w)), axis=1), g.input(b))
        ref = ((ref[None, :] * w) >> 12).sum(axis=1) + b
        if li_ + 2 < len(widths):
            t = g.mul(y, g.broadcast_to(c_scale, (n_out,)))
            u = g.mul(g.recip(g.add(g.exp2(t), g.broadcast_to(c_one, (n_out,)))), g.broadcast_to(c_two, (n_out,)))
            h = g.add(u, g.broadcast_to(c_neg1, (n_out,)))
            e = np.rint(np.exp2(((ref * cs) >> 12) / S) * S).astype(np.int64)
            ref = ((((S * S) // (e + S)) * 2 * S) >> 12) - S
        else:
            h = y
    g.output(h)
    return g, x_in, h, ref


def member_inputs(n_members, width=2, seed=11):
    return np.random.default_rng(seed).integers(-2048, 2048, size=(n_members, width))


def _tables_words(ctx, tables):
    return [(k, n, ctx.download(b)[:n * (NCOLS_ALL[k])]) for k, b, n in tables]


NCOLS_ALL = {0: 15, 1: 16, 2: 13, 3: 12, 4: 1, 5: 14, 6: 15, 7: 13, 8: 16, 9: 12, 10: 1, 11: 12, 12: 1, 13: 22, 14: 1, 15: 7, 16: 11}


def check_graph(ctx, n_members=5, widths=(2, 8, 8, 1)):
    """the MLP with a per-member input and shared weights: every member's tables from gen_trace_many equal, word for word,
    the tables gen_trace produces for that member's input alone; read(h, m) equals the numpy forward pass"""
    xs = member_inputs(n_members, widths[0])
    g, x_in, h, _ = mlp_graph(ctx, xs[0], widths, per_member=True)
    pies, luts, bufs, refused = g.gen_trace_many(n_members, {x_in: xs})
    assert refused == [0] * n_members
    many = [_tables_words(ctx, pie) for pie in pies]
    outs = [g.read(h, m) for m in range(n_members)]
    weights = [n.out for n in g.nodes if n.host is not None and not n.per_member]
    shared = [g.read(t) for t in weights] + [g.read(t, member=3) for t in weights[:1]]
    try:
        g.read(h)
    except ValueError:
        pass
    else:
        raise AssertionError("read() of a per-member tensor without a member was accepted")
    for b in bufs:
        b.free()
    for t, got in zip(weights + weights[:1], shared):
        host = next(n.host for n in g.nodes if n.out is t)
        assert np.array_equal(got, host)
    for m in range(n_members):
        g1, _, h1, ref = mlp_graph(ctx, xs[m], widths)
        tables, luts1, bufs1 = g1.gen_trace()
        single = _tables_words(ctx, tables)
        assert [(k, n) for k, n, _ in single] == [(k, n) for k, n, _ in many[m]], "member %d: table shapes" % m
        for (k, n, want), (_, _, got) in zip(single, many[m]):
            assert np.array_equal(got, want), "member %d: table of kind %d differs from gen_trace's" % (m, k)
        assert np.array_equal(outs[m], ref) and np.array_equal(g1.read(h1), ref), "member %d: forward pass" % m
        assert sorted(luts1) == sorted(luts) and all(np.array_equal(luts1[k][1], luts[k][1]) for k in luts)
        for b in bufs1:
            b.free()


def check_graph_feeds_are_checked(ctx):
    xs = member_inputs(3)
    g, x_in, h, _ = mlp_graph(ctx, xs[0], per_member=True)
    other = next(n.out for n in g.nodes if n.host is not None and not n.per_member)
    for feeds in ({}, {x_in: xs[:2]}, {x_in: xs, other: np.zeros((3,) + other.shape)}):
        try:
            g.gen_trace_many(3, feeds)
        except ValueError:
            continue
        raise AssertionError("gen_trace_many accepted feeds %r" % (feeds,))


def check_batch_end_to_end(batch_lib_path, device=0, n_members=5, widths=(2, 8, 8, 1), lut_half_range=8 * 4096):
    """gen_trace_many's device-resident tables through BatchProver.prove_batch: every member's proof is the bytes
    Context.prove_tables returns for that member's per-pie tables (gen_trace on the member's input alone), and verifies under
    VARIANT_PINNED.  Then with one member whose input drives an Exp2 argument out of the LUT's range: that member alone gets
    a non-zero code, the others' proofs are still the same bytes."""
    import ctypes as C
    from luminair_amd import backend as B
    from luminair_amd.batch import BatchProver
    lib = B.Library(batch_lib_path)
    cfg = lib.default_config()
    cfg.protocol_variant = B.VARIANT_PINNED
    ctx = B.Context(device, cfg, lib)
    bp = BatchProver(device, n_members, protocol_variant=B.VARIANT_PINNED, library_path=batch_lib_path)
    try:
        xs = member_inputs(n_members, widths[0])
        want = []
        for m in range(n_members):
            g1, _, _, _ = mlp_graph(ctx, xs[m], widths, lut_half_range=lut_half_range)
            tables, luts1, bufs1 = g1.gen_trace()
            want.append(ctx.prove_tables(tables, luts1))
            for b in bufs1:
                b.free()
        g, x_in, h, _ = mlp_graph(ctx, xs[0], widths, lut_half_range=lut_half_range, per_member=True)
        pies, luts, bufs, refused = g.gen_trace_many(n_members, {x_in: xs})
        assert refused == [0] * n_members
        got = bp.prove_batch(pies, luts)
        for m in range(n_members):
            assert got[m] == want[m], "member %d: the batched proof differs from prove_tables of its own tables" % m
            lib.verify(got[m], B.VARIANT_PINNED)
        assert ctx.prove_tables(pies[2], luts) == want[2]          # the same tables on the producing context
        for b in bufs:
            b.free()
        # member 1 leaves the LUT: the first layer's Exp2 argument is about -2.9 * y, |y| up to ~0.3 * |x| + 0.125
        bad = xs.copy()
        bad[1] = [2 ** 29, 2 ** 29]
        pies, luts, bufs, refused = g.gen_trace_many(n_members, {x_in: bad})
        assert refused[1] > 0 and [r for m, r in enumerate(refused) if m != 1] == [0] * (n_members - 1), refused
        arrs = (C.POINTER(B.LmnTable) * n_members)()
        keep = []
        for i, t in enumerate(pies):
            arr, nt, st, k = B.Context._marshal_tables(None, t, luts)
            keep.append(k)
            arrs[i] = C.cast(arr, C.POINTER(B.LmnTable))
        proofs, lens, rcs = (C.POINTER(C.c_uint8) * n_members)(), (C.c_size_t * n_members)(), (C.c_int * n_members)()
        rc = bp.lib.lib.lmn_batch_prove(bp.handle, n_members, arrs, nt, C.byref(st), proofs, lens, rcs)
        out = []
        for i in range(n_members):
            out.append(C.string_at(proofs[i], lens[i]) if proofs[i] else None)
            if proofs[i]:
                bp.lib.lib.lmn_free(proofs[i])
        assert rc != 0 and rcs[1] != 0 and out[1] is None, (rc, list(rcs))
        assert [c for m, c in enumerate(rcs) if m != 1] == [0] * (n_members - 1), list(rcs)
        for m in range(n_members):
            if m != 1:
                assert out[m] == want[m], "member %d: proof changed next to a refused member" % m
        for b in bufs:
            b.free()
    finally:
        bp.close()
        ctx.close()
