"""Checks of the device producers that fill a row sink (`lmn_rows_append_*`: the `sink=` argument of `Context.trace_*`,
`DeviceGraph.gen_trace(columns=True)`), shared by the emulation suite (tests/test_trace_sink_emu.py) and the GPU suite
(tests/test_gpu_trace_sink.py).  Every comparison is exact.  The expected rows are those of the plain Python-integer
references of tests/trace_checks.py; the expected columns are those rows transposed, followed by `lmn_kind_padding_row` up to
2^log_size, and a finished sink's columns are read with `lmn_download` from `table.rows` (`RowSink.columns`).

The sizes are the edges of a 64-lane wave, a 256-lane block and the 256-row chunk tile of the sinks: a node of n rows in
{1, 255, 256, 257, 513} appended at a sink count in {0, 3, 256, 259} - a count is reached by appending a first node of that
many rows."""
import ctypes as C

import numpy as np

import trace_checks as tc
import trace_many_checks as tm
from row_stream_checks import padded_columns
from trace_checks import ADD, BINARY, CONTIG, INPUTS, LT, MARK, MAX, MUL, NCOLS, P, R, RECIP, REM, SQRT, SUM
from luminair_amd import backend
from luminair_amd.backend import LmnView, LuminairBackendError

KINDS = (ADD, MUL, RECIP, SQRT, REM, LT, CONTIG, INPUTS)
SIZES = (1, 255, 256, 257, 513)
COUNTS = (0, 3, 256, 259)
ERR_INVALID, ERR_EMPTY = -6, -1
SIN, EXP2 = 3, 9
NODE = dict(node=9, ids=(3, 4))


def _i32(v):
    return np.asarray(v, dtype=np.int64).astype(np.int32)


def in_contract(kind):
    """(lhs, rhs) of `edge_operands(kind)` without the elements the contract refuses: each kind's value edges"""
    lhs, rhs = tc.edge_operands(kind)
    rows = tc.ref_elementwise(kind, lhs, rhs)[0]
    keep = rows[:, tm.MARK_COL[kind]] != MARK
    assert keep.any()
    pick = lambda v: [x for x, k in zip(v, keep) if k] if v is not None else None
    return pick(lhs), pick(rhs)


def tiled(vals, n, shift=0):
    return [vals[(i + shift) % len(vals)] for i in range(n)] if vals is not None else None


class Refused:
    """the shared uint32 counter of refused elements"""

    def __init__(self, ctx):
        self.ctx, self.buf = ctx, ctx.upload(np.zeros(1, dtype=np.uint32))

    def read(self):
        return int(self.ctx.download(self.buf)[0])

    def free(self):
        self.buf.free()


def append(ctx, sink, kind, lhs, rhs, rc=None, refused=None, lhs_view=None, rhs_view=None, n=None, node=2, ids=(0, 1),
           mults=(-1, -1), consumers=1, final=False):
    """one lmn_rows_append_elementwise_v call on int32 host arrays; returns the output tensor (int64).  Reading it back
    waits for the producer, so the operands are free when this returns."""
    dl = ctx.upload(_i32(lhs))
    dr = ctx.upload(_i32(rhs)) if rhs is not None else None
    n = n if n is not None else len(lhs)
    k = 2 if kind in BINARY else 1
    kw = dict(node_id=node, input_ids=list(ids[:k]), num_consumers=consumers, is_final_output=final, input_mults=list(mults[:k]),
              lhs_view=lhs_view, rhs_view=rhs_view, sink=sink, refused=refused.buf if refused else None)
    try:
        if kind == LT:
            got, ob = ctx.trace_less_than(dl, dr, n, range_check_mult=rc, **kw)
        else:
            got, ob = ctx.trace_elementwise(kind, dl, dr, n, **kw)
        assert got is sink
        out = ctx.download(ob, np.int32).astype(np.int64)
        ob.free()
        return out
    finally:
        dl.free()
        if dr is not None:
            dr.free()


def assert_columns(sink, lib, rows, what):
    want = padded_columns(lib, sink.kind, rows)
    got = sink.columns()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        c, r = bad[0]
        raise AssertionError("%s: %d words differ, first at column %d row %d: sink %d, reference %d"
                             % (what, len(bad), c, r, got[c, r], want[c, r]))


# ---- 1. elementwise, every kind, every size at every sink count
def check_kind(ctx, kind, sizes=SIZES, counts=COUNTS):
    lib = ctx.lib
    lhs0, rhs0 = in_contract(kind)
    for n in sizes:
        a, b = tiled(lhs0, n), tiled(rhs0, n)
        want_rows, want_out, want_rc = tc.ref_elementwise(kind, a, b, **NODE)
        row_rows, row_out, row_rc = tc._run(ctx, kind, a, b, **NODE)          # the row form on the same operands
        tc._assert_rows(row_rows, want_rows, "row form, kind %d n %d" % (kind, n))
        for count in counts:
            what = "kind %d n %d at count %d" % (kind, n, count)
            rc = ctx.upload(np.zeros(256, dtype=np.uint32)) if kind == LT else None
            with ctx.row_sink(kind, count + n) as sink:
                first_rows, first_rc = np.zeros((0, NCOLS[kind]), dtype=np.uint32), 0
                if count:
                    fa, fb = tiled(lhs0, count, 1), tiled(rhs0, count, 1)
                    append(ctx, sink, kind, fa, fb, rc=rc, node=7, ids=(5, 6))
                    first_rows, _, first_rc = tc.ref_elementwise(kind, fa, fb, node=7, ids=(5, 6))
                    assert sink.n_rows == count, what
                out = append(ctx, sink, kind, a, b, rc=rc, **NODE)
                assert sink.n_rows == count + n, what
                sink.finish()
                assert_columns(sink, lib, np.concatenate([first_rows, want_rows]), what)
                assert np.array_equal(out, want_out) and np.array_equal(out, row_out), what + ": output tensor"
                if kind == LT:
                    got_rc = ctx.download(rc).astype(np.int64)
                    assert np.array_equal(got_rc, want_rc + first_rc), what + ": range-check multiplicities"
                    if not count:
                        assert np.array_equal(got_rc, row_rc), what
                    rc.free()


# ---- 2. views
def check_views(ctx, seed=4, n=257):
    """an expanded dimension (stride 0), a slice with an offset and a permutation at n = 257 (prime: its permutation can only
    swap a unit axis), and check_views' own 4-d permutation at n = 120; each appended at count 3"""
    rng = np.random.default_rng(seed)
    edge = np.array(tc.EDGES[:11], dtype=np.int64)             # the in-range edges
    base = rng.choice(edge[np.abs(edge) <= 4097], size=7 + 3 * n)
    other = rng.choice(edge[np.abs(edge) <= 4097], size=len(base))
    cases = [
        ("expanded", (n,), (0,), 5, (n,), (1,), 0),
        ("expanded 2-d", (n, 1), (0, 1), 2, (1, n), (0, 1), 3),
        ("slice+offset", (n,), (3,), 7, (n,), (2,), 1),
        ("permuted unit axis", (n, 1), (1, n), 0, (1, n), (n, 1), 0),
        ("permute 4-d", (5, 2, 4, 3), (1, 60, 15, 5), 0, (5, 2, 4, 3), (24, 12, 3, 1), 0),
    ]
    for name, ls, lst, lo, rs, rst, ro in cases:
        lv, rv = LmnView.make(ls, lst, lo), LmnView.make(rs, rst, ro)
        a, b = base[tc.view_index(ls, lst, lo)], other[tc.view_index(rs, rst, ro)]
        m = len(a)
        for kind in (ADD, MUL, LT, RECIP, CONTIG):
            binary = kind in BINARY
            if kind == RECIP:
                src_a, va = np.abs(base) + 1, np.abs(a) + 1
            else:
                src_a, va = base, a
            want_rows, want_out, _ = tc.ref_elementwise(kind, va, b if binary else None, **NODE)
            rc = ctx.upload(np.zeros(256, dtype=np.uint32)) if kind == LT else None
            with ctx.row_sink(kind, 3 + m) as sink:
                fa, fb = tiled(list(va), 3), tiled(list(b), 3) if binary else None
                append(ctx, sink, kind, fa, fb, rc=rc, node=7, ids=(5, 6))
                out = append(ctx, sink, kind, src_a, other if binary else None, rc=rc, lhs_view=lv,
                             rhs_view=rv if binary else None, n=m, **NODE)
                sink.finish()
                first = tc.ref_elementwise(kind, fa, fb, node=7, ids=(5, 6))[0]
                assert_columns(sink, ctx.lib, np.concatenate([first, want_rows]), "%s kind %d" % (name, kind))
                assert np.array_equal(out, want_out), (name, kind)
            if rc is not None:
                rc.free()


# ---- 3. two nodes and a host chunk in one sink
def check_mixed_with_host_push(ctx, n1=257, n_host=5, n2=300):
    for kind in (ADD, LT):
        lhs0, rhs0 = in_contract(kind)
        a1, b1, ah, bh, a2, b2 = (tiled(v, n, s) for n, s in ((n1, 0), (n_host, 2), (n2, 5)) for v in (lhs0, rhs0))
        r1 = tc.ref_elementwise(kind, a1, b1, node=3, ids=(1, 2))[0]
        rh = tc.ref_elementwise(kind, ah, bh, node=4, ids=(1, 2))[0]
        r2 = tc.ref_elementwise(kind, a2, b2, node=5, ids=(3, 2), mults=(-1, 0), final=True)[0]
        rc = ctx.upload(np.zeros(256, dtype=np.uint32)) if kind == LT else None
        with ctx.row_sink(kind, n1 + n_host + n2) as sink:
            append(ctx, sink, kind, a1, b1, rc=rc, node=3, ids=(1, 2))
            sink.push(rh)
            assert sink.n_rows == n1 + n_host
            append(ctx, sink, kind, a2, b2, rc=rc, node=5, ids=(3, 2), mults=(-1, 0), final=True)
            sink.finish()
            assert_columns(sink, ctx.lib, np.concatenate([r1, rh, r2]), "device, host, device; kind %d" % kind)
        if rc is not None:
            rc.free()
    # ... and in the other order: the host chunk first, a device node behind it, a host chunk last
    lhs0, rhs0 = in_contract(MUL)
    a, b = tiled(lhs0, n1), tiled(rhs0, n1)
    rd = tc.ref_elementwise(MUL, a, b, **NODE)[0]
    rh = tc.ref_elementwise(MUL, tiled(lhs0, n_host, 1), tiled(rhs0, n_host, 1), node=4)[0]
    with ctx.row_sink(MUL, n1 + 2 * n_host) as sink:
        sink.push(rh)
        append(ctx, sink, MUL, a, b, **NODE)
        sink.push(rh)
        sink.finish()
        assert_columns(sink, ctx.lib, np.concatenate([rh, rd, rh]), "host, device, host")


# ---- 4. reduce
REDUCE_SHAPES = ((1, 1, 1), (3, 300, 1), (2, 5, 7), (1, 257, 2))


def append_reduce(ctx, sink, t, maximum, refused=None, node=21, input_id=20, consumers=1):
    front, dim, back = t.shape
    dt = ctx.upload(_i32(t.reshape(-1)))
    try:
        got, ob = ctx.trace_sum_reduce(dt, front, dim, back, node_id=node, input_id=input_id, num_consumers=consumers,
                                       maximum=maximum, sink=sink, refused=refused.buf if refused else None)
        assert got is sink
        out = ctx.download(ob, np.int32).astype(np.int64)
        ob.free()
        return out
    finally:
        dt.free()


def reduce_groups(t):
    front, dim, back = t.shape
    return t.transpose(0, 2, 1).reshape(front * back, dim).tolist()


def check_reduce(ctx, shapes=REDUCE_SHAPES, counts=(0, 3), seed=3):
    """groups that straddle blocks ((3, 300, 1): 900 rows, (1, 257, 2)), back > 1, running sums past +-P"""
    rng = np.random.default_rng(seed)
    for front, dim, back in shapes:
        groups = tc.wrapping_groups(rng, front * back, dim, marked=False)
        t = groups.reshape(front, back, dim).transpose(0, 2, 1).copy()
        head = np.array([5, -7, R], dtype=np.int64).reshape(1, 3, 1)
        for maximum in (False, True):
            kind = MAX if maximum else SUM
            want, want_out = tc.ref_reduce(reduce_groups(t), maximum, node=21, input_id=20)
            row_form = tc.check_reduce(ctx, t, maximum)                        # the row form == the reference
            assert np.array_equal(row_form, want)
            for count in counts:
                what = "%s (%d, %d, %d) at count %d" % ("max" if maximum else "sum", front, dim, back, count)
                with ctx.row_sink(kind, count + t.size) as sink:
                    first = np.zeros((0, NCOLS[kind]), dtype=np.uint32)
                    if count:
                        assert head.size == count
                        append_reduce(ctx, sink, head, maximum, node=11, input_id=10)
                        first = tc.ref_reduce(reduce_groups(head), maximum, node=11, input_id=10)[0]
                    out = append_reduce(ctx, sink, t, maximum)
                    assert sink.n_rows == count + t.size, what
                    sink.finish()
                    assert_columns(sink, ctx.lib, np.concatenate([first, want]), what)
                    assert np.array_equal(out, want_out), what


# ---- 5. contiguous, buffer rule
def check_contiguous(ctx, seed=6):
    """check_contiguous' cases: in_size > out_size (a slice), in_size < out_size (an expansion), equal sizes; in-contract
    edge values in the buffer; at counts 0 and 3"""
    rng = np.random.default_rng(seed)
    for in_size, shape, strides, offset in ((300, (7, 9), (20, 2), 11), (40, (3, 40), (0, 1), 0), (257, (257,), (1,), 0),
                                            (6, (4, 256), (0, 0), 5)):
        phys = rng.choice(np.array(tc.EDGES[:11], dtype=np.int64), size=in_size)
        out_size = int(np.prod(shape))
        view = LmnView.make(shape, strides, offset)
        want_rows, want_out = tc.ref_contiguous_buffer(phys, phys[tc.view_index(shape, strides, offset)], 4, 2, -1, 3)
        dp = ctx.upload(_i32(phys))
        rb, ob = ctx.trace_contiguous(dp, in_size, out_size, node_id=4, input_id=2, num_consumers=3, view=view)   # row form
        tc._assert_rows(ctx.download(rb).reshape(-1, 11), want_rows, "row form")
        rb.free()
        ob.free()
        for count in (0, 3):
            what = "contiguous in %d out %d at count %d" % (in_size, out_size, count)
            with ctx.row_sink(CONTIG, count + max(in_size, out_size)) as sink:
                first = np.zeros((0, 11), dtype=np.uint32)
                if count:
                    _, o1 = ctx.trace_contiguous(dp, 3, 3, node_id=8, input_id=2, num_consumers=1, sink=sink)
                    o1.free()
                    first = tc.ref_contiguous_buffer(phys[:3], phys[:3], 8, 2, -1, 1)[0]
                got, ob = ctx.trace_contiguous(dp, in_size, out_size, node_id=4, input_id=2, num_consumers=3, view=view, sink=sink)
                assert got is sink and sink.n_rows == count + max(in_size, out_size), what
                out = ctx.download(ob, np.int32).astype(np.int64)
                ob.free()
                sink.finish()
                assert_columns(sink, ctx.lib, np.concatenate([first, want_rows]), what)
                assert np.array_equal(out, want_out), what
        dp.free()


# ---- 6. LUT
def check_lut(ctx, n=257):
    """two disjoint ranges, inputs on both ends of both: columns, outputs and multiplicities equal the single form's (and the
    rows spelled out here); then one input outside every range: LMN_OK, counted once, the finish refused"""
    lib = ctx.lib
    ranges = [(-4097, -4095), (4095, 4100)]
    ends = [v for a, b in ranges for v in (a, b)]
    L = 16
    rng = np.random.default_rng(8)
    col1 = rng.integers(0, P, size=L).astype(np.uint32)
    col1[:3] = [0, P - 1, (P >> 1) + 1]         # words that read back as 0, -1 and the most negative value
    dcol = ctx.upload(col1)
    li = lambda a: a + 4097 if a <= -4095 else 3 + a - 4095
    inputs = tiled(ends + [-4096, 4097], n)
    di = ctx.upload(_i32(inputs))
    common = dict(node_id=6, input_id=5, num_consumers=2, lut_col1=dcol, ranges=ranges)
    # the single form
    m1 = ctx.upload(np.zeros(L, dtype=np.uint32))
    rb, ob = ctx.trace_lut(EXP2, di, n, mult=m1, **common)
    single_rows, single_out = ctx.download(rb).reshape(-1, 12), ctx.download(ob, np.int32)
    single_mult = ctx.download(m1)
    words = [int(col1[li(a)]) for a in inputs]
    want = np.array([[6, 5, i, int(i == n - 1), 6, 5, i + 1, tc.m31(a), w, tc.m31(-1), 2, 1]
                     for i, (a, w) in enumerate(zip(inputs, words))], dtype=np.int64).astype(np.uint32)
    tc._assert_rows(single_rows, want, "single LUT form")
    for b in (rb, ob):
        b.free()
    for count in (0, 3):
        m2 = ctx.upload(np.zeros(L, dtype=np.uint32))
        refused = Refused(ctx)
        with ctx.row_sink(EXP2, count + n) as sink:
            first = np.zeros((0, 12), dtype=np.uint32)
            if count:
                _, o1 = ctx.trace_lut(EXP2, di, count, mult=m2, sink=sink, **common)
                o1.free()
                first = want[:count].copy()
                first[:, 3] = [0, 0, 1]
            got, ob = ctx.trace_lut(EXP2, di, n, mult=m2, sink=sink, refused=refused.buf, **common)
            assert got is sink
            out = ctx.download(ob, np.int32)
            ob.free()
            sink.finish()
            assert_columns(sink, lib, np.concatenate([first, single_rows]), "LUT at count %d" % count)
            assert np.array_equal(out, single_out)
            want_mult = single_mult.astype(np.int64)
            for a in inputs[:count]:
                want_mult[li(a)] += 1
            assert np.array_equal(ctx.download(m2).astype(np.int64), want_mult)
            assert refused.read() == 0
        m2.free()
        refused.free()
    # one input outside every range
    for bad in (4094, -4094, 4101, -2 ** 31):
        bad_in = list(inputs)
        bad_in[129] = bad
        db = ctx.upload(_i32(bad_in))
        m2 = ctx.upload(np.zeros(L, dtype=np.uint32))
        refused = Refused(ctx)
        with ctx.row_sink(EXP2, n) as sink:
            _, ob = ctx.trace_lut(EXP2, db, n, mult=m2, sink=sink, refused=refused.buf, **common)     # LMN_OK: no exception
            out = ctx.download(ob, np.int32)
            assert refused.read() == 1, bad
            want_out = single_out.copy()
            want_out[129] = tc.MARK - P             # the word P read back as a value: 0
            assert np.array_equal(out, want_out), bad
            want_mult = single_mult.astype(np.int64)
            want_mult[li(inputs[129])] -= 1
            assert np.array_equal(ctx.download(m2).astype(np.int64), want_mult), bad
            _finish_refused(sink)
            ob.free()
        for b in (db, m2):
            b.free()
        refused.free()
    for b in (dcol, di, m1):
        b.free()


def _finish_refused(sink):
    try:
        sink.finish()
    except LuminairBackendError as e:
        assert e.code == ERR_INVALID, e
        assert "refused" in str(e) and "canonical" in str(e), e
    else:
        raise AssertionError("lmn_rows_finish accepted a sink with a refused element")
    assert sink.table is None


# ---- 7. refused elements
def check_refused(ctx, kind):
    """edge_operands(kind), out-of-contract values included: the count, the zeros in the output tensor, the refused finish;
    then reset, a clean table and a finish that succeeds: the reset is ordered between the two tables' producers"""
    lhs, rhs = tc.edge_operands(kind)
    n = len(lhs)
    want_rows, want_out, want_rc = tc.ref_elementwise(kind, lhs, rhs, **NODE)
    n_marked = int((want_rows[:, tm.MARK_COL[kind]] == MARK).sum())
    assert n_marked > 0
    ca, cb = in_contract(kind)
    ca, cb = tiled(ca, 300), tiled(cb, 300)
    clean_rows, clean_out, clean_rc = tc.ref_elementwise(kind, ca, cb, node=12, ids=(10, 11))
    refused = Refused(ctx)
    with ctx.row_sink(kind, max(n, 300)) as sink:
        for round_ in range(2):        # the second round: a failed table behind a clean one, too
            rc = ctx.upload(np.zeros(256, dtype=np.uint32)) if kind == LT else None
            before = refused.read()
            out = append(ctx, sink, kind, lhs, rhs, rc=rc, refused=refused, **NODE)
            assert refused.read() - before == n_marked, (kind, refused.read(), n_marked)
            assert np.array_equal(out, want_out), kind
            assert np.all(out[want_rows[:, tm.MARK_COL[kind]] == MARK] == 0)
            if kind == LT:
                assert np.array_equal(ctx.download(rc).astype(np.int64), want_rc), "a refused element added a multiplicity"
            _finish_refused(sink)
            # the context and the sink are usable: appending without a reset is refused, a reset starts a clean table
            try:
                append(ctx, sink, kind, ca, cb, rc=rc, node=12, ids=(10, 11))
            except LuminairBackendError as e:
                assert e.code == ERR_INVALID and "rows" in str(e), e
            else:
                raise AssertionError("append to a failed sink without reset was accepted")
            if rc is not None:
                ctx.upload_to(rc, np.zeros(256, dtype=np.uint32))
            sink.reset()
            assert sink.n_rows == 0
            out = append(ctx, sink, kind, ca, cb, rc=rc, refused=refused, node=12, ids=(10, 11))
            sink.finish()                                   # must succeed
            assert_columns(sink, ctx.lib, clean_rows, "clean table behind a failed one, kind %d" % kind)
            assert np.array_equal(out, clean_out)
            if kind == LT:
                assert np.array_equal(ctx.download(rc).astype(np.int64), clean_rc)
                rc.free()
            assert refused.read() - before == n_marked      # never reset by a call, and the clean table added nothing
            sink.reset()
    refused.free()


def check_refused_reduce(ctx, seed=5):
    rng = np.random.default_rng(seed)
    groups = tc.wrapping_groups(rng, 4, 300, marked=True)
    t = groups.reshape(4, 1, 300).transpose(0, 2, 1).copy()
    for maximum in (False, True):
        want, want_out = tc.ref_reduce(reduce_groups(t), maximum, node=21, input_id=20)
        n_marked = int((want[:, 8] == MARK).sum())
        assert n_marked > 0
        refused = Refused(ctx)
        with ctx.row_sink(MAX if maximum else SUM, t.size) as sink:
            out = append_reduce(ctx, sink, t, maximum, refused=refused)
            assert refused.read() == n_marked
            assert np.array_equal(out, want_out)
            _finish_refused(sink)
            sink.reset()
            clean = tc.wrapping_groups(rng, 4, 300, marked=False).reshape(4, 1, 300).transpose(0, 2, 1).copy()
            append_reduce(ctx, sink, clean, maximum, refused=refused)
            sink.finish()
            assert_columns(sink, ctx.lib, tc.ref_reduce(reduce_groups(clean), maximum, node=21, input_id=20)[0], "clean reduce")
            assert refused.read() == n_marked
        refused.free()


# ---- 8. refusals
def _info(node=2, ids=(0, 1), consumers=1):
    return backend.LmnNodeInfo(node, (C.c_uint32 * 2)(*ids), consumers, 0, (C.c_int32 * 2)(-1, -1))


def check_refusals(ctx, other_device=None):
    """every refusal of the contract with its code, the count unchanged behind each, and a later finish that yields exactly
    the earlier content; append after finish; the capacity reached exactly and passed by one row.
    other_device: a second device of the machine (None: there is none, the case cannot be built)."""
    L, lib = ctx.lib.lib, ctx.lib
    a0, b0 = in_contract(ADD)
    n = 20
    a, b = tiled(a0, n), tiled(b0, n)
    da, db = ctx.upload(_i32(a)), ctx.upload(_i32(b))
    out = ctx.alloc(4 * 64)
    info = _info()
    content = tc.ref_elementwise(ADD, a, b)[0]
    view_bad = LmnView.make((3, 5), (5, 1), 0)          # 15 elements, not n
    err = lambda c: L.lmn_last_error(c.handle).decode()

    with ctx.row_sink(ADD, 2 * n) as sink, ctx.row_sink(MUL, n) as mul_sink, ctx.row_sink(SUM, n) as sum_sink, \
            ctx.row_sink(CONTIG, n) as contig_sink, ctx.row_sink(EXP2, n) as lut_sink:
        append(ctx, sink, ADD, a, b)
        assert sink.n_rows == n
        ew = lambda s, kind=ADD, lhs=da.ptr, rhs=db.ptr, m=n, lv=None, inf=info, c=ctx: L.lmn_rows_append_elementwise_v(
            c.handle, s, kind, lhs, C.byref(lv) if lv is not None else None, rhs, None, m, C.byref(inf) if inf else None, None,
            out.ptr, None)
        rg = (backend.LmnRange * 1)(backend.LmnRange(0, 15))
        cases = [
            ("null rows", lambda: ew(None), ERR_INVALID, "rows"),
            ("kind", lambda: ew(mul_sink.handle), ERR_INVALID, "rows"),
            ("kind, reduce", lambda: L.lmn_rows_append_reduce(ctx.handle, sink.handle, 0, da.ptr, 1, n, 1, C.byref(info), out.ptr, None),
             ERR_INVALID, "rows"),
            ("kind, max into a sum sink", lambda: L.lmn_rows_append_reduce(ctx.handle, sum_sink.handle, 1, da.ptr, 1, n, 1, C.byref(info),
                                                                         out.ptr, None), ERR_INVALID, "rows"),
            ("kind, contiguous", lambda: L.lmn_rows_append_contiguous(ctx.handle, sink.handle, da.ptr, n, None, n, C.byref(info), out.ptr,
                                                                     None), ERR_INVALID, "rows"),
            ("kind, lut", lambda: L.lmn_rows_append_lut_ranges(ctx.handle, sink.handle, EXP2, da.ptr, None, n, C.byref(info), db.ptr, rg, 1,
                                                               out.ptr, out.ptr, None), ERR_INVALID, "rows"),
            ("capacity", lambda: ew(sink.handle, m=n + 1, lhs=da.ptr), ERR_INVALID, "capacity"),
            ("n == 0", lambda: ew(sink.handle, m=0), ERR_EMPTY, "EmptyTrace"),
            ("view", lambda: ew(sink.handle, lv=view_bad), ERR_INVALID, "view"),
            ("null lhs_dev", lambda: ew(sink.handle, lhs=None), ERR_INVALID, "lhs_dev"),
            ("null rhs of a binary kind", lambda: ew(sink.handle, rhs=None), ERR_INVALID, "right operand"),
            ("null info", lambda: ew(sink.handle, inf=None), ERR_INVALID, "info"),
            ("not elementwise", lambda: ew(sum_sink.handle, kind=SUM), ERR_INVALID, "elementwise"),
            ("reduce dim 0", lambda: L.lmn_rows_append_reduce(ctx.handle, sum_sink.handle, 0, da.ptr, 1, 0, 1, C.byref(info), out.ptr, None),
             ERR_EMPTY, "EmptyTrace"),
            ("contiguous view leaves the buffer", lambda: L.lmn_rows_append_contiguous(
                ctx.handle, contig_sink.handle, da.ptr, 10, C.byref(view_bad), 15, C.byref(info), out.ptr, None), ERR_INVALID, "view"),
            ("lut kind", lambda: L.lmn_rows_append_lut_ranges(ctx.handle, lut_sink.handle, ADD, da.ptr, None, n, C.byref(info), db.ptr, rg,
                                                              1, out.ptr, out.ptr, None), ERR_INVALID, "Sin, Exp2 or Log2"),
            ("lut ranges", lambda: L.lmn_rows_append_lut_ranges(ctx.handle, lut_sink.handle, EXP2, da.ptr, None, n, C.byref(info), db.ptr,
                                                                rg, 0, out.ptr, out.ptr, None), ERR_INVALID, "ranges"),
            ("lut null mult_dev", lambda: L.lmn_rows_append_lut_ranges(ctx.handle, lut_sink.handle, EXP2, da.ptr, None, n, C.byref(info),
                                                                       db.ptr, rg, 1, None, out.ptr, None), ERR_INVALID, "mult_dev"),
        ]
        for name, call, code, word in cases:
            rc = int(call())
            assert rc == code, (name, rc, err(ctx))
            assert word in err(ctx) and "lmn_rows_append" in err(ctx), (name, err(ctx))
            assert [s.n_rows for s in (sink, mul_sink, sum_sink, contig_sink, lut_sink)] == [n, 0, 0, 0, 0], name
        if other_device is not None:
            other = backend.Context(other_device, None, lib)
            try:
                oa, ob_ = other.upload(_i32(a)), other.upload(_i32(b))
                rc = int(ew(sink.handle, lhs=oa.ptr, rhs=ob_.ptr, c=other))
                assert rc == ERR_INVALID and "device" in err(other), (rc, err(other))
                assert sink.n_rows == n
                oa.free()
                ob_.free()
            finally:
                other.close()
        # the capacity reached exactly is accepted, one row more is refused
        append(ctx, sink, ADD, a, b)
        assert sink.n_rows == 2 * n
        assert int(ew(sink.handle, m=1)) == ERR_INVALID and "capacity" in err(ctx)
        sink.finish()
        assert_columns(sink, lib, np.concatenate([content, content]), "nothing was written by a refused call")
        # append after finish without reset
        assert int(ew(sink.handle, m=1)) == ERR_INVALID and "lmn_rows_reset" in err(ctx)
        assert sink.n_rows == 2 * n
        sink.reset()
        append(ctx, sink, ADD, a, b)
        sink.finish()
        assert_columns(sink, lib, content, "after reset")
    for buf in (da, db, out):
        buf.free()


def check_batch_library_refuses(batch_lib):
    """libluminair_hip_batch.so exports the entry points; no sink can exist there, and they refuse in the same way"""
    ctx = backend.Context(0, None, batch_lib)
    try:
        L = batch_lib.lib
        h = C.c_void_p()
        assert int(L.lmn_rows_open(ctx.handle, ADD, 16, C.byref(h))) == ERR_INVALID and not h.value
        da = ctx.upload(np.zeros(16, dtype=np.int32))
        info = _info()
        rg = (backend.LmnRange * 1)(backend.LmnRange(0, 15))
        calls = [lambda: L.lmn_rows_append_elementwise_v(ctx.handle, None, ADD, da.ptr, None, da.ptr, None, 16, C.byref(info), None, None, None),
                 lambda: L.lmn_rows_append_contiguous(ctx.handle, None, da.ptr, 16, None, 16, C.byref(info), None, None),
                 lambda: L.lmn_rows_append_reduce(ctx.handle, None, 0, da.ptr, 1, 16, 1, C.byref(info), None, None),
                 lambda: L.lmn_rows_append_lut_ranges(ctx.handle, None, EXP2, da.ptr, None, 16, C.byref(info), da.ptr, rg, 1, da.ptr, None,
                                                      None)]
        for call in calls:
            assert int(call()) == ERR_INVALID
            assert "rows" in L.lmn_last_error(ctx.handle).decode()
        da.free()
    finally:
        ctx.close()


# ---- 9. compaction
def check_compaction(lib, device=0):
    """sinks opened for 1000 rows that receive 20 (Add) and 40 (Inputs): finished strides 32 and 64, the right content, and the
    proof of the row form's tables (the pinned variant: the Inputs component has a claim slot there)"""
    cfg = lib.default_config()
    cfg.protocol_variant = backend.VARIANT_PINNED
    ctx = backend.Context(device, cfg, lib)
    a0, b0 = in_contract(ADD)
    a, b = tiled([v for v in a0 if abs(v) < 1 << 20], 20), tiled([v for v in b0 if abs(v) < 1 << 20], 20, 3)
    da, db = ctx.upload(_i32(a)), ctx.upload(_i32(b))
    ins = dict(input_ids=(), input_mults=(), num_consumers=1)
    add = dict(node_id=2, input_ids=(0, 1), num_consumers=0, is_final_output=True)
    # the row form
    rows_in = ctx.alloc(40 * 7 * 4)
    _, ta = ctx.trace_elementwise(INPUTS, da, None, 20, node_id=0, rows=rows_in, **ins)
    _, tb = ctx.trace_elementwise(INPUTS, db, None, 20, node_id=1, rows=rows_in, row_offset=20, **ins)
    rows_add, to = ctx.trace_elementwise(ADD, ta, tb, 20, **add)
    want = ctx.prove_tables([(ADD, rows_add, 20), (INPUTS, rows_in, 40)])
    want_add, want_in = ctx.download(rows_add).reshape(20, 15), ctx.download(rows_in).reshape(40, 7)
    tc._assert_rows(want_add, tc.ref_elementwise(ADD, a, b, final=True)[0], "row form")
    with ctx.row_sink(ADD, 1000) as s_add, ctx.row_sink(INPUTS, 1000) as s_in:
        ctx.trace_elementwise(INPUTS, da, None, 20, node_id=0, out=ta, sink=s_in, **ins)
        ctx.trace_elementwise(INPUTS, db, None, 20, node_id=1, out=tb, sink=s_in, **ins)
        ctx.trace_elementwise(ADD, ta, tb, 20, out=to, sink=s_add, **add)
        s_add.finish()
        s_in.finish()
        assert s_add.columns().shape == (15, 32) and s_in.columns().shape == (7, 64)
        assert_columns(s_add, ctx.lib, want_add, "compacted Add")
        assert_columns(s_in, ctx.lib, want_in, "compacted Inputs")
        assert ctx.prove_tables([(ADD, s_add, 20), (INPUTS, s_in, 40)]) == want
        rep = ctx.check_trace([(ADD, s_add, 20), (INPUTS, s_in, 40)])
        assert rep.ok, rep.summary
    for buf in (da, db, rows_in, rows_add, ta, tb, to):
        buf.free()
    ctx.close()


# ---- 10. end to end
def add_graph(ctx, n, seed):
    from luminair_amd.graph import DeviceGraph
    rng = np.random.default_rng(seed)
    g = DeviceGraph(ctx)
    x, y = g.input(rng.integers(-(1 << 20), 1 << 20, size=n)), g.input(rng.integers(-(1 << 20), 1 << 20, size=n))
    g.output(g.add(x, y))
    return g


def check_end_to_end(lib, device=0, add_rows=1 << 13):
    """`gen_trace(columns=True)` against `gen_trace()` on edge_graph and on an Add graph of 2^13 elements, at log_blowup 1 and
    2: the same proof bytes, `lmn_trace_check` ok on the sink tables, and a second pie through the first one's sinks"""
    for log_blowup in (1, 2):
        cfg = lib.default_config()
        cfg.protocol_variant = backend.VARIANT_PINNED
        cfg.log_blowup = log_blowup
        ctx = backend.Context(device, cfg, lib)
        try:
            for make in (tc.edge_graph, lambda c: add_graph(c, add_rows, 1)):
                g = make(ctx)
                tables, luts, bufs = g.gen_trace()
                want = ctx.prove_tables(tables, luts)
                for b in bufs:
                    b.free()
                tables, luts, bufs = g.gen_trace(columns=True)
                sinks = g.sinks_of(bufs)
                assert sorted(sinks) == sorted(k for k, r, _ in tables if isinstance(r, backend.RowSink))
                assert all(isinstance(r, backend.RowSink) == (k not in (4, 10, 12, 14)) for k, r, _ in tables)
                assert [k for k, _, _ in tables] == sorted(k for k, _, _ in tables)
                rep = ctx.check_trace(tables, luts)
                assert rep.ok, rep.summary
                assert ctx.prove_tables(tables, luts) == want, "log_blowup %d" % log_blowup
                for b in bufs:
                    b.free()
                assert all(s.handle is None for s in sinks.values())       # freeing the buffers closed the sinks
            # a second pie of the same shape through the first one's sinks
            g1, g2 = add_graph(ctx, 300, 1), add_graph(ctx, 300, 2)
            t1, l1, b1 = g1.gen_trace(columns=True)
            p1 = ctx.prove_tables(t1, l1)
            sinks = g1.sinks_of(b1)
            for b in b1:
                if b.__class__.__name__ != "_SinkLease":
                    b.free()
            t2, l2, b2 = g2.gen_trace(columns=True, sinks=sinks)
            assert g2.sinks_of(b2) == sinks                                 # reset and reused, not reopened
            p2 = ctx.prove_tables(t2, l2)
            for b in b2:
                b.free()
            t2r, l2r, b2r = g2.gen_trace()
            assert p2 == ctx.prove_tables(t2r, l2r) and p2 != p1
            for b in b2r:
                b.free()
            lib.verify(p2, backend.VARIANT_PINNED, config=cfg)
        finally:
            ctx.close()


def check_graph_refuses(lib, device=0):
    """a graph with an element outside the contract: the dry run's ValueError, with the count"""
    from luminair_amd.graph import DeviceGraph
    cfg = lib.default_config()
    cfg.protocol_variant = backend.VARIANT_PINNED
    ctx = backend.Context(device, cfg, lib)
    g = DeviceGraph(ctx)
    g.output(g.recip(g.input(np.array([4096, 0, -5, 7], dtype=np.int64))))
    try:
        g.gen_trace(columns=True)
    except ValueError as e:
        assert "2 elements refused" in str(e), e
    else:
        raise AssertionError("gen_trace(columns=True) accepted Recip of 0 and of a negative value")
    g2 = add_graph(ctx, 300, 3)                   # the context is usable
    tables, luts, bufs = g2.gen_trace(columns=True)
    assert ctx.check_trace(tables, luts).ok
    for b in bufs:
        b.free()
    ctx.close()
