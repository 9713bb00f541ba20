"""Checks of float tensors in and out (`lmn_trace_inputs_float`, its many-member, sink and eval forms, `lmn_tensor_to_float`,
`DeviceGraph.input_float` / `read_float`), shared by the emulation suite (tests/test_float_io_emu.py) and the GPU suite
(tests/test_gpu_float_io.py).  Every comparison is exact equality of integers or bit patterns.

The references are independent of the code under test (nothing of luminair_amd but `backend`, for the calls themselves):
  float -> Fixed<12>:  sign * floor(abs(float64(x)) * 4096 + 0.5) in numpy f64 - exact for every accepted value; bf16 is
                       widened by bits << 16.  Refused: not finite, or a result outside [-(2^30-1), 2^30-1].
  Fixed<12> -> f32/f16: (v.astype(float64) / 4096).astype(target) - one IEEE rounding of an exact quotient.
  Fixed<12> -> bf16:    plain Python integers, round-to-nearest-even of |v| to 8 significant bits.
A refused element carries the word P in its Inputs row's val and 0 in the output tensor, and is counted."""
import ctypes as C
import functools

import numpy as np

from luminair_amd import backend
from luminair_amd.backend import LuminairBackendError

P = (1 << 31) - 1
S = 4096
R = (1 << 30) - 1
TPB = 256
INPUTS = 15
F32, F16, BF16 = 0, 1, 2
CODES = (F32, F16, BF16)
NAME = {F32: "f32", F16: "f16", BF16: "bf16"}
BITS_DT = {F32: np.uint32, F16: np.uint16, BF16: np.uint16}
SIZES = (1, 63, 64, 65, TPB - 1, TPB, TPB + 1, 4 * TPB + 3)


# ---------------------------------------------------------------------------------------------- references
def widen(code, bits):
    """the float64 value of every bit pattern (exact widening)"""
    bits = np.asarray(bits)
    with np.errstate(invalid="ignore"):          # (a signalling NaN widens to a quiet one, and numpy says so)
        if code == F32:
            return bits.astype(np.uint32).view(np.float32).astype(np.float64)
        if code == F16:
            return bits.astype(np.uint16).view(np.float16).astype(np.float64)
        return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def ref_to_fixed(code, bits):
    """(values int64 with 0 for a refused element, refused mask)"""
    x = widen(code, bits)
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.floor(np.abs(x) * 4096.0 + 0.5)
        bad = ~np.isfinite(x) | ~(y <= R)
    v = np.where(bad, 0.0, np.where(np.signbit(x), -y, y))
    return v.astype(np.int64), bad


def bf16_bits_py(v: int) -> int:
    """v / 4096 rounded once to bfloat16 (8 significant bits, to nearest even), in Python integers"""
    if v == 0:
        return 0
    m = abs(v)
    p = m.bit_length() - 1                 # m = 1.xxx * 2^p
    if p <= 7:
        q = m << (7 - p)
    else:
        r = p - 7
        q, rem, half = m >> r, m & ((1 << r) - 1), 1 << (r - 1)
        if rem > half or (rem == half and q & 1):
            q += 1
    if q == 256:
        q, p = 128, p + 1
    return (0x8000 if v < 0 else 0) | ((p - 12 + 127) << 7) | (q & 0x7f)


def ref_from_fixed(code, v):
    """the bit patterns (uint32 for f32, uint16 otherwise) of v / 4096 rounded once to the format"""
    v = np.asarray(v, dtype=np.int64)
    if code == BF16:
        return np.array([bf16_bits_py(int(x)) for x in v.reshape(-1)], dtype=np.uint16).reshape(v.shape)
    with np.errstate(over="ignore"):
        f = (v.astype(np.float64) / 4096.0).astype(np.float32 if code == F32 else np.float16)
    return f.view(BITS_DT[code])


def ref_rows(vals, bad, node, consumers, final=False):
    """the Inputs rows (prim.rs:52-88): node, idx, is_last, next_node, next_idx, val, multiplicity"""
    n = len(vals)
    idx = np.arange(n, dtype=np.int64)
    val = np.where(bad, P, np.asarray(vals, dtype=np.int64) % P)
    full = lambda x: np.full(n, x, dtype=np.int64)
    rows = np.stack([full(node), idx, (idx == n - 1).astype(np.int64), full(node), idx + 1, val,
                     full(0 if final else consumers)], axis=1)
    return rows.astype(np.uint32)


# ---------------------------------------------------------------------------------------------- bit patterns
def f32_bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def to_fixed_patterns(code):
    """the bit patterns of the float -> fixed value test (one launch each), computed once"""
    if code != F32:
        return np.arange(65536, dtype=np.uint32).astype(np.uint16)          # every pattern of the format
    rng = np.random.default_rng(20260)
    mants = [0, 1, 1 << 22, (1 << 23) - 1] + [int(m) for m in rng.integers(0, 1 << 23, size=4)]
    grid = [(s << 31) | (e << 23) | m for s in (0, 1) for e in range(256) for m in mants]
    ties = np.array([(2 * k + 1) / 8192.0 for k in range(65)], dtype=np.float32)      # exact in f32
    assert np.all(ties.astype(np.float64) * 8192 == 2 * np.arange(65) + 1)
    around = np.concatenate([ties, np.nextafter(ties, np.float32(0)), np.nextafter(ties, np.float32(1)), -ties,
                             np.nextafter(-ties, np.float32(0)), np.nextafter(-ties, np.float32(-1))])
    t13 = np.float32(2.0 ** -13)
    named = np.array([t13, -t13, np.nextafter(t13, np.float32(0)), -np.nextafter(t13, np.float32(0)),
                      2.0 ** 18 - 2.0 ** -6, -(2.0 ** 18 - 2.0 ** -6), 2.0 ** 18, -2.0 ** 18, 3e38, -3e38, np.inf, -np.inf,
                      0.0, -0.0], dtype=np.float32)
    raw = [0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffffffff, 0x7fa00000,     # quiet / signalling NaNs
           0x00000001, 0x80000001, 0x007fffff, 0x807fffff]                                        # smallest / largest denormals
    rand = rng.integers(0, 1 << 32, size=65536, dtype=np.uint64)
    return np.concatenate([np.array(grid, dtype=np.uint64), f32_bits(around).astype(np.uint64),
                           f32_bits(named).astype(np.uint64), np.array(raw, dtype=np.uint64), rand]).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def to_fixed_reference(code):
    return ref_to_fixed(code, to_fixed_patterns(code))


def shape_bits(code, n, seed=0):
    """n patterns for the shape tests: accepted values of every magnitude, with refused ones (NaN, Inf, too large) mixed in"""
    rng = np.random.default_rng(1000 * code + n + seed)
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-14, 15, size=n))).astype(np.float32)
    if code == F32:
        bits = x.view(np.uint32).copy()
        special = [0x7fc00000, 0xff800000, f32_bits(2.0 ** 18)[()], 0x80000000]
    elif code == F16:
        bits = x.astype(np.float16).view(np.uint16).copy()
        special = [0x7e00, 0xfc00, 0x7c01, 0x8000]
    else:
        bits = (x.view(np.uint32) >> 16).astype(np.uint16)
        special = [0x7fc0, 0xff80, int(f32_bits(2.0 ** 18)[()]) >> 16, 0x8000]
    for k, sp in enumerate(special):
        if n > 2 * k + 1:
            bits[(2 * k + 1) * n // 9 % n] = sp
    return bits


def clean_bits(code, n, seed=0):
    """as shape_bits without refused elements (a sink with a refused element cannot be finished and read)"""
    bits = shape_bits(code, n, seed)
    bad = ref_to_fixed(code, bits)[1]
    bits[bad] = 0x3c00 if code == F16 else 0x3f80 if code == BF16 else 0x3f800000
    return bits


# ---------------------------------------------------------------------------------------------- device helpers
class Src:
    """float bits on the device, `skew` elements into an allocation (an odd skew: a 2-byte aligned source)"""

    def __init__(self, ctx, code, bits, skew=0):
        bits = np.ascontiguousarray(bits, dtype=BITS_DT[code]).reshape(-1)
        raw = np.concatenate([np.zeros(skew, dtype=bits.dtype), bits]).view(np.uint8)
        raw = np.concatenate([raw, np.zeros(-raw.nbytes % 4, dtype=np.uint8)])
        self.buf = ctx.upload(raw)
        self.ptr = self.buf.ptr + skew * bits.dtype.itemsize
        self.n = len(bits)

    def free(self):
        self.buf.free()


class Counter:
    def __init__(self, ctx, n=1):
        self.ctx, self.buf = ctx, ctx.upload(np.zeros(n, dtype=np.uint32))

    def read(self):
        return [int(c) for c in self.ctx.download(self.buf)]

    def free(self):
        self.buf.free()


def rows_of(ctx, buf, n_rows):
    return ctx.download(buf)[:n_rows * 7].reshape(n_rows, 7)


def i32(ctx, buf, n):
    return ctx.download(buf, np.int32)[:n].astype(np.int64)


def int_operand(vals, bad):
    """what the integer form is given for the same rows: the converted integers, and a value outside the range for a
    refused element"""
    return np.where(bad, R + 1, vals).astype(np.int32)


def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d differ, first at %s: got %s, want %s"
                             % (what, len(at), got.size, tuple(at[0]), got[tuple(at[0])], want[tuple(at[0])]))


def padded_columns(lib, rows):
    size = max(16, 1 << max(len(rows) - 1, 0).bit_length())
    pad = (C.c_uint32 * 7)()
    assert lib.lib.lmn_kind_padding_row(INPUTS, pad) == 0
    full = np.tile(np.array(list(pad), dtype=np.uint32), (size, 1))
    full[:len(rows)] = rows
    return np.ascontiguousarray(full.T)


# ---------------------------------------------------------------------------------------------- 1. float -> fixed values
def check_to_fixed_values(ctx, code, with_sink=True):
    """every pattern of the set in ONE launch of each form: rows and tensor against the reference, neighbours of refused
    elements exact, the eval / many / sink counters equal to the reference's refused count"""
    bits = to_fixed_patterns(code)
    vals, bad = to_fixed_reference(code)
    n, n_bad = len(bits), int(bad.sum())
    assert n_bad > 0 and (code != F16 or n_bad == 2 * 1024), n_bad      # f16: exactly the Inf / NaN patterns
    src = Src(ctx, code, bits)
    want_rows = ref_rows(vals, bad, node=7, consumers=3)
    try:
        rows, out = ctx.trace_inputs_float(code, src.ptr, n, node_id=7, num_consumers=3)
        assert_same(rows_of(ctx, rows, n), want_rows, "%s row form: rows" % NAME[code])
        assert_same(i32(ctx, out, n), vals, "%s row form: tensor" % NAME[code])
        rows.free(), out.free()
        # eval form: tensor, range and count
        cnt, mm = Counter(ctx), ctx.alloc(8)
        out = ctx.eval_inputs_float(code, src.ptr, n, minmax=mm, refused=cnt.buf)
        assert_same(i32(ctx, out, n), vals, "%s eval form: tensor" % NAME[code])
        assert list(ctx.download(mm, np.int32)) == [int(vals.min()), int(vals.max())]
        assert cnt.read() == [n_bad]
        out.free(), mm.free(), cnt.free()
        # many form, one member
        cnt, rows, out = Counter(ctx), ctx.alloc(n * 28), ctx.alloc(n * 4)
        ctx.trace_many_inputs_float(code, src.ptr, n, 1, node_id=7, num_consumers=3, rows=rows, rows_stride=n, out=out,
                                    out_stride=n, src_stride=n, refused=cnt.buf)
        assert_same(rows_of(ctx, rows, n), want_rows, "%s many form: rows" % NAME[code])
        assert_same(i32(ctx, out, n), vals, "%s many form: tensor" % NAME[code])
        assert cnt.read() == [n_bad]
        rows.free(), out.free(), cnt.free()
        if with_sink:
            cnt, sink = Counter(ctx), ctx.row_sink(INPUTS, n)
            got, out = ctx.trace_inputs_float(code, src.ptr, n, node_id=7, num_consumers=3, sink=sink, refused=cnt.buf)
            assert got is sink and sink.n_rows == n
            assert_same(i32(ctx, out, n), vals, "%s sink form: tensor" % NAME[code])
            assert cnt.read() == [n_bad]
            try:
                sink.finish()
            except LuminairBackendError as e:
                assert e.code == backend.ERR_INVALID_ARGUMENT, e
            else:
                raise AssertionError("a sink holding refused elements finished")
            # the same launch without its refused elements: the columns, P nowhere
            keep = ~bad
            sink.reset()
            clean = Src(ctx, code, bits[keep])
            _, out2 = ctx.trace_inputs_float(code, clean.ptr, clean.n, node_id=7, num_consumers=3, sink=sink, refused=cnt.buf)
            sink.finish()
            assert_same(sink.columns(), padded_columns(ctx.lib, ref_rows(vals[keep], bad[keep], 7, 3)),
                        "%s sink form: columns" % NAME[code])
            assert cnt.read() == [n_bad]
            out.free(), out2.free(), cnt.free(), clean.free(), sink.close()
    finally:
        src.free()


# ---------------------------------------------------------------------------------------------- 2. fixed -> float values
@functools.lru_cache(maxsize=None)
def from_fixed_values(code):
    v = [0, 1, -1, 2, 3, 4095, 4096, 4097, R, -R, R - 1]
    for base in (1 << 24, 1 << 25):
        for d in (-3, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8):              # 2^24 + 1, 2^25 + 2: ties to even, down; + 3, + 6: up
            v += [base + d, -(base + d)]
    top = 65504 * S                                                    # the largest finite f16
    v += [s * (top + d) for s in (1, -1) for d in (-32 * S, -1, 0, 1, 16 * S - 1, 16 * S, 16 * S + 1, 32 * S)]   # + 16: the tie, Inf
    for k in range(0, 22):                                             # bf16 ties: 9 significant bits ending in 1
        v += [s * (m << k) for s in (1, -1) for m in (0x101, 0x103, 0x1ff, 0x17f) if (m << k) <= R]
    rng = np.random.default_rng(77 + code)
    mag = (rng.integers(1, 1 << 30, size=65536) >> rng.integers(0, 30, size=65536))      # every magnitude
    rand = np.where(rng.integers(0, 2, size=65536) == 1, -mag, mag)
    return np.concatenate([np.array(v, dtype=np.int64), rand]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def from_fixed_reference(code):
    return ref_from_fixed(code, from_fixed_values(code))


def check_from_fixed_values(ctx, code):
    v = from_fixed_values(code)
    want = from_fixed_reference(code)
    if code == F16:
        f = want.view(np.float16)
        assert np.isinf(f[v == 65520 * S]).all() and np.isfinite(f[v == 65520 * S - 1]).all()
    src = ctx.upload(v)
    dst = ctx.tensor_to_float(code, src, len(v))
    got = ctx.download(dst, BITS_DT[code])[:len(v)]
    assert_same(got, want, "tensor_to_float %s" % NAME[code])
    src.free(), dst.free()


# ---------------------------------------------------------------------------------------------- 3. shapes
def check_shapes(ctx, code, sizes=SIZES):
    """every size through the row form (behind another node's rows), the sink form (behind a host push) and the eval form;
    rows and tensors against the reference AND against lmn_trace_elementwise(Inputs) on the reference integers; 2-byte
    sources at an odd element offset"""
    other = ref_rows(np.array([5, -6, 7]), np.zeros(3, dtype=bool), node=1, consumers=2)
    for n in sizes:
        skew = 0 if code == F32 else 1
        bits = shape_bits(code, n)
        vals, bad = ref_to_fixed(code, bits)
        src = Src(ctx, code, bits, skew)
        want = np.concatenate([other, ref_rows(vals, bad, node=4, consumers=2, final=n % 2 == 0)])
        what = "%s n=%d" % (NAME[code], n)
        # row form at row_offset 3 of a table whose first rows another node wrote
        table = ctx.upload(np.concatenate([other.reshape(-1), np.full(n * 7, 0xAAAAAAAA, dtype=np.uint32)]))
        _, out = ctx.trace_inputs_float(code, src.ptr, n, node_id=4, num_consumers=2, is_final_output=n % 2 == 0, rows=table,
                                        row_offset=3)
        got_rows, got_out = rows_of(ctx, table, n + 3), i32(ctx, out, n)
        assert_same(got_rows, want, what + " row form: rows")
        assert_same(got_out, vals, what + " row form: tensor")
        # the integer form on the converted integers: the same words
        table_i = ctx.upload(np.concatenate([other.reshape(-1), np.full(n * 7, 0xAAAAAAAA, dtype=np.uint32)]))
        ints = ctx.upload(int_operand(vals, bad))
        _, out_i = ctx.trace_elementwise(INPUTS, ints, None, n, node_id=4, input_ids=(), num_consumers=2, input_mults=(),
                                         is_final_output=n % 2 == 0, rows=table_i, row_offset=3)
        assert_same(got_rows, rows_of(ctx, table_i, n + 3), what + ": float form vs integer form, rows")
        assert_same(got_out, i32(ctx, out_i, n), what + ": float form vs integer form, tensor")
        for b in (table, out, table_i, out_i):
            b.free()
        # eval form
        cnt, mm = Counter(ctx), ctx.alloc(8)
        out = ctx.eval_inputs_float(code, src.ptr, n, minmax=mm, refused=cnt.buf)
        assert_same(i32(ctx, out, n), vals, what + " eval form: tensor")
        assert list(ctx.download(mm, np.int32)) == [int(vals.min()), int(vals.max())], what
        assert cnt.read() == [int(bad.sum())], what
        out_e = ctx.eval_elementwise(INPUTS, ints, None, n, minmax=mm)
        assert_same(i32(ctx, out, n), i32(ctx, out_e, n), what + ": float eval vs integer eval")
        for b in (out, out_e, mm, ints):
            b.free()
        cnt.free()
        src.free()
        # sink form behind a host push (values without refused elements: the finished columns are read)
        bits = clean_bits(code, n)
        vals, bad = ref_to_fixed(code, bits)
        assert not bad.any()
        src, cnt = Src(ctx, code, bits, skew), Counter(ctx)
        sink, sink_i = ctx.row_sink(INPUTS, n + 3), ctx.row_sink(INPUTS, n + 3)
        sink.push(other), sink_i.push(other)
        _, out = ctx.trace_inputs_float(code, src.ptr, n, node_id=4, num_consumers=2, sink=sink, refused=cnt.buf)
        ints = ctx.upload(vals.astype(np.int32))
        _, out_i = ctx.trace_elementwise(INPUTS, ints, None, n, node_id=4, input_ids=(), num_consumers=2, input_mults=(),
                                         sink=sink_i, refused=cnt.buf)
        assert sink.n_rows == n + 3
        sink.finish(), sink_i.finish()
        cols = sink.columns()
        assert_same(cols, padded_columns(ctx.lib, np.concatenate([other, ref_rows(vals, bad, 4, 2)])), what + " sink form: columns")
        assert_same(cols, sink_i.columns(), what + ": float sink vs integer sink")
        assert_same(i32(ctx, out, n), vals, what + " sink form: tensor")
        assert cnt.read() == [0]
        for b in (out, out_i, ints, src, cnt):
            b.free()
        sink.close(), sink_i.close()


def check_many(ctx, code, n=TPB + 1):
    """1 and 3 members, a per-member source and a shared one (stride 0, with the shared-output rule), against the reference
    and against lmn_trace_many_elementwise_v on the reference integers"""
    skew = 0 if code == F32 else 1
    for members in (1, 3):
        for shared in (False, True):
            per = 1 if shared else members
            bits = np.concatenate([shape_bits(code, n, seed=m) for m in range(per)])
            vals, bad = ref_to_fixed(code, bits)
            src = Src(ctx, code, bits, skew)
            stride = n + 5                                   # rows per member's table: 2 rows in front, 3 behind
            cnt, cnt_i = Counter(ctx, members), Counter(ctx, members)
            fill = np.full(members * stride * 7, 0xAAAAAAAA, dtype=np.uint32)
            rows, rows_i = ctx.upload(fill), ctx.upload(fill)
            n_out = n if shared else members * n
            out, out_i = ctx.upload(np.full(n_out, 0x55555555, dtype=np.uint32)), ctx.upload(np.full(n_out, 0x55555555, dtype=np.uint32))
            kw = dict(node_id=9, num_consumers=1, rows_stride=stride, row_offset=2, out_stride=0 if shared else n)
            ctx.trace_many_inputs_float(code, src.ptr, n, members, rows=rows, out=out, src_stride=0 if shared else n,
                                        refused=cnt.buf, **kw)
            ints = ctx.upload(int_operand(vals, bad))
            ctx.trace_many_elementwise(INPUTS, ints, None, n, members, input_ids=(), input_mults=(), rows=rows_i, out=out_i,
                                       lhs_stride=0 if shared else n, refused=cnt_i.buf, **kw)
            what = "%s many form, %d members, %s source" % (NAME[code], members, "shared" if shared else "per-member")
            got, got_i = ctx.download(rows).reshape(members, stride, 7), ctx.download(rows_i).reshape(members, stride, 7)
            assert_same(got, got_i, what + ": float form vs integer form, rows")
            assert_same(ctx.download(out), ctx.download(out_i), what + ": float form vs integer form, tensor")
            assert cnt.read() == cnt_i.read()
            for m in range(members):
                sl = slice(0, n) if shared else slice(m * n, (m + 1) * n)
                assert_same(got[m, 2:2 + n], ref_rows(vals[sl], bad[sl], 9, 1), what + ": member %d rows" % m)
                assert (got[m, :2] == 0xAAAAAAAA).all() and (got[m, 2 + n:] == 0xAAAAAAAA).all(), what + ": rows outside the node"
                assert cnt.read()[m] == int(bad[sl].sum()), what
            assert_same(i32(ctx, out, n_out), vals, what + ": tensor")
            for b in (src, cnt, cnt_i, rows, rows_i, out, out_i, ints):
                b.free()


# ---------------------------------------------------------------------------------------------- 4. argument errors
def _refused(fn, code, *names):
    try:
        fn()
    except LuminairBackendError as e:
        assert e.code == code, (e, code)
        assert all(nm in str(e) for nm in names), (str(e), names)
    else:
        raise AssertionError("accepted: expected code %d naming %s" % (code, names))


def check_argument_errors(ctx, with_sink=True):
    """every refusal gives its code and names its argument, and nothing is launched: rows pre-filled with a pattern stay
    untouched, a sink keeps its count"""
    INV, EMPTY = backend.ERR_INVALID_ARGUMENT, backend.ERR_EMPTY_TRACE
    n = 8
    src = Src(ctx, F32, f32_bits(np.arange(n, dtype=np.float32)))
    fill = np.full(4 * n * 7, 0xAAAAAAAA, dtype=np.uint32)
    rows, out = ctx.upload(fill), ctx.upload(np.full(4 * n, 0x55555555, dtype=np.uint32))
    cnt = Counter(ctx, 4)
    row = lambda dtype, ptr, n_: (lambda: ctx.trace_inputs_float(dtype, ptr, n_, node_id=1, num_consumers=1, rows=rows, out=out))
    many = lambda dtype, ptr, n_, members=2, **kw: (lambda: ctx.trace_many_inputs_float(
        dtype, ptr, n_, members, node_id=1, num_consumers=1, rows=rows, out=out, refused=cnt.buf,
        **dict(dict(rows_stride=n, out_stride=n, src_stride=n), **kw)))
    ev = lambda dtype, ptr, n_: (lambda: ctx.eval_inputs_float(dtype, ptr, n_, out=out, refused=cnt.buf))
    forms = [("lmn_trace_inputs_float", row, EMPTY), ("lmn_trace_many_inputs_float", many, EMPTY),
             ("lmn_eval_inputs_float", ev, INV)]
    sink = None
    if with_sink:
        sink = ctx.row_sink(INPUTS, 4 * n)
        sink.push(ref_rows(np.array([1, 2]), np.zeros(2, dtype=bool), 0, 1))
        app = lambda dtype, ptr, n_: (lambda: ctx.trace_inputs_float(dtype, ptr, n_, node_id=1, num_consumers=1, sink=sink, out=out,
                                                                     refused=cnt.buf))
        forms.append(("lmn_rows_append_inputs_float", app, EMPTY))
    for call, form, empty_code in forms:
        _refused(form(3, src.ptr, n), INV, call, "dtype")
        _refused(form(0xffffffff, src.ptr, n), INV, call, "dtype")
        _refused(form(F32, None, n), INV, call, "src_dev")
        _refused(form(F32, src.ptr, 0), empty_code, call, "n is 0")
        _refused(form(F32, src.ptr + 2, n - 1), INV, call, "src_dev", "aligned")
        _refused(form(F16, src.ptr + 1, n), INV, call, "src_dev", "aligned")
        _refused(form(BF16, src.ptr + 3, n), INV, call, "src_dev", "aligned")
        _refused(form(F32, src.ptr, 1 << 31), INV, call, "too large")
    # the sibling forms' own errors
    _refused(many(F32, src.ptr, n, rows_stride=n - 1), INV, "lmn_trace_many_inputs_float", "rows_member_stride")
    _refused(many(F32, src.ptr, n, members=backend.TRACE_MANY_MAX + 1), INV, "lmn_trace_many_inputs_float", "n_members")
    _refused(many(F32, src.ptr, n, out_stride=0), INV, "lmn_trace_many_inputs_float", "out_member_stride")
    _refused(many(F32, src.ptr, n, out_stride=n - 1), INV, "lmn_trace_many_inputs_float", "out_member_stride")
    ctx.trace_many_inputs_float(F32, src.ptr, n, 0, node_id=1, num_consumers=1, rows=rows, rows_stride=0, out=out, out_stride=0)
    _refused(lambda: ctx.tensor_to_float(3, rows, n, dst=out), INV, "lmn_tensor_to_float", "dtype")
    _refused(lambda: ctx.tensor_to_float(F32, None, n, dst=out), INV, "lmn_tensor_to_float", "src_dev")
    _refused(lambda: ctx.tensor_to_float(F32, rows, 0, dst=out), INV, "lmn_tensor_to_float", "n is 0")
    _refused(lambda: ctx.tensor_to_float(F16, rows, n, dst=out.ptr + 1), INV, "lmn_tensor_to_float", "dst_dev", "aligned")
    _refused(lambda: ctx.tensor_to_float(F32, rows, n, dst=out.ptr + 2), INV, "lmn_tensor_to_float", "dst_dev", "aligned")
    if with_sink:
        wrong = ctx.row_sink(0, n)
        _refused(lambda: ctx.trace_inputs_float(F32, src.ptr, n, node_id=1, num_consumers=1, sink=wrong, out=out), INV,
                 "lmn_rows_append_inputs_float", "rows")
        _refused(lambda: ctx.trace_inputs_float(F32, src.ptr, 4 * n, node_id=1, num_consumers=1, sink=sink, out=out), INV,
                 "lmn_rows_append_inputs_float", "rows", "capacity")
        assert sink.n_rows == 2 and wrong.n_rows == 0
        sink.close(), wrong.close()
    assert (ctx.download(rows) == 0xAAAAAAAA).all() and (ctx.download(out) == 0x55555555).all()
    assert cnt.read() == [0] * 4
    for b in (src, rows, out, cnt):
        b.free()


def check_batch_library_sink_refuses(ctx):
    """libluminair_hip_batch.so exports the sink form, and it refuses as every lmn_rows_append_* does there"""
    src = Src(ctx, F32, f32_bits([1.0]))
    info = backend.LmnNodeInfo(1, (C.c_uint32 * 2)(0, 0), 1, 0, (C.c_int32 * 2)(0, 0))
    rc = ctx.lib.lib.lmn_rows_append_inputs_float(ctx.handle, None, F32, src.ptr, 1, C.byref(info), None, None)
    assert rc == backend.ERR_INVALID_ARGUMENT
    text = ctx.lib.lib.lmn_last_error(ctx.handle).decode()
    assert "lmn_rows_append_inputs_float" in text and "batch library" in text, text
    src.free()


# ---------------------------------------------------------------------------------------------- 5. the host mirrors
def check_host_mirrors():
    """luminair_amd.to_fixed / from_fixed against the same references"""
    import luminair_amd
    for code in CODES:
        bits = to_fixed_patterns(code)
        vals, bad = to_fixed_reference(code)
        arg = bits.view(np.float32) if code == F32 else bits.view(np.float16) if code == F16 else bits
        refused = []
        got = luminair_amd.to_fixed(arg, backend.BF16 if code == BF16 else None, refused=refused)
        assert got.dtype == np.int32
        assert_same(got.astype(np.int64), vals, "to_fixed %s" % NAME[code])
        assert_same(np.array(refused), np.flatnonzero(bad), "to_fixed %s: refused" % NAME[code])
        try:
            luminair_amd.to_fixed(arg, backend.BF16 if code == BF16 else None)
        except ValueError:
            pass
        else:
            raise AssertionError("to_fixed accepted refused elements")
        keep = ~bad
        assert_same(luminair_amd.to_fixed(arg[keep], backend.BF16 if code == BF16 else None).astype(np.int64), vals[keep],
                    "to_fixed %s, accepted only" % NAME[code])
        v = from_fixed_values(code)
        dt = {F32: np.float32, F16: np.float16, BF16: "bfloat16"}[code]
        got = luminair_amd.from_fixed(v, dt)
        assert_same(got.view(BITS_DT[code]), from_fixed_reference(code), "from_fixed %s" % NAME[code])
    assert luminair_amd.from_fixed(np.array([[4096, -2048]])).tolist() == [[1.0, -0.5]]
    assert luminair_amd.to_fixed(np.array([[1.0, -0.5]], dtype=np.float32)).tolist() == [[4096, -2048]]


# ---------------------------------------------------------------------------------------------- 6. end to end
def _bf16_tensor(bits):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16)).view(torch.bfloat16)


def graph_inputs(shape=(7, 41), seed=5):
    """float bit patterns of the three dtypes - more than one block of elements, |a * b + c| <= 0.5 so that the Sin LUT the
    settings derive from the converted values stays at 2^13 rows - and their reference integers"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.5, 0.5, size=shape).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, size=shape).astype(np.float16)
    c = (rng.uniform(-0.25, 0.25, size=shape).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    ints = [ref_to_fixed(F32, a.view(np.uint32))[0], ref_to_fixed(F16, b.view(np.uint16))[0], ref_to_fixed(BF16, c)[0]]
    return (a, b, c), [v.reshape(shape) for v in ints]


def build_graph(ctx, inputs, floats, to_device=None):
    """sum over axis 1 of sin(a * b + c); floats: input_float of the three dtypes (bf16 as a torch tensor; to_device: every
    input as a torch tensor produced on the device), else input() of the integers"""
    from luminair_amd.graph import DeviceGraph
    g = DeviceGraph(ctx)
    if floats:
        a, b, c = inputs
        c = _bf16_tensor(c).reshape(a.shape)
        if to_device is not None:
            import torch
            a, b, c = (to_device(torch.from_numpy(x) if isinstance(x, np.ndarray) else x) for x in (a, b, c))
        ta, tb, tcc = g.input_float(a), g.input_float(b), g.input_float(c)
    else:
        ta, tb, tcc = (g.input(v) for v in inputs)
    y = g.sum_reduce(g.sin(g.add(g.mul(ta, tb), tcc)), axis=1)
    g.output(y)
    return g, y


def _settings_key(s):
    return {k: (list(v.layout.ranges), v.layout.log_size) for k, v in (s.layouts or {}).items()}


def check_end_to_end(lib, device=0, to_device=None):
    """the float graph through gen_circuit_settings (host and device), gen_trace (rows and columns), prove and verify: the
    settings, every table and the proof bytes equal those of the same graph built from the reference integers; read_float of
    the output equals the reference"""
    cfg = lib.default_config()
    cfg.protocol_variant = backend.VARIANT_PINNED
    ctx = backend.Context(device, cfg, lib)
    try:
        floats, ints = graph_inputs()
        gi, yi = build_graph(ctx, ints, False)
        si = gi.gen_circuit_settings()
        tables_i, luts_i, bufs_i = gi.gen_trace()
        words_i = [(k, n, ctx.download(b)) for k, b, n in tables_i]
        proof_i = ctx.prove_tables(tables_i, luts_i)
        y_ref = gi.read(yi).astype(np.int64)
        lib.verify(proof_i, backend.VARIANT_PINNED)
        for b in bufs_i:
            b.free()
        for dev_settings in (False, True):
            gf, yf = build_graph(ctx, floats, True, to_device)
            sf = gf.gen_circuit_settings(device=dev_settings)
            assert _settings_key(sf) == _settings_key(si), "settings (device=%s)" % dev_settings
            if dev_settings:
                assert_same(gf.read(yf), y_ref, "dry_run_device: output")
            tables, luts, bufs = gf.gen_trace()
            assert [(k, n) for k, _, n in tables] == [(k, n) for k, n, _ in words_i]
            for (k, b, n), (_, _, want) in zip(tables, words_i):
                assert_same(ctx.download(b), want, "table of kind %d" % k)
            if not dev_settings:
                assert ctx.prove_tables(tables, luts) == proof_i, "proof bytes, row form"
            assert_same(gf.read(yf), y_ref, "output tensor")
            for code in CODES:
                dt = {F32: np.float32, F16: np.float16, BF16: "bfloat16"}[code]
                got = gf.read_float(yf, dtype=dt)
                assert got.shape == yf.shape
                assert_same(got.view(BITS_DT[code]), ref_from_fixed(code, y_ref), "read_float %s" % NAME[code])
            for b in bufs:
                b.free()
            if dev_settings:
                tables, luts, bufs = gf.gen_trace(columns=True)
                assert ctx.prove_tables(tables, luts) == proof_i, "proof bytes, column form"
                for b in bufs:
                    b.free()
        # a refused element fails the column form as the dry run does, and the host dry run names it
        bad = (floats[0].copy(), floats[1], floats[2])
        bad[0][1, 2] = np.nan
        gb, _ = build_graph(ctx, bad, True, to_device)
        for run in (gb.gen_circuit_settings, lambda: gb.gen_circuit_settings(device=True)):
            try:
                run()
            except ValueError:
                pass
            else:
                raise AssertionError("a NaN input passed the dry run")
    finally:
        ctx.close()


def check_many_end_to_end(lib, device=0, to_device=None, members=3, width=70):
    """gen_trace_many with float feeds: the pies equal those of integer feeds word for word; the member holding a NaN is
    counted and its pie alone is refused by the prover"""
    from luminair_amd.graph import DeviceGraph
    cfg = lib.default_config()
    cfg.protocol_variant = backend.VARIANT_PINNED
    ctx = backend.Context(device, cfg, lib)
    try:
        rng = np.random.default_rng(9)
        x = rng.standard_normal((members, width)).astype(np.float32)
        x[1, 5] = np.nan
        w = rng.standard_normal(width).astype(np.float16)
        c = ((rng.standard_normal(width)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        xv, xbad = ref_to_fixed(F32, x.view(np.uint32))
        wv, cv = ref_to_fixed(F16, w.view(np.uint16))[0], ref_to_fixed(BF16, c)[0]

        def build(floats):
            g = DeviceGraph(ctx)
            if floats:
                conv = (lambda t: to_device(t)) if to_device is not None else (lambda t: t)
                import torch
                tx = g.input_float(x[0], per_member=True)
                tw = g.input_float(conv(torch.from_numpy(w)) if to_device is not None else w)
                tcc = g.input_float(conv(_bf16_tensor(c)))
                feed = conv(torch.from_numpy(x)) if to_device is not None else x
            else:
                tx, tw, tcc = g.input(xv[0], per_member=True), g.input(wv), g.input(cv)
                feed = np.where(xbad, R + 1, xv)
            y = g.sum_reduce(g.add(g.mul(tx, tw), tcc), axis=0)
            g.output(y)
            return g, tx, y, feed
        gi, txi, yi, feed_i = build(False)
        pies_i, luts_i, bufs_i, refused_i = gi.gen_trace_many(members, {txi: feed_i})
        gf, txf, yf, feed_f = build(True)
        pies_f, luts_f, bufs_f, refused_f = gf.gen_trace_many(members, {txf: feed_f})
        assert refused_f == refused_i == [0, 1, 0], (refused_f, refused_i)
        for m in range(members):
            assert [(k, n) for k, _, n in pies_f[m]] == [(k, n) for k, _, n in pies_i[m]]
            for (k, bf, n), (_, bi, _) in zip(pies_f[m], pies_i[m]):
                assert_same(ctx.download(bf), ctx.download(bi), "member %d, table of kind %d" % (m, k))
            assert_same(gf.read(yf, m), gi.read(yi, m), "member %d output" % m)
            assert_same(gf.read_float(yf, m).view(np.uint32), ref_from_fixed(F32, gi.read(yi, m)), "member %d read_float" % m)
            if m == 1:
                _refused(lambda: ctx.prove_tables(pies_f[m], luts_f), backend.ERR_INVALID_ARGUMENT)
            else:
                proof = ctx.prove_tables(pies_f[m], luts_f)
                lib.verify(proof, backend.VARIANT_PINNED)
                assert proof == ctx.prove_tables(pies_i[m], luts_i), "member %d proof" % m
        for b in bufs_i + bufs_f:
            b.free()
        # a feed of another dtype than its input is refused
        try:
            gf.gen_trace_many(members, {txf: x.astype(np.float16)})
        except ValueError:
            pass
        else:
            raise AssertionError("a float16 feed for a float32 input was accepted")
    finally:
        ctx.close()


def check_read_float_device(lib, device=0):
    """read_float(device=True): a torch tensor on the context's device, equal to the reference bit for bit"""
    import torch
    ctx = backend.Context(device, None, lib)
    try:
        from luminair_amd.graph import DeviceGraph
        v = from_fixed_values(F32)[:4099]
        g = DeviceGraph(ctx)
        t = g.input(v)
        g.output(t)
        _, _, bufs = g.gen_trace()
        for code, tdt, idt in ((F32, torch.float32, torch.int32), (F16, torch.float16, torch.int16), (BF16, torch.bfloat16, torch.int16)):
            got = g.read_float(t, dtype=tdt, device=True)
            assert got.is_cuda and got.dtype == tdt and tuple(got.shape) == t.shape
            bits = got.view(idt).cpu().numpy().view(BITS_DT[code])
            assert_same(bits, ref_from_fixed(code, v), "read_float(device=True) %s" % NAME[code])
        for b in bufs:
            b.free()
    finally:
        ctx.close()
