"""Value and shape edges of the level-2 field ops (`lmn_op_*` / `lmn_col_*`): circle FFT (interpolate, evaluate,
extend, evaluate_block), eval_at_point, FRI quotients, the two folds, decompose, accumulate, bit_reverse, logup and
composition.  Run against the emulation build on CPU (tests/test_numeric_edges_emu.py) and the HIP library on GPU
(tests/test_gpu_numeric_edges.py).

Reference.  Up to 2^8 points every op is restated here with plain Python integers mod P (QM31 = CM31[u] / (u^2 - 2 - i),
CM31 = M31[i] / (i^2 + 1)): evaluation by the basis definition (coefficient j multiplies y^j0 * x^j1 * pi(x)^j2 ...,
pi(x) = 2x^2 - 1, on the bit-reversed canonic domain), folds, quotients, decompose and eval_at_point by their stwo
definitions, logup from the `Rel` entries of `oracle.air.COMPONENTS` read as data (fractions, running sums, the
coset-order scan), and of composition everything but the local constraints (the logup constraints, Z, the previous-row
lookup, the claimed shift, the accumulate step; the local constraint sets are stated once, in the oracle, and are tied to
the kernel by the low-degree identity on valid witnesses).  Only the domain points come from `oracle.circle` (pinned by
the KAT).  These restatements also pin the
numpy oracle at those sizes.  Above 2^8 the reference is `oracle.fft` / `oracle.prover` (uint64 arithmetic, exact
because every product is < 2^62), and from 2^21 points the C oracle (`oracle.cbackend`, tied to numpy by
test_oracle_c.py).  Algebraic identities are checked as well: interpolate(evaluate(c)) == c, a constant column
interpolates to [k, 0, ...], a constant polynomial evaluates to its constant anywhere.

Value classes (data, alpha, point coordinates, sample values): all 0, all P-1, alternating 0 / P-1, words drawn from
EDGE_WORDS, uniform random, and inputs built so that outputs land on 0.  Every output word must be canonical (< P)."""
import numpy as np

P = (1 << 31) - 1
U64 = np.uint64
EDGE_WORDS = [0, 1, 2, 1 << 16, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, P - 2, P - 1]
CLASSES = ("zero", "pm1", "alt", "edge", "random", "zero_out")


class LimitError(AssertionError):
    pass


# ----------------------------------------------------------------------------- plain-integer field arithmetic
def c_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def c_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def c_inv(a):
    n = (a[0] * a[0] + a[1] * a[1]) % P
    assert n, "CM31 zero has no inverse"
    ni = pow(n, P - 2, P)
    return (a[0] * ni % P, -a[1] * ni % P)


def q(*w):
    return tuple(int(v) % P for v in w)


Q0, Q1 = (0, 0, 0, 0), (1, 0, 0, 0)


def q_add(a, b):
    return tuple((x + y) % P for x, y in zip(a, b))


def q_sub(a, b):
    return tuple((x - y) % P for x, y in zip(a, b))


def q_mul(a, b):
    A, B, C, D = a[:2], a[2:], b[:2], b[2:]
    bd = c_mul(B, D)
    rbd = ((2 * bd[0] - bd[1]) % P, (bd[0] + 2 * bd[1]) % P)        # (2 + i) * B * D
    lo = ((c_mul(A, C)[0] + rbd[0]) % P, (c_mul(A, C)[1] + rbd[1]) % P)
    hi = ((c_mul(A, D)[0] + c_mul(B, C)[0]) % P, (c_mul(A, D)[1] + c_mul(B, C)[1]) % P)
    return lo + hi


def q_mul_m(a, m):
    return tuple(x * m % P for x in a)


def q_conj(a):
    return (a[0], a[1], -a[2] % P, -a[3] % P)


def q_pow(a, e):
    r = Q1
    for _ in range(e):
        r = q_mul(r, a)
    return r


def m_inv(a):
    assert a % P, "M31 zero has no inverse"
    return pow(a, P - 2, P)


# ----------------------------------------------------------------------------- value classes
def words(cls, shape, rng):
    """uint64 array of `shape` in value class `cls` ("zero_out" has no generic form: callers build it; here it is
    the edge words with half of them zeroed)."""
    n = int(np.prod(shape))
    if cls == "zero":
        w = np.zeros(n, dtype=U64)
    elif cls == "pm1":
        w = np.full(n, P - 1, dtype=U64)
    elif cls == "alt":
        w = (np.arange(n, dtype=U64) % U64(2)) * U64(P - 1)
    elif cls == "edge":
        w = np.array(EDGE_WORDS, dtype=U64)[rng.integers(0, len(EDGE_WORDS), size=n)]
    elif cls == "random":
        w = rng.integers(0, P, size=n, dtype=U64)
    elif cls == "zero_out":
        w = np.array(EDGE_WORDS, dtype=U64)[rng.integers(0, len(EDGE_WORDS), size=n)]
        w[rng.random(n) < 0.5] = 0
    else:
        raise ValueError(cls)
    return w.reshape(shape)


def qword(cls, rng):
    return q(*[int(v) for v in words("random" if cls == "zero_out" else cls, (4,), rng)])


def canonical(a, what):
    a = np.asarray(a)
    assert a.size == 0 or int(a.max()) < P, "%s: a non-canonical word (%d) in the output" % (what, int(a.max()))


def canonical_q(t, what):
    assert all(0 <= int(v) < P for v in t), "%s: non-canonical %r" % (what, t)


def same(got, want, what):
    got, want = np.asarray(got).astype(U64), np.asarray(want).astype(U64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError("%s: %d words differ, first at %s: got %d want %d" % (what, len(bad), i, got[i], want[i]))


# ----------------------------------------------------------------------------- domain points
_PTS = {}


def domain_points(log):
    """bit-reversed canonic domain of 2^log points as Python-int lists (x, y)"""
    if log not in _PTS:
        from oracle.circle import CanonicCoset
        xs, ys = CanonicCoset(log).circle_domain().points_bitrev()
        _PTS[log] = ([int(v) for v in xs], [int(v) for v in ys])
    return _PTS[log]


def basis_values(x, y, n, mul, one):
    """[prod_k maps[k]^(bit k of j) for j < 2^n], maps = [y, x, pi(x), pi^2(x), ...]"""
    maps = [y, x]
    cur = x
    while len(maps) < n:
        cur = mul(cur, cur)
        cur = tuple((2 * v) % P for v in cur) if isinstance(cur, tuple) else 2 * cur % P
        cur = q_sub(cur, Q1) if isinstance(cur, tuple) else (cur - 1) % P
        maps.append(cur)
    b = [one]
    for k in range(n):
        b = b + [mul(v, maps[k]) for v in b]
    return b


_BASIS = {}


def basis_matrix(log_coeffs, log_domain):
    key = (log_coeffs, log_domain)
    if key not in _BASIS:
        xs, ys = domain_points(log_domain)
        m = [basis_values(x, y, log_coeffs, lambda a, b: a * b % P, 1) for x, y in zip(xs, ys)]
        _BASIS[key] = np.array(m, dtype=object)
    return _BASIS[key]


PY_MAX_LOG = 8        # plain-integer reference up to 2^8 points
C_MIN_LOG = 21        # the C oracle from 2^21 points


def _c_oracle():
    from oracle.cbackend import CKernels
    global _CK
    try:
        return _CK
    except NameError:
        _CK = CKernels()
        return _CK


def ref_evaluate(co, log_domain):
    """(ncols, 2^k) coefficients -> (ncols, 2^log_domain) evaluations"""
    co = np.asarray(co, dtype=U64)
    k = co.shape[1].bit_length() - 1
    if log_domain <= PY_MAX_LOG:
        B = basis_matrix(k, log_domain)
        return (B.dot(co.astype(object).T) % P).T.astype(U64)
    if log_domain >= C_MIN_LOG:
        return _c_oracle()._evaluate(co.astype(np.uint32), log_domain).astype(U64)
    from oracle import fft
    return fft.evaluate(co, log_domain)


def ref_interpolate(ev):
    ev = np.asarray(ev, dtype=U64)
    log = ev.shape[1].bit_length() - 1
    if log >= C_MIN_LOG:
        return np.stack(_c_oracle().interpolate_cols(list(ev.astype(np.uint32)))).astype(U64)
    from oracle import fft
    co = fft.interpolate(ev)
    if log <= PY_MAX_LOG:     # the basis is a bijection: these coefficients are the only ones that evaluate to ev
        same(ref_evaluate(co, log), ev, "numpy oracle interpolate, log %d" % log)
    return co


def ref_eval_at_point(co, pt):
    """one coefficient vector at a QM31 point pt = (x, y) (tuples of 4 words)"""
    co = [int(v) for v in co]
    n = len(co).bit_length() - 1
    if n <= PY_MAX_LOG:
        if n == 0:
            return q(co[0], 0, 0, 0)
        b = basis_values(pt[0], pt[1], n, q_mul, Q1)
        acc = Q0
        for c, v in zip(co, b):
            acc = q_add(acc, q_mul_m(v, c))
        return acc
    from oracle import fft
    from oracle.field import QM31
    return tuple(fft.eval_at_point(np.array(co, dtype=U64), (QM31(*pt[0]), QM31(*pt[1]))).v)


# ----------------------------------------------------------------------------- 1. the small-domain evaluate regression
SMALL_DOMAIN_CASES = ((1, 2), (2, 3), (3, 4), (1, 4), (2, 4))


def dirty_context(ctx, rng):
    """run other ops first, so that the arena and the allocator hold stale non-zero words"""
    junk = rng.integers(1, P, size=(5, 1 << 10), dtype=U64).astype(np.uint32)
    ctx.evaluate(junk, 12)
    ctx.interpolate(junk)
    h = ctx.col_from_cpu(junk)
    for lg in (4, 5, 8):
        ctx.col_from_cpu(rng.integers(1, P, size=(3, 1 << lg), dtype=U64)).free()
    h.free()


def check_small_domain_evaluate(ctx, lc, ld):
    """evaluate onto 2^4 points or fewer from a smaller polynomial: the words past the coefficients are zero, not
    whatever follows them in memory (the next column, stale arena words)"""
    rng = np.random.default_rng(100 * lc + ld)
    dirty_context(ctx, rng)
    for cls in ("random", "zero", "pm1"):
        co = words(cls, (3, 1 << lc), rng)
        want = ref_evaluate(co, ld)
        got = ctx.evaluate(co.astype(np.uint32), ld)
        canonical(got, "op_evaluate")
        same(got, want, "op_evaluate %d -> %d, 3 columns, %s" % (lc, ld, cls))
        h = ctx.col_from_cpu(co)
        e = h.evaluate(ld)
        same(e.to_cpu(), want, "col_evaluate %d -> %d, 3 columns, %s" % (lc, ld, cls))
        e.free()
        for c in range(3):                       # one-column handles: the read must not leave the allocation
            h1 = ctx.col_from_cpu(co[c:c + 1])
            e1 = h1.evaluate(ld)
            same(e1.to_cpu(), want[c:c + 1], "col_evaluate %d -> %d, column %d alone, %s" % (lc, ld, c, cls))
            e1.free()
            h1.free()
            same(ctx.evaluate(co[c:c + 1].astype(np.uint32), ld), want[c:c + 1], "op_evaluate one column")
        h.free()


# ----------------------------------------------------------------------------- 2. FFT: interpolate / evaluate / extend
def fft_coeffs(cls, ncols, log, rng):
    """coefficients in value class cls; "zero_out": the interpolant of edge words half of which are 0, so that the
    evaluation on the same-size domain lands on 0 (and on P - 1, 1, 2^30 ...) exactly"""
    if cls != "zero_out":
        return words(cls, (ncols, 1 << log), rng)
    return ref_interpolate(words("zero_out", (ncols, 1 << log), rng))


def check_fft_case(ctx, log, blowup, ncols, cls, col_form=True, seed=0):
    rng = np.random.default_rng(seed * 7919 + log * 131 + blowup * 17 + ncols)
    ld = log + blowup
    tag = "log %d blowup %d ncols %d %s" % (log, blowup, ncols, cls)
    co = fft_coeffs(cls, ncols, log, rng)
    want = ref_evaluate(co, ld)
    got = ctx.evaluate(co.astype(np.uint32), ld)
    canonical(got, "op_evaluate " + tag)
    same(got, want, "op_evaluate " + tag)
    # interpolate: values in the class (zero_out: evaluations of a sparse polynomial, so most coefficients are 0)
    if cls == "zero_out":
        sparse = words("edge", (ncols, 1 << log), rng)
        sparse[:, 1::2] = 0
        sparse[:, (1 << log) // 2:] = 0
        ev = ref_evaluate(sparse, log)
    else:
        ev = words(cls, (ncols, 1 << log), rng)
    gi = ctx.interpolate(ev.astype(np.uint32))
    canonical(gi, "op_interpolate " + tag)
    same(gi, sparse if cls == "zero_out" else ref_interpolate(ev), "op_interpolate " + tag)
    if not col_form:
        return
    h = ctx.col_from_cpu(co)
    e = h.evaluate(ld)
    ge = e.to_cpu()
    canonical(ge, "col_evaluate " + tag)
    same(ge, want, "col_evaluate " + tag)
    ext = h.extend(ld)
    zext = np.concatenate([co, np.zeros((ncols, (1 << ld) - (1 << log)), dtype=U64)], axis=1)
    same(ext.to_cpu(), zext, "col_extend " + tag)
    e2 = ext.evaluate(ld)
    same(e2.to_cpu(), want, "evaluate(extend(c)) " + tag)
    e.interpolate()                                             # interpolate(evaluate(c)) == c, zero-extended
    gb = e.to_cpu()
    canonical(gb, "col_interpolate " + tag)
    same(gb, zext, "interpolate(evaluate(c)) " + tag)
    for x in (h, e, ext, e2):
        x.free()


def check_constant_columns(ctx, log):
    """a constant column interpolates to [k, 0, ...]; the constant polynomial evaluates to k on any domain and at any
    point"""
    rng = np.random.default_rng(log)
    ks = np.array([0, 1, P - 1, 1 << 30, int(rng.integers(0, P))], dtype=U64)
    ev = np.repeat(ks[:, None], 1 << log, axis=1)
    co = ctx.interpolate(ev.astype(np.uint32))
    canonical(co, "interpolate constant")
    want = np.zeros_like(ev)
    want[:, 0] = ks
    same(co, want, "constant columns interpolate, log %d" % log)
    same(ctx.evaluate(co, log + 1), np.repeat(ks[:, None], 2 << log, axis=1), "constant polynomial evaluates")
    pt = (qword("random", rng), qword("random", rng))
    for c in range(len(ks)):
        assert ctx.eval_at_point(co[c], list(pt[0]) + list(pt[1])) == (int(ks[c]), 0, 0, 0)


# ----------------------------------------------------------------------------- evaluate_block
def check_evaluate_block_case(ctx, log_coeffs, log_domain, g, cls, ncols=3, col_form=False):
    rng = np.random.default_rng(log_domain * 10 + g)
    co = fft_coeffs(cls, ncols, log_coeffs, rng)
    full = ref_evaluate(co, log_domain)
    S = 1 << (log_domain - g)
    h = ctx.col_from_cpu(co) if col_form else None
    for b in range(1 << g):
        got = ctx.evaluate_block(co.astype(np.uint32), log_domain, g, b)
        canonical(got, "evaluate_block")
        same(got, full[:, b * S:(b + 1) * S], "evaluate_block %d -> %d, g %d, block %d, %s" % (log_coeffs, log_domain, g, b, cls))
        if h is not None:
            blk = h.evaluate_block(log_domain, g, b)
            same(blk.to_cpu(), full[:, b * S:(b + 1) * S], "col_evaluate_block %d -> %d g %d b %d" % (log_coeffs, log_domain, g, b))
            blk.free()
    if h is not None:
        h.free()


# ----------------------------------------------------------------------------- eval_at_point
def point_in_class(cls, rng):
    if cls == "zero_out":
        return (q(int(rng.integers(0, P)), 0, 0, 0), q(int(rng.integers(0, P)), 0, 0, 0))
    return (qword(cls, rng), qword(cls, rng))


def check_eval_at_point_case(ctx, log, cls):
    rng = np.random.default_rng(log * 3 + CLASSES.index(cls))
    co = words("random" if cls == "zero_out" else cls, (2, 1 << log), rng)
    pt = point_in_class(cls, rng)
    if cls == "zero_out":          # base-field point: the value is an M31 word, and c0 is chosen to cancel it
        for c in range(2):
            v = ref_eval_at_point(co[c], pt)
            co[c, 0] = (int(co[c, 0]) - v[0]) % P
    words_pt = list(pt[0]) + list(pt[1])
    h = ctx.col_from_cpu(co)
    for c in range(2):
        want = ref_eval_at_point(co[c], pt)
        if cls == "zero_out":
            assert want == Q0
        if log <= PY_MAX_LOG and log >= 1:        # pins the numpy oracle at this size
            from oracle import fft
            from oracle.field import QM31
            assert tuple(fft.eval_at_point(co[c], (QM31(*pt[0]), QM31(*pt[1]))).v) == want
        got = ctx.eval_at_point(co[c].astype(np.uint32), words_pt)
        canonical_q(got, "op_eval_at_point")
        assert got == want, ("op_eval_at_point log %d %s column %d" % (log, cls, c), got, want)
        got = h.eval_at_point(c, words_pt)
        canonical_q(got, "col_eval_at_point")
        assert got == want, ("col_eval_at_point log %d %s column %d" % (log, cls, c), got, want)
    h.free()


# ----------------------------------------------------------------------------- quotients
def ref_quotients(log, cols, samples, points, alpha):
    """stwo accumulate_quotients: samples [(col, point index, value)] in (column, mask) order; batches by point index in
    first-appearance order.  -> (4, 2^log)"""
    order, by_pt = [], {}
    for c, p, v in samples:
        if p not in by_pt:
            by_pt[p] = []
            order.append(p)
        by_pt[p].append((c, v))
    xs, ys = domain_points(log)
    L = 1 << log
    out = np.zeros((4, L), dtype=U64)
    coeffs = []
    for p in order:
        px, py = points[p]
        al, lines = Q1, []
        for c, v in by_pt[p]:
            al = q_mul(al, alpha)
            a = q_sub(q_conj(v), v)
            cc = q_sub(q_conj(py), py)
            b = q_sub(q_mul(v, cc), q_mul(a, py))
            lines.append((c, q_mul(al, a), q_mul(al, b), q_mul(al, cc)))
        coeffs.append((px, py, lines, q_pow(alpha, len(lines))))
    colv = [[int(v) for v in col] for col in cols]
    for r in range(L):
        x, y = xs[r], ys[r]
        acc = Q0
        for px, py, lines, bc in coeffs:
            num = Q0
            for c, a, b, cc in lines:
                num = q_add(num, q_sub(q_mul_m(cc, colv[c][r]), q_add(q_mul_m(a, y), b)))
            den = c_sub(c_mul(c_sub(px[:2], (x, 0)), py[2:]), c_mul(c_sub(py[:2], (y, 0)), px[2:]))
            di = c_inv(den)
            acc = q_add(q_mul(acc, bc), q_mul(num, di + (0, 0)))
        out[:, r] = acc
    return out


def quotient_case(cls, log, npts, per_batch, rng, extra_cols=0):
    """(cols, samples, points, alpha) with npts distinct points, per_batch[b] samples at point b"""
    ncols = max(per_batch) + extra_cols
    L = 1 << log
    if cls == "zero_out":           # constant columns sampled at their own value: every numerator is exactly 0
        ks = words("edge", (ncols,), rng)
        cols = np.repeat(ks[:, None], L, axis=1)
    else:
        cols = words(cls, (ncols, L), rng)
    points = []
    for _ in range(npts):           # the class sets the real parts; the u-parts stay random so no denominator is 0
        re = words("random" if cls == "zero_out" else cls, (4,), rng)
        im = rng.integers(1, P, size=4)
        points.append((q(re[0], re[1], im[0], im[1]), q(re[2], re[3], im[2], im[3])))
    samples = []
    for c in range(ncols):
        for b in range(npts):
            if c < per_batch[b]:
                v = q(int(ks[c]), 0, 0, 0) if cls == "zero_out" else qword(cls, rng)
                samples.append((c, b, v))
    alpha = qword(cls, rng)
    return list(cols), samples, points, alpha


def check_quotients_case(ctx, cls, log, npts, per_batch, col_form=True, seed=0):
    rng = np.random.default_rng(seed + 1000 * log + 100 * npts + sum(per_batch))
    cols, samples, points, alpha = quotient_case(cls, log, npts, per_batch, rng)
    tag = "quotients log %d, %d points, %s per batch, %s" % (log, npts, per_batch, cls)
    pts_w = [list(px) + list(py) for px, py in points]
    if log <= PY_MAX_LOG:
        want = ref_quotients(log, cols, samples, points, alpha)
        if len(samples) <= 64:                # pins the numpy oracle (it batches by point value: the points differ)
            from oracle.field import QM31
            from oracle.prover import accumulate_quotients
            per_col = [[] for _ in cols]
            for c, p, v in samples:
                per_col[c].append(((QM31(*points[p][0]), QM31(*points[p][1])), QM31(*v)))
            same(accumulate_quotients(log, [np.asarray(c, dtype=U64) for c in cols], per_col, QM31(*alpha)).T, want,
                 "numpy oracle " + tag)
    else:
        from oracle.field import QM31
        from oracle.prover import accumulate_quotients
        per_col = [[] for _ in cols]
        for c, p, v in samples:
            per_col[c].append(((QM31(*points[p][0]), QM31(*points[p][1])), QM31(*v)))
        want = accumulate_quotients(log, [np.asarray(c, dtype=U64) for c in cols], per_col, QM31(*alpha)).T
    if cls == "zero_out":
        assert not want.any()
    got = ctx.accumulate_quotients([np.asarray(c, dtype=np.uint32) for c in cols], samples, pts_w, alpha)
    canonical(got, "op_accumulate_quotients " + tag)
    same(got, want, "op_accumulate_quotients " + tag)
    if col_form:
        h = ctx.col_from_cpu(np.stack(cols))
        out = ctx.col_accumulate_quotients([h], samples, pts_w, alpha)
        g = out.to_cpu()
        canonical(g, "col_accumulate_quotients " + tag)
        same(g, want, "col_accumulate_quotients " + tag)
        out.free()
        h.free()


def check_quotient_limits(ctx):
    """more than 4 distinct sample points or more than 512 samples is a caller error (LMN_ERR_INVALID_ARGUMENT = -6),
    in both forms; exactly 4 points and 512 samples are computed"""
    from luminair_amd.backend import LuminairBackendError
    rng = np.random.default_rng(77)
    log = 3
    cols, samples, points, alpha = quotient_case("random", log, 5, [1, 1, 1, 1, 1], rng)
    pts_w = [list(px) + list(py) for px, py in points]
    h = ctx.col_from_cpu(np.stack(cols))
    too_many = [
        (samples, pts_w),                                                       # 5 distinct points
        ([(k % len(cols), 0, s[2]) for k, s in enumerate(samples * 103)][:513], pts_w[:1]),   # 513 samples
    ]
    for smp, pts in too_many:
        for call in (lambda: ctx.accumulate_quotients([np.asarray(c, dtype=np.uint32) for c in cols], smp, pts, alpha),
                     lambda: ctx.col_accumulate_quotients([h], smp, pts, alpha)):
            try:
                call()
            except LuminairBackendError as e:
                assert e.code == -6, (e.code, str(e))
            else:
                raise LimitError("accumulate_quotients accepted %d samples at %d points" % (len(smp), len({s[1] for s in smp})))
    # the context stays usable, and the largest accepted call is right: 4 points, 512 samples (128 per point)
    many = [(k % len(cols), k % 4, qword("random", rng)) for k in range(512)]
    many.sort(key=lambda s: s[0])              # (column, mask position) order
    want = ref_quotients(log, cols, many, points, alpha)
    same(ctx.accumulate_quotients([np.asarray(c, dtype=np.uint32) for c in cols], many, pts_w[:4], alpha), want,
         "op_accumulate_quotients, 4 points x 128 samples")
    out = ctx.col_accumulate_quotients([h], many, pts_w[:4], alpha)
    same(out.to_cpu(), want, "col_accumulate_quotients, 4 points x 128 samples")
    out.free()
    h.free()


# ----------------------------------------------------------------------------- folds
def ref_fold_line(src, alpha):
    """src (4, 2^k) on LineDomain(half_odds(k)) bit-reversed -> (4, 2^(k-1))"""
    from oracle.circle import Coset, LineDomain
    k = src.shape[1].bit_length() - 1
    n = src.shape[1] // 2
    if k > PY_MAX_LOG:
        from oracle.field import QM31
        from oracle.prover import fold_line
        return fold_line(src.T.astype(U64), QM31(*alpha), LineDomain(Coset.half_odds(k))).T
    xs = [int(v) for v in LineDomain(Coset.half_odds(k)).xs_bitrev()]
    out = np.zeros((4, n), dtype=U64)
    for i in range(n):
        a, b = q(*src[:, 2 * i]), q(*src[:, 2 * i + 1])
        f0, f1 = q_add(a, b), q_mul_m(q_sub(a, b), m_inv(xs[2 * i]))
        out[:, i] = q_add(f0, q_mul(alpha, f1))
    return out


def ref_fold_circle(dst, src, alpha):
    k = src.shape[1].bit_length() - 1
    n = src.shape[1] // 2
    if k > PY_MAX_LOG:
        from oracle.field import QM31
        from oracle.prover import fold_circle_into_line
        return fold_circle_into_line(dst.T.astype(U64), src.T.astype(U64), QM31(*alpha), k).T
    _, ys = domain_points(k)
    a2 = q_mul(alpha, alpha)
    out = np.zeros((4, n), dtype=U64)
    for i in range(n):
        a, b = q(*src[:, 2 * i]), q(*src[:, 2 * i + 1])
        f0, f1 = q_add(a, b), q_mul_m(q_sub(a, b), m_inv(ys[2 * i]))
        out[:, i] = q_add(q_mul(q(*dst[:, i]), a2), q_add(f0, q_mul(alpha, f1)))
    return out


def check_folds_case(ctx, log_src, cls, col_form=True):
    rng = np.random.default_rng(log_src * 11 + CLASSES.index(cls))
    n = 1 << log_src
    if cls == "zero_out":          # pairs (a, P - a) and alpha = 0: f0 = a + (P - a) must be written as 0
        a = words("edge", (4, n // 2), rng)
        src = np.empty((4, n), dtype=U64)
        src[:, 0::2] = a
        src[:, 1::2] = (U64(P) - a) % U64(P)
        alpha = Q0
        dst = np.zeros((4, n // 2), dtype=U64)
    else:
        src = words(cls, (4, n), rng)
        alpha = qword(cls, rng)
        dst = np.full((4, n // 2), P - 1, dtype=U64)
    tag = "log_src %d %s" % (log_src, cls)
    want = ref_fold_line(src, alpha)
    if cls == "zero_out":
        assert not want.any()
    if log_src <= PY_MAX_LOG:
        from oracle.circle import Coset, LineDomain
        from oracle.field import QM31
        from oracle.prover import fold_line, fold_circle_into_line
        same(fold_line(src.T, QM31(*alpha), LineDomain(Coset.half_odds(log_src))).T, want, "numpy fold_line " + tag)
    got = ctx.fold_line(src.astype(np.uint32), alpha)
    canonical(got, "op_fold_line " + tag)
    same(got, want, "op_fold_line " + tag)
    want_c = ref_fold_circle(dst, src, alpha)
    if log_src <= PY_MAX_LOG:
        same(fold_circle_into_line(dst.T, src.T, QM31(*alpha), log_src).T, want_c, "numpy fold_circle_into_line " + tag)
    got = ctx.fold_circle_into_line(dst.astype(np.uint32), src.astype(np.uint32), alpha)
    canonical(got, "op_fold_circle_into_line " + tag)
    same(got, want_c, "op_fold_circle_into_line " + tag)
    if col_form:
        hs = ctx.col_from_cpu(src)
        fl = hs.fold_line(alpha)
        same(fl.to_cpu(), want, "col_fold_line " + tag)
        hd = ctx.col_from_cpu(dst)
        hd.fold_circle_into_line(hs, alpha)
        g = hd.to_cpu()
        canonical(g, "col_fold_circle_into_line " + tag)
        same(g, want_c, "col_fold_circle_into_line " + tag)
        for x in (hs, fl, hd):
            x.free()


# ----------------------------------------------------------------------------- decompose / accumulate / bit_reverse
def check_decompose_accumulate_bitrev_case(ctx, log, cls):
    rng = np.random.default_rng(log * 13 + CLASSES.index(cls))
    n = 1 << log
    tag = "log %d %s" % (log, cls)
    if cls == "zero_out":          # f = lambda on the first half, -lambda on the second: g == 0
        lam = words("edge", (4,), rng)
        f = np.empty((4, n), dtype=U64)
        f[:, :n // 2] = lam[:, None]
        f[:, n // 2:] = ((U64(P) - lam) % U64(P))[:, None]
    else:
        f = words(cls, (4, n), rng)
    inv_n = m_inv(n % P)
    want_lam = tuple((int(f[k, :n // 2].sum()) - int(f[k, n // 2:].sum())) * inv_n % P for k in range(4))   # < 2^50
    want_g = f.copy()
    for k in range(4):
        want_g[k, :n // 2] = (f[k, :n // 2] + U64(P) - U64(want_lam[k])) % U64(P)
        want_g[k, n // 2:] = (f[k, n // 2:] + U64(want_lam[k])) % U64(P)
    if cls == "zero_out":
        assert want_lam == tuple(int(v) for v in lam) and not want_g.any()
    hf = ctx.col_from_cpu(f)
    g, lam_got = hf.decompose()
    canonical_q(lam_got, "decompose lambda " + tag)
    assert lam_got == want_lam, ("decompose lambda " + tag, lam_got, want_lam)
    gg = g.to_cpu()
    canonical(gg, "decompose g " + tag)
    same(gg, want_g, "decompose g " + tag)
    g.free()
    # accumulate: x + (P - x) for zero_out, else the class plus uniform words
    other = (U64(P) - f) % U64(P) if cls == "zero_out" else words("random" if cls == "zero" else cls, (4, n), rng)
    ho = ctx.col_from_cpu(other)
    hf.accumulate(ho)
    acc = hf.to_cpu()
    canonical(acc, "accumulate " + tag)
    same(acc, (f + other) % U64(P), "accumulate " + tag)
    # bit_reverse: a permutation and an involution
    idx = np.zeros(n, dtype=np.int64)
    for b in range(log):
        idx |= ((np.arange(n) >> b) & 1) << (log - 1 - b)
    ho.bit_reverse()
    same(ho.to_cpu(), other[:, idx], "bit_reverse " + tag)
    ho.bit_reverse()
    same(ho.to_cpu(), other, "bit_reverse twice " + tag)
    hf.free()
    ho.free()


# ----------------------------------------------------------------------------- logup / composition
def relation_elements(rng):
    """five (z, alpha) pairs drawn as the channel would: uniform QM31"""
    return [(qword("random", rng), qword("random", rng)) for _ in range(5)]


def _oracle_elems(elems):
    from oracle.field import QM31
    return [(QM31(*z), QM31(*a)) for z, a in elems]


def q_inv(a):
    """1 / (A + B u) = (A - B u) / (A^2 - (2 + i) B^2)"""
    A, B = a[:2], a[2:]
    b2 = c_mul(B, B)
    di = c_inv(c_sub(c_mul(A, A), ((2 * b2[0] - b2[1]) % P, (b2[0] + 2 * b2[1]) % P)))
    return c_mul(A, di) + c_mul(c_sub((0, 0), B), di)


def coset_order(log):
    """storage index of every coset position (the order in which the trace rows follow each other): position i is
    circle-domain index i / 2 for even i and n - (i + 1) / 2 for odd i, stored at that index bit-reversed"""
    n = 1 << log
    i = np.arange(n, dtype=np.int64)
    cd = np.where(i % 2 == 0, i // 2, n - (i + 1) // 2)
    s = np.zeros(n, dtype=np.int64)
    for b in range(log):
        s |= ((cd >> b) & 1) << (log - 1 - b)
    return s


def _int_cols(a):
    return [] if a is None else [[int(v) for v in col] for col in a]


def _rel_den_num(rel, main, pre, elems, r):
    """row r of one relation entry: (val + alpha * id - z, +-mult); main / pre are lists of Python-int columns"""
    src = pre if rel.pre else main
    z, alpha = elems[rel.elems]
    den = q(src[rel.val][r], 0, 0, 0)
    if rel.id is not None:
        den = q_add(den, q_mul_m(alpha, src[rel.id][r]))
    m = main[rel.mult][r]
    return q_sub(den, z), (-m % P if rel.neg else m)


def ref_logup(comp, main, pre, elems):
    """the interaction trace of a component in plain integers, from its `Rel` entries read as data: group j of row r is
    the sum of +-mult / (val + alpha * id - z) over relations 0..j; the last group is replaced by the running sum, along
    coset order, of itself minus claimed / n.  -> ((4 * relations, n) words, claimed sum)"""
    main, pre = _int_cols(main), _int_cols(pre)
    n = len(main[0])
    log = n.bit_length() - 1
    nr = len(comp.relations)
    out = np.zeros((4 * nr, n), dtype=U64)
    last = []
    for r in range(n):
        S = Q0
        for j, rel in enumerate(comp.relations):
            den, num = _rel_den_num(rel, main, pre, elems, r)
            S = q_add(S, q_mul_m(q_inv(den), num))
            out[4 * j:4 * j + 4, r] = S
        last.append(S)
    claimed = Q0
    for S in last:
        claimed = q_add(claimed, S)
    shift = q_mul_m(claimed, m_inv(n % P))
    run = Q0
    for s in coset_order(log):
        run = q_add(run, q_sub(last[s], shift))
        out[4 * nr - 4:, s] = run
    return out, claimed


def oracle_logup_last_group(comp, main, elems, pre, oracle_cols):
    """the numpy oracle's last group before the scan, (n, 4): the group before it, which `gen_interaction_trace` returns
    unscanned in `oracle_cols`, plus the last relation's fraction from the pieces `gen_interaction_trace` is made of"""
    from oracle import field as F
    from oracle.prover import combine, rel_operands
    nr = len(comp.relations)
    rel = comp.relations[-1]
    z, alpha = elems[rel.elems]
    val, idv, mult = rel_operands(rel, main, pre)
    frac = F.q_mul_m(F.q_inv(combine(z, alpha, val, idv)), mult)
    if nr == 1:
        return frac
    return F.q_add(np.ascontiguousarray(oracle_cols[4 * nr - 8:4 * nr - 4].T), frac)


def check_logup_scan(got, claimed, last_group, what):
    """The scan on its own, from the op's output: along coset order the first differences of the scanned column, plus
    shift = claimed / n, are the last group's per-row sums; they must be the oracle's unscanned fractions, the column
    must end on 0, and every prefix must be a numpy cumsum of those fractions minus their shift (words < 2^31 over at most
    2^21 rows stay below 2^52: uint64 is exact).  The message says which part is wrong: a wrong fraction changes the
    claimed sum, and so does a wrong block total (the op adds the claimed sum up from them); a scan that is wrong after
    its totals leaves the sum alone."""
    n = got.shape[1]
    log = n.bit_length() - 1
    assert log <= 21
    order = coset_order(log)
    t = got[-4:].astype(U64).T[order]                                     # (n, 4) in coset order
    shift = np.array(q_mul_m(claimed, m_inv(n % P)), dtype=U64)
    before = np.concatenate([np.zeros((1, 4), dtype=U64), t[:-1]])
    s_last = (t + U64(P) - before + shift) % U64(P)
    want_last = np.asarray(last_group, dtype=U64)[order]
    want_claimed = tuple(int(v) for v in want_last.sum(axis=0) % U64(P))
    want_shift = np.array(q_mul_m(want_claimed, m_inv(n % P)), dtype=U64)
    pref = np.cumsum((want_last + U64(P) - want_shift) % U64(P), axis=0) % U64(P)
    said = []
    bad = np.argwhere(s_last != want_last)
    if len(bad):
        i, k = (int(v) for v in bad[0])
        said.append("the last group recovered from the first differences differs from the oracle's fractions in %d words, "
                    "first at coset position %d (storage index %d) coordinate %d: got %d want %d"
                    % (len(bad), i, order[i], k, s_last[i, k], want_last[i, k]))
    if t[-1].any():
        said.append("the scanned column ends on %r, not 0" % (tuple(int(v) for v in t[-1]),))
    bad = np.argwhere(t != pref)
    if len(bad):
        i, k = (int(v) for v in bad[0])
        said.append("%d prefix words differ from the cumsum, first at coset position %d (storage index %d) coordinate %d: "
                    "got %d want %d" % (len(bad), i, order[i], k, t[i, k], pref[i, k]))
    if tuple(claimed) != want_claimed:
        said.append("claimed sum %r, the oracle's fractions add up to %r" % (tuple(claimed), want_claimed))
        verdict = "the claimed sum is wrong: the last relation's FRACTIONS, or the block totals of the scan that the sum is made of"
    else:
        verdict = "the claimed sum is right, so the fractions add up: the SCAN is wrong"
    if said:
        raise AssertionError("%s: %s: %s" % (what, verdict, "; ".join(said)))


def check_logup_kind(ctx, kind, log, cls="random"):
    """lmn_col_logup on full-range main columns.  Up to 2^8 rows the reference is `ref_logup` (plain integers), which the
    numpy oracle (`oracle.prover.gen_interaction_trace`) must equal too; above, the oracle is the reference and
    `check_logup_scan` checks the scan on its own.

    Not tested: a zero denominator, z = val + alpha * id in some row.  Only caller-chosen relation elements reach it (a
    proof draws z at random); the oracle returns a value there, the kernel's one batched inverse per row makes every
    fraction of that row 0."""
    from oracle import air
    from oracle.prover import gen_interaction_trace
    comp = air.COMPONENTS[kind]
    rng = np.random.default_rng(kind * 100 + log)
    n = 1 << log
    tag = "logup kind %d log %d %s" % (kind, log, cls)
    main = words(cls, (comp.n_cols, n), rng)
    pre = words("random", (len(comp.pre_cols), n), rng) if comp.pre_cols else None
    elems = relation_elements(rng)
    pre_l = list(pre) if pre is not None else ()
    want_cols, want_claimed = gen_interaction_trace(comp, main, _oracle_elems(elems), pre_l)
    want, want_claimed = np.stack(want_cols), tuple(int(v) for v in want_claimed.v)
    if log <= PY_MAX_LOG:                        # pins the numpy oracle at this size
        oracle, oracle_claimed = want, want_claimed
        want, want_claimed = ref_logup(comp, main, pre, elems)
        same(oracle, want, "numpy oracle " + tag)
        assert oracle_claimed == want_claimed, ("numpy oracle claimed sum " + tag, oracle_claimed, want_claimed)
    hm = ctx.col_from_cpu(main)
    hp = ctx.col_from_cpu(pre) if pre is not None else None
    inter, claimed = ctx.col_logup(kind, hm, hp, {i: e for i, e in enumerate(elems)})
    got = inter.to_cpu()
    for x in (hm, hp, inter):
        if x is not None:
            x.free()
    canonical(got, tag)
    canonical_q(claimed, "claimed sum " + tag)
    if log > PY_MAX_LOG:
        same(got[:-4], want[:-4], tag + ": the groups before the last, which the fraction kernel writes and no scan touches")
        check_logup_scan(got, claimed, oracle_logup_last_group(comp, main, _oracle_elems(elems), pre_l, want), tag)
    same(got, want, tag)
    assert claimed == want_claimed, ("claimed sum " + tag, claimed, want_claimed)


def check_logup_refusals(ctx):
    """what lmn_col_logup must refuse with LMN_ERR_INVALID_ARGUMENT (-6): 2^3 and 2^27 rows (the 2^27 handles are two
    zeroed one-column allocations of 512 MiB, kind 14), a column count that is not the kind's, a lookup kind without its
    preprocessed columns or with them at another size, a relation element word that is not canonical.  After each
    refusal a correct 2^4 call on the same context succeeds."""
    from luminair_amd.backend import LuminairBackendError
    from oracle import air
    rng = np.random.default_rng(2727)
    good = {i: e for i, e in enumerate(relation_elements(rng))}

    def cols(kind, log, extra=0):
        return ctx.col_from_cpu(words("random", (air.COMPONENTS[kind].n_cols + extra, 1 << log), rng))

    def pre_of(kind, log):
        return ctx.col_from_cpu(words("random", (len(air.COMPONENTS[kind].pre_cols), 1 << log), rng))

    def bad_elems(set_index, alpha, word, value):
        e = {i: (list(z), list(a)) for i, (z, a) in good.items()}
        e[set_index][alpha][word] = value
        return e

    cases = [
        ("2^3 rows", 0, lambda: cols(0, 3), None, good),
        ("2^27 rows", 14, lambda: ctx.col_zeros(1, 27), lambda: ctx.col_zeros(1, 27), good),
        ("one column too many", 0, lambda: cols(0, 4, 1), None, good),
        ("one column too few", 13, lambda: cols(13, 4, -1), None, good),
        ("a lookup kind without its preprocessed columns", 4, lambda: cols(4, 4), None, good),
        ("preprocessed columns of another size", 4, lambda: cols(4, 5), lambda: pre_of(4, 4), good),
        ("z word = P", 0, lambda: cols(0, 4), None, bad_elems(0, 0, 0, P)),
        ("alpha word = 2^32 - 1", 13, lambda: cols(13, 4), None, bad_elems(1, 1, 3, 0xFFFFFFFF)),
    ]
    for what, kind, make_main, make_pre, elems in cases:
        hm = make_main()
        hp = make_pre() if make_pre else None
        try:
            inter, _ = ctx.col_logup(kind, hm, hp, elems)
        except LuminairBackendError as e:
            assert e.code == -6, (what, e.code, str(e))
        else:
            inter.free()
            raise LimitError("col_logup accepted " + what)
        finally:
            hm.free()
            if hp is not None:
                hp.free()
        check_logup_kind(ctx, kind, 4)


# ----------------------------------------------------------------------------- composition
def prev_row_index(k):
    """for every storage index s of the 2^(k+1)-point evaluation domain, the storage index of the point p_s moved back
    by one step of the 2^k-row trace subgroup: circle-group multiplication on the coordinates, then a lookup of the
    point.  The domain's half coset walks in steps of that subgroup's generator, and domain indices 0 and 1 are stored
    at 0 and 2^k, so the step is p[2^k] * conj(p[0])."""
    xs, ys = domain_points(k + 1)

    def mul(a, b):
        return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)
    step = mul((xs[1 << k], ys[1 << k]), (xs[0], -ys[0] % P))
    back = (step[0], -step[1] % P)
    where = {(x, y): s for s, (x, y) in enumerate(zip(xs, ys))}
    assert len(where) == len(xs)
    return [where[mul((x, y), back)] for x, y in zip(xs, ys)]


def ref_composition_relations(comp, k, main, inter, pre, elems, claimed, rel_coeffs, acc0):
    """acc0 + (sum over the relations of coeff_j * c_j) / Z on the 2^(k+1)-point domain in plain integers, the local
    constraints left out (their coefficients are 0 in the call this is compared with):
    c_j = (cur_j - cur_(j-1)) * den_j - (+-mult_j), and for the last relation
    c = (cur - cur_(j-1) - last[prev(s)] + claimed / 2^k) * den - (+-mult);  Z(s) = pi^(k-1)(x_s)"""
    main, inter, pre = _int_cols(main), _int_cols(inter), _int_cols(pre)
    E = 2 << k
    xs, _ = domain_points(k + 1)
    prev = prev_row_index(k)
    shift = q_mul_m(claimed, m_inv((1 << k) % P))
    nr = len(comp.relations)
    last = [q(*(inter[4 * (nr - 1) + t][s] for t in range(4))) for s in range(E)]
    out = np.zeros((4, E), dtype=U64)
    for s in range(E):
        z = xs[s]
        for _ in range(k - 1):
            z = (2 * z * z - 1) % P
        total, before = Q0, Q0
        for j, rel in enumerate(comp.relations):
            cur = q(*(inter[4 * j + t][s] for t in range(4)))
            den, num = _rel_den_num(rel, main, pre, elems, s)
            diff = q_sub(cur, before)
            if j == nr - 1:
                diff = q_add(q_sub(diff, last[prev[s]]), shift)
            total = q_add(total, q_mul(rel_coeffs[j], q_sub(q_mul(diff, den), q(num, 0, 0, 0))))
            before = cur
        out[:, s] = q_add(q(*acc0[:, s]), q_mul_m(total, m_inv(z)))
    return out


def _oracle_composition(comp, log, main, inter, pre, elems, claimed, coeffs):
    """(4, 2^(log+1)): sum_k c_k * coeff_k / Z by the numpy oracle"""
    from oracle.field import QM31
    from oracle.prover import ComponentInstance, eval_component_constraints_on_domain
    ci = ComponentInstance(comp, log, (0, comp.n_cols), (0, inter.shape[0]), QM31(*claimed))
    return eval_component_constraints_on_domain(ci, main, inter, _oracle_elems(elems), [QM31(*c) for c in coeffs], log + 1,
                                                list(pre) if pre is not None else ()).T


def _run_composition(ctx, kind, main, inter, pre, elems, claimed, coeffs, acc0):
    hm, hi = ctx.col_from_cpu(main), ctx.col_from_cpu(inter)
    hp = ctx.col_from_cpu(pre) if pre is not None else None
    acc = ctx.col_from_cpu(acc0)
    try:
        ctx.col_composition(kind, hm, hi, hp, {i: el for i, el in enumerate(elems)}, claimed, coeffs, acc)
        return acc.to_cpu()
    finally:
        for x in (hm, hi, hp, acc):
            if x is not None:
                x.free()


def check_composition_relations(ctx, kind, log, cls, coeff_cls):
    """lmn_col_composition with every local coefficient 0 and the relation coefficients in `coeff_cls`: what is left is
    the logup constraints, Z, the previous-row lookup, the claimed shift and the accumulate step, all of which
    `ref_composition_relations` restates.  The numpy oracle must equal it at the same inputs."""
    from oracle import air
    assert log + 1 <= PY_MAX_LOG
    comp = air.COMPONENTS[kind]
    rng = np.random.default_rng([kind, log, CLASSES.index(cls), CLASSES.index(coeff_cls)])
    E = 2 << log
    tag = "composition, relations only, kind %d log %d -> %d, columns %s, coefficients %s" % (kind, log, log + 1, cls, coeff_cls)
    main = words(cls, (comp.n_cols, E), rng)
    inter = words(cls, (4 * len(comp.relations), E), rng)
    pre = words("random", (len(comp.pre_cols), E), rng) if comp.pre_cols else None
    elems = relation_elements(rng)
    claimed = qword("random", rng)
    rel_coeffs = [qword(coeff_cls, rng) for _ in comp.relations]
    coeffs = [Q0] * comp.n_local + rel_coeffs
    acc0 = words("pm1", (4, E), rng)
    want = ref_composition_relations(comp, log, main, inter, pre, elems, claimed, rel_coeffs, acc0)
    oracle = (_oracle_composition(comp, log, main, inter, pre, elems, claimed, coeffs) + acc0) % U64(P)
    same(oracle, want, "numpy oracle " + tag)
    got = _run_composition(ctx, kind, main, inter, pre, elems, claimed, coeffs, acc0)
    canonical(got, tag)
    same(got, want, tag)


def check_composition_kind(ctx, kind, log, cls, coeff_cls, acc="class"):
    """lmn_col_composition (acc += sum_k c_k * coeff_k / Z) vs oracle.prover.eval_component_constraints_on_domain.
    acc: what the accumulator holds before the call - "class" (all P - 1 under random columns, random words otherwise),
    "zero", or "cancel" (P - the expected sum: every output word must then be exactly 0)"""
    from oracle import air
    comp = air.COMPONENTS[kind]
    rng = np.random.default_rng(kind * 1000 + log * 10 + CLASSES.index(cls))
    e = log + 1
    E = 1 << e
    main = words(cls, (comp.n_cols, E), rng)
    inter = words(cls, (4 * len(comp.relations), E), rng)
    pre = words("random", (len(comp.pre_cols), E), rng) if comp.pre_cols else None
    elems = relation_elements(rng)
    claimed = qword("random", rng)
    coeffs = [qword(coeff_cls, rng) for _ in range(comp.n_constraints)]
    acc0 = words("pm1" if cls == "random" else "random", (4, E), rng)
    want = _oracle_composition(comp, log, main, inter, pre, elems, claimed, coeffs)
    if acc == "zero":
        acc0 = np.zeros_like(acc0)
    elif acc == "cancel":
        acc0 = (U64(P) - want) % U64(P)
    else:
        assert acc == "class"
    want = (want + acc0) % U64(P)
    got = _run_composition(ctx, kind, main, inter, pre, elems, claimed, coeffs, acc0)
    tag = "composition kind %d log %d -> %d, columns %s, coefficients %s, accumulator %s" % (kind, log, e, cls, coeff_cls, acc)
    canonical(got, tag)
    if acc == "cancel":
        assert not want.any()
    same(got, want, tag)


COMPOSITION_COLUMN_CLASSES = ("zero", "pm1", "alt", "edge", "random")
COMPOSITION_COEFF_CLASSES = ("zero", "pm1", "edge", "random")
COMPOSITION_LARGE_KINDS = (0, 13, 4, 14)      # 3 and 7 node relations, a width-2 and a width-1 lookup


def composition_class_pairs(kind, log):
    """(column class, coefficient class) pairs of one kind at one size.  Up to 2^9 points: all twenty.  Above, where the
    oracle takes a tenth of a second and more per case: each column class once and each coefficient class at least once,
    the pairing rotated by the kind, so that over the 17 kinds every pair occurs; at 2^19 points (seconds per case) the
    kinds with many columns keep random / random and edge / edge."""
    cols, coeffs = COMPOSITION_COLUMN_CLASSES, COMPOSITION_COEFF_CLASSES
    if log <= 8:
        return [(c, k) for c in cols for k in coeffs]
    if log >= 18 and kind in (0, 13):
        return [("random", "random"), ("edge", "edge")]
    return [(c, coeffs[(i + kind) % len(coeffs)]) for i, c in enumerate(cols)]


# ----------------------------------------------------------------------------- the low-degree identity
def low_degree_tail(co, k):
    """the coefficients that vanish on a valid witness of 2^k rows: every index above 2^k.  The bound is the ORACLE's: its
    own composition, interpolated on 2^(k+1) points, shows for all 17 kinds at k = 4 and k = 6 zeros from index 2^k + 1 on
    and a non-zero coefficient AT index 2^k, not zeros from 2^k on.  (Degree-2 constraints over Z leave a circle polynomial
    of degree 2^(k-1); that space has 2^k + 1 dimensions, the last of them the basis function pi^(k-1)(x) of index 2^k.)"""
    co = np.asarray(co)
    assert co.shape[1] == 2 << k
    return co[:, (1 << k) + 1:]


def valid_witness(kind, k, rng):
    """(main columns (n_cols, 2^k), preprocessed columns or None) of a trace every constraint holds on: 2^k - 3 valid rows
    (tests/trace_doctor_checks.py builds them from luminair_amd.synthetic; a lookup component's row is a multiplicity),
    padded as the prover pads"""
    import trace_doctor_checks as tdc
    from oracle import air
    comp = air.COMPONENTS[kind]
    n = (1 << k) - 3
    rows = tdc._valid_rows(kind, n, rng) if comp.n_local else rng.integers(0, 5, size=(n, 1))
    main = air.pad_table(comp, rows)
    assert main.shape == (comp.n_cols, 1 << k)
    for c in comp.local([air.MV(col) for col in main]):
        assert not np.asarray(c.a).any(), "the witness of kind %d is not valid" % kind
    pre = words("random", (len(comp.pre_cols), 1 << k), rng) if comp.pre_cols else None
    return main, pre


def check_low_degree(ctx, kind, k):
    """On a valid witness the composition is a polynomial: logup on the main columns, every column extended to 2^(k+1)
    points, composition into a zero accumulator with random coefficients, and the accumulator interpolated has no
    coefficient of index > 2^k in any of its four coordinate columns.  No reference is needed for that; the bound is the
    one the oracle's own composition of the same witness shows (`low_degree_tail`), asserted of the oracle first, never
    read off the op.  One changed main cell - the is_last flag of row 0, or row 0's multiplicity for a lookup component, with the
    interaction trace left as it was - must leave a non-zero upper half."""
    from oracle import air, fft
    from oracle.prover import gen_interaction_trace
    comp = air.COMPONENTS[kind]
    rng = np.random.default_rng([kind, k, 5])
    tag = "low-degree identity, kind %d, 2^%d rows" % (kind, k)
    e = k + 1
    main, pre = valid_witness(kind, k, rng)
    elems = relation_elements(rng)
    coeffs = [qword("random", rng) for _ in range(comp.n_constraints)]
    pre_l = list(pre) if pre is not None else ()
    # the oracle's side: it fixes the bound, and shows that the changed cell breaks it
    o_inter, o_claimed = gen_interaction_trace(comp, main, _oracle_elems(elems), pre_l)
    o_inter, o_claimed = np.stack(o_inter), tuple(int(v) for v in o_claimed.v)

    def extend(a):
        return fft.evaluate(fft.interpolate(np.asarray(a, dtype=U64)), e)
    inter_e = extend(o_inter)
    pre_e = extend(pre) if pre is not None else None
    changed = main.copy()
    cell = comp.padding.index(1) if comp.n_local else comp.relations[0].mult        # is_last: the padding row's only 1
    changed[cell, 0] = (int(changed[cell, 0]) + 2) % P
    o_vals = {}
    for name, m in (("valid", main), ("changed", changed)):
        o_vals[name] = _oracle_composition(comp, k, extend(m), inter_e, pre_e, elems, o_claimed, coeffs)
        co = fft.interpolate(o_vals[name])
        if name == "valid":
            assert not low_degree_tail(co, k).any() and co[:, :1 << k].any(), "oracle: " + tag
            assert co[:, 1 << k].any(), "oracle: index 2^k is zero too, the bound is lower than recorded: " + tag
        else:
            assert low_degree_tail(co, k).any(), "oracle: the changed cell is not seen: " + tag
    # the ops
    hm = ctx.col_from_cpu(main)
    hp = ctx.col_from_cpu(pre) if pre is not None else None
    inter, claimed = ctx.col_logup(kind, hm, hp, {i: el for i, el in enumerate(elems)})
    assert claimed == o_claimed, (tag, claimed, o_claimed)
    lde = [inter.interpolate().evaluate(e), hp.interpolate().evaluate(e) if hp is not None else None]
    for x in (hm, hp, inter):
        if x is not None:
            x.free()
    for name, m in (("valid", main), ("changed", changed)):
        hm = ctx.col_from_cpu(m)
        me = hm.interpolate().evaluate(e)
        acc = ctx.col_zeros(4, e)
        ctx.col_composition(kind, me, lde[0], lde[1], {i: el for i, el in enumerate(elems)}, claimed, coeffs, acc)
        same(acc.to_cpu(), o_vals[name], "%s, %s witness: composition values" % (tag, name))
        co = acc.interpolate().to_cpu()
        canonical(co, tag)
        for x in (hm, me, acc):
            x.free()
        if name == "valid":
            up = low_degree_tail(co, k)
            assert not up.any(), "%s: %d non-zero coefficients of index > 2^%d, first at (column, index) %s" % (
                tag, np.count_nonzero(up), k, tuple(np.argwhere(up)[0] + [0, (1 << k) + 1]))
        else:
            assert low_degree_tail(co, k).any(), "%s: a changed main cell leaves the upper coefficients zero" % tag
    for x in lde:
        if x is not None:
            x.free()
