"""`lmn_col_batch_inverse` / `lmn_col_batch_inverse_secure` (FieldOps::batch_inverse on device columns; kernels
k_batch_inverse_m / k_batch_inverse_q) at their value and shape edges.  Run against the emulation build on CPU
(tests/test_field_ops_emu.py) and the HIP library on GPU (tests/test_gpu_field_ops.py).

Reference.  Up to 2^8 rows: plain Python integers - `pow(x, P - 2, P)` for M31, `numeric_checks.q_inv` (through CM31) for
QM31.  Above: the defining identity in numpy uint64 (every product is below 2^62): x * out == 1 for every non-zero x,
out == 0 where x == 0, every word < P.  Inverses are unique, so the identity is a complete specification.

The contract for zero (include/luminair_hip.h): a zero element gives 0, changes no other element, and is counted - words
for the M31 form, QM31 elements for the secure form."""
import ctypes as C

import numpy as np

import numeric_checks as nc

P, U64 = nc.P, nc.U64
TPB = 256                      # kernels_common.h: a lane's elements are TPB words apart, a tile is TPB * E words
LOGS = tuple(range(14))        # fewer words than a wave .. one wave .. TPB .. one tile and several for any E up to 32
NCOLS = (1, 2, 3, 5)
VIEW_LOGS = (0, 1, 2, 8)
INVALID_ARGUMENT = -6


# ----------------------------------------------------------------------------- references
def np_mul(a, b):
    return (a * b) % U64(P)


def np_c_mul(a, b):
    return ((np_mul(a[0], b[0]) + U64(P) - np_mul(a[1], b[1])) % U64(P), (np_mul(a[0], b[1]) + np_mul(a[1], b[0])) % U64(P))


def np_q_mul(x, y):
    """(4, n) * (4, n) in QM31 = CM31[u] / (u^2 - 2 - i)"""
    A, B, Cc, D = (x[0], x[1]), (x[2], x[3]), (y[0], y[1]), (y[2], y[3])
    bd = np_c_mul(B, D)
    rbd = ((U64(2) * bd[0] + U64(P) - bd[1]) % U64(P), (bd[0] + U64(2) * bd[1]) % U64(P))
    ac, ad, bc = np_c_mul(A, Cc), np_c_mul(A, D), np_c_mul(B, Cc)
    return np.stack([(ac[0] + rbd[0]) % U64(P), (ac[1] + rbd[1]) % U64(P), (ad[0] + bc[0]) % U64(P), (ad[1] + bc[1]) % U64(P)])


def check_m31_result(got, x, what):
    """got, x: (ncols, n).  -> the number of zero words of x"""
    got, x = np.asarray(got).astype(U64), np.asarray(x).astype(U64)
    assert got.shape == x.shape, (what, got.shape, x.shape)
    nc.canonical(got, what)
    if x.shape[1] <= 1 << nc.PY_MAX_LOG:
        want = np.array([[pow(int(v), P - 2, P) if v else 0 for v in col] for col in x], dtype=U64).reshape(x.shape)
        nc.same(got, want, what)
    else:
        zero = x == 0
        assert not got[zero].any(), "%s: %d zero words have a non-zero result" % (what, np.count_nonzero(got[zero]))
        prod = np_mul(x, got)
        bad = np.argwhere(~zero & (prod != 1))
        assert not len(bad), "%s: x * out != 1 at %d words, first at %s" % (what, len(bad), tuple(bad[0]))
    return int(np.count_nonzero(x == 0))


def check_qm31_result(got, x, what):
    """got, x: (4, n).  -> the number of zero elements of x"""
    got, x = np.asarray(got).astype(U64), np.asarray(x).astype(U64)
    assert got.shape == x.shape and x.shape[0] == 4, (what, got.shape, x.shape)
    nc.canonical(got, what)
    zero = ~x.any(axis=0)
    if x.shape[1] <= 1 << nc.PY_MAX_LOG:
        want = np.zeros_like(x)
        for i in range(x.shape[1]):
            if not zero[i]:
                want[:, i] = nc.q_inv(tuple(int(v) for v in x[:, i]))
        nc.same(got, want, what)
    else:
        assert not got[:, zero].any(), "%s: %d zero elements have a non-zero result" % (what, np.count_nonzero(got[:, zero].any(axis=0)))
        prod = np_q_mul(x, got)
        one = np.array([1, 0, 0, 0], dtype=U64)[:, None]
        bad = np.argwhere(~zero & (prod != one).any(axis=0))
        assert not len(bad), "%s: x * out != 1 at %d elements, first at %d" % (what, len(bad), int(bad[0][0]))
    return int(np.count_nonzero(zero))


# ----------------------------------------------------------------------------- one op, every calling form
def run_every_form(ctx, x, secure, what):
    """x (ncols, n) through the op out of place with the count, out of place without it, and in place: the three must
    write the same bytes, the source of the out-of-place calls must stay as it was, the count must be the reference's"""
    check = check_qm31_result if secure else check_m31_result
    x = np.asarray(x).astype(U64)
    junk = np.full(x.shape, P - 1, dtype=U64)
    src = ctx.col_from_cpu(x)
    d1, d2 = ctx.col_from_cpu(junk), ctx.col_from_cpu(junk)
    call = (lambda h, **kw: h.batch_inverse_secure(**kw)) if secure else (lambda h, **kw: h.batch_inverse(**kw))
    try:
        out, n_zero = call(src, out=d1, count_zeros=True)
        assert out is d1
        got = d1.to_cpu()
        want_zero = check(got, x, what + ", out of place, counting")
        assert n_zero == want_zero, "%s: %d zeros counted, the input has %d" % (what, n_zero, want_zero)
        assert call(src, out=d2) is d2
        nc.same(d2.to_cpu(), got, what + ": without the count against with it")
        nc.same(src.to_cpu(), x, what + ": the source after the out-of-place calls")
        assert call(src) is src
        nc.same(src.to_cpu(), got, what + ": in place against out of place")
        out, n_zero = call(src, count_zeros=True)        # the results back in place: zeros stay zeros, the count too
        assert n_zero == want_zero, "%s, second pass in place: %d zeros counted, want %d" % (what, n_zero, want_zero)
        back = src.to_cpu().astype(U64)
        nc.same(back, x, what + ": the inverse of the inverse")
        return got
    finally:
        for h in (src, d1, d2):
            h.free()


def check_m31_classes(ctx, log, ncols_list=NCOLS, classes=nc.CLASSES):
    n = 1 << log
    for ncols in ncols_list:
        for cls in classes:
            rng = np.random.default_rng([log, ncols, nc.CLASSES.index(cls)])
            run_every_form(ctx, nc.words(cls, (ncols, n), rng), False, "batch_inverse log %d ncols %d %s" % (log, ncols, cls))


def zero_positions(n):
    return sorted({i for i in (0, 1, TPB - 1, TPB, n // 2, n - 1) if 0 <= i < n})


def check_m31_one_zero(ctx, log):
    """a random non-zero column with a single zero at each of the lane, wave and tile positions; all zero but one"""
    n = 1 << log
    rng = np.random.default_rng([log, 71])
    base = rng.integers(1, P, size=(2, n), dtype=U64)
    for at in zero_positions(n):
        x = base.copy()
        x[1, at] = 0
        run_every_form(ctx, x, False, "batch_inverse log %d, one zero at %d" % (log, at))
        x = np.zeros((2, n), dtype=U64)
        x[0, at] = base[0, at]
        run_every_form(ctx, x, False, "batch_inverse log %d, all zero but index %d" % (log, at))


def qm31_class(cls, n, rng):
    return nc.words(cls, (4, n), rng)


def check_qm31_classes(ctx, log, classes=nc.CLASSES):
    n = 1 << log
    for cls in classes:
        rng = np.random.default_rng([log, 4, nc.CLASSES.index(cls)])
        run_every_form(ctx, qm31_class(cls, n, rng), True, "batch_inverse_secure log %d %s" % (log, cls))


def check_qm31_subsets(ctx, log):
    """elements supported exactly on each of the 15 non-empty subsets of the four coordinates (A = 0 and B = 0 among
    them); on (a, 0, 0, 0) the secure form is the M31 form in coordinate 0 and 0 in the other three"""
    n = 1 << log
    rng = np.random.default_rng([log, 15])
    for mask in range(1, 16):
        x = rng.integers(1, P, size=(4, n), dtype=U64)
        for k in range(4):
            if not mask >> k & 1:
                x[k] = 0
        got = run_every_form(ctx, x, True, "batch_inverse_secure log %d, support mask %d" % (log, mask))
        if mask == 1:
            base = run_every_form(ctx, x[:1], False, "batch_inverse log %d, the base-field column" % log)
            nc.same(got[:1], base, "secure form on (a, 0, 0, 0) against the M31 form, log %d" % log)
            assert not got[1:].any(), "secure form on (a, 0, 0, 0): a non-zero word outside coordinate 0"


def check_qm31_one_zero(ctx, log):
    n = 1 << log
    rng = np.random.default_rng([log, 72])
    base = rng.integers(1, P, size=(4, n), dtype=U64)
    for at in zero_positions(n):
        x = base.copy()
        x[:, at] = 0
        run_every_form(ctx, x, True, "batch_inverse_secure log %d, one zero at %d" % (log, at))
        x = np.zeros((4, n), dtype=U64)
        x[:, at] = base[:, at]
        run_every_form(ctx, x, True, "batch_inverse_secure log %d, all zero but index %d" % (log, at))


# ----------------------------------------------------------------------------- views
PARENT_COLS = 16      # the view starts at column 1: its base is only 4-byte aligned at log sizes 0 and 1


def check_views(ctx, log, secure):
    """src and dst as views (first = 1) of two parents, then of one parent in place: the right words in the view, the
    parents' other columns unchanged word for word"""
    n = 1 << log
    k = 4 if secure else 2
    what = "%s on views, log %d" % ("batch_inverse_secure" if secure else "batch_inverse", log)
    check = check_qm31_result if secure else check_m31_result
    rng = np.random.default_rng([log, int(secure), 73])
    xs = rng.integers(0, P, size=(PARENT_COLS, n), dtype=U64)
    xs[1, 0] = 0                                               # a zero inside the view
    xd = rng.integers(1, P, size=(PARENT_COLS, n), dtype=U64)
    ps, pd = ctx.col_from_cpu(xs), ctx.col_from_cpu(xd)
    vs, vd = ps.view(1, k), pd.view(1, k)
    call = (lambda h, **kw: h.batch_inverse_secure(**kw)) if secure else (lambda h, **kw: h.batch_inverse(**kw))
    try:
        _, n_zero = call(vs, out=vd, count_zeros=True)
        got = pd.to_cpu().astype(U64)
        want_zero = check(got[1:1 + k], xs[1:1 + k], what)
        assert n_zero == want_zero, (what, n_zero, want_zero)
        nc.same(got[:1], xd[:1], what + ": the destination parent's column before the view")
        nc.same(got[1 + k:], xd[1 + k:], what + ": the destination parent's columns after the view")
        nc.same(ps.to_cpu(), xs, what + ": the source parent")
        call(vs)                                               # in place on the view
        after = ps.to_cpu().astype(U64)
        nc.same(after[1:1 + k], got[1:1 + k], what + ": in place on the view")
        nc.same(after[:1], xs[:1], what + ", in place: the parent's column before the view")
        nc.same(after[1 + k:], xs[1 + k:], what + ", in place: the parent's columns after the view")
    finally:
        for h in (vs, vd, ps, pd):
            h.free()


# ----------------------------------------------------------------------------- refusals
def check_refusals(ctx):
    """every refusal of the contract: LMN_ERR_INVALID_ARGUMENT, a text that names the argument, the destination as it
    was, and the same context completes a valid call afterwards"""
    L = ctx.lib.lib
    rng = np.random.default_rng(74)
    log, n = 4, 16
    fns = {False: L.lmn_col_batch_inverse, True: L.lmn_col_batch_inverse_secure}

    def cols(ncols, lg=log):
        a = rng.integers(1, P, size=(ncols, 1 << lg), dtype=U64)
        return a, ctx.col_from_cpu(a)

    def refused(secure, src, dst, names, watch, what):
        """watch: (handle, expected words) pairs that must be unchanged after the refusal"""
        for counted in (False, True):
            n_zero = C.c_uint64(12345)
            rc = fns[secure](ctx.handle, src, dst, C.byref(n_zero) if counted else None)
            text = L.lmn_last_error(ctx.handle).decode()
            assert rc == INVALID_ARGUMENT, (what, rc, text)
            assert names in text, "%s: the text %r does not name %r" % (what, text, names)
            assert n_zero.value == 12345, (what, "the count was written")
            for h, words in watch:
                nc.same(h.to_cpu(), words, what + ": a handle after the refusal")
        # the context and the handles stay usable
        run_every_form(ctx, rng.integers(0, P, size=(4, n), dtype=U64), True, "after the refusal of " + what)

    a3, h3 = cols(3)
    a4, h4 = cols(4)
    b4, g4 = cols(4)
    a5, h5 = cols(5)
    a4big, h4big = cols(4, log + 1)
    a1, h1 = cols(1)
    try:
        for secure in (False, True):
            refused(secure, None, g4.handle, "src is null", [(g4, b4)], "a null source")
            refused(secure, h4.handle, None, "dst is null", [(h4, a4)], "a null destination")
            refused(secure, h4.handle, h4big.handle, "dst", [(h4big, a4big), (h4, a4)], "a destination of another log size")
        refused(False, h4.handle, h3.handle, "dst", [(h3, a3), (h4, a4)], "a destination with fewer columns")
        refused(False, h3.handle, h4.handle, "dst", [(h4, a4)], "a destination with more columns")
        refused(True, h3.handle, h3.handle, "src", [(h3, a3)], "a secure source of 3 columns")
        refused(True, h5.handle, h5.handle, "src", [(h5, a5)], "a secure source of 5 columns")
        refused(True, h4.handle, h1.handle, "dst", [(h1, a1), (h4, a4)], "a secure destination of 1 column")
        # partial overlaps: views of one parent, shifted by one column, either way round
        lo, hi = h5.view(0, 4), h5.view(1, 4)
        for secure in (False, True):
            refused(secure, lo.handle, hi.handle, "dst overlaps src", [(h5, a5)], "a destination one column above the source")
            refused(secure, hi.handle, lo.handle, "dst overlaps src", [(h5, a5)], "a destination one column below the source")
        lo.free()
        hi.free()
        # a handle over exactly the same range is the in-place form
        same_range = h4.view(0, 4)
        out, n_zero = h4.batch_inverse_secure(out=same_range, count_zeros=True)
        check_qm31_result(h4.to_cpu(), a4, "a view over the whole source as destination")
        assert n_zero == 0
        same_range.free()
    finally:
        for h in (h3, h4, g4, h5, h4big, h1):
            h.free()
    with_null_ctx = L.lmn_col_batch_inverse(None, None, None, None)
    assert with_null_ctx == INVALID_ARGUMENT


# ----------------------------------------------------------------------------- large sizes (GPU only)
def check_large(ctx, log, secure, cls):
    rng = np.random.default_rng([log, int(secure), 75])
    x = nc.words(cls, (4 if secure else 1, 1 << log), rng)
    check = check_qm31_result if secure else check_m31_result
    src = ctx.col_from_cpu(x)
    try:
        if secure:
            _, n_zero = src.batch_inverse_secure(count_zeros=True)
        else:
            _, n_zero = src.batch_inverse(count_zeros=True)
        want_zero = check(src.to_cpu(), x, "%s log %d %s" % ("secure" if secure else "m31", log, cls))
        assert n_zero == want_zero, (log, secure, cls, n_zero, want_zero)
    finally:
        src.free()
