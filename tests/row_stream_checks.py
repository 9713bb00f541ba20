"""Checks of the row sinks (`lmn_rows_*`, luminair_amd.backend.RowSink), shared by the emulation suite
(tests/test_row_stream_emu.py, in process) and the GPU suite (tests/test_gpu_row_stream.py, one child process per check:
`python tests/row_stream_checks.py <library> <check>`).  The reference of every byte comparison is `lmn_prove` on the same
rows as plain host tables - the path the oracle pins (tests/test_emu_hostlogic.py, tests/test_gpu_parity.py)."""
import ctypes as C
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from luminair_amd import backend, synthetic as syn   # noqa: E402
from luminair_amd.pie import LuminairPie              # noqa: E402
from luminair_amd.prover import ProverPool            # noqa: E402

P = (1 << 31) - 1
PRIMES = (1, 3, 61, 257, 1021)
MODES = ("pageable", "pinned", "mixed")

_ctx_cache = {}


def ctx_for(lib, variant=backend.VARIANT_KAT, log_blowup=1):
    key = (id(lib), variant, log_blowup)
    if key not in _ctx_cache:
        cfg = lib.default_config()
        cfg.protocol_variant = variant
        cfg.log_blowup = log_blowup
        _ctx_cache[key] = backend.Context(0, cfg, lib)
    return _ctx_cache[key]


# ---- chunkings: lists of chunk lengths that sum to n
def one_chunk(n):
    return [n]


def single_rows(n):
    return [1] * n


def primes_cycled(n):
    out, left = [], n
    for p in itertools.cycle(PRIMES):
        if left == 0:
            break
        out.append(min(p, left))
        left -= out[-1]
    return out


def tile_borders(n):
    """chunk borders at 63 / 64 / 65 and 255 / 256 / 257 rows (as far as the table reaches), then the rest"""
    out, at = [], 0
    for border in (63, 64, 65, 255, 256, 257):
        if border < n:
            out.append(border - at)
            at = border
    out.append(n - at)
    return out


def chunkings(n):
    cs = [("one", one_chunk(n)), ("primes", primes_cycled(n)), ("borders", tile_borders(n))]
    if n <= 64:
        cs.append(("rows", single_rows(n)))
    return cs


def padded_columns(lib, kind, rows):
    """numpy's own transpose + lmn_kind_padding_row padding: what a finished sink must hold"""
    ncols = lib.kind_columns(kind)
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1, ncols)
    size = max(16, 1 << max(len(rows) - 1, 0).bit_length())
    pad = (C.c_uint32 * ncols)()
    assert lib.lib.lmn_kind_padding_row(kind, pad) == 0
    full = np.tile(np.array(list(pad), dtype=np.uint32), (size, 1))
    full[:len(rows)] = rows
    return np.ascontiguousarray(full.T)


def fill(sink, rows, lengths, mode, pinned_src=None):
    """push `rows` in chunks of `lengths`; `pinned_src` = the same rows in page-locked memory"""
    assert sum(lengths) == len(rows)
    at = 0
    for i, m in enumerate(lengths):
        use_pinned = mode == "pinned" or (mode == "mixed" and i % 2 == 1)
        if use_pinned:
            sink.push_pinned(pinned_src[at:at + m])
        else:
            sink.push(rows[at:at + m])
        at += m
    return sink


class Pinned:
    """the tables of a pie copied into page-locked memory once"""

    def __init__(self, lib, tabs):
        self.bufs = []
        for _, r in tabs:
            b = lib.host_rows(r.shape)
            b.array[...] = r
            self.bufs.append(b)

    def __getitem__(self, i):
        return self.bufs[i].array

    def free(self):
        for b in self.bufs:
            b.free()


def prove_from_sinks(ctx, tabs, lengths_of, mode, pinned, luts=None, capacity_of=None, check_columns=True):
    sinks = []
    try:
        for i, (k, r) in enumerate(tabs):
            cap = capacity_of(len(r)) if capacity_of else len(r)
            s = ctx.row_sink(k, cap)
            sinks.append(s)
            fill(s, r, lengths_of(len(r)), mode, pinned[i] if pinned is not None else None)
            assert s.n_rows == len(r)
            s.finish()
            assert s.table.flags == backend.TABLE_COLS_ON_DEVICE and s.table.n_rows == len(r) and s.table.kind == k
            if check_columns:
                assert np.array_equal(s.columns(), padded_columns(ctx.lib, k, r)), (k, len(r), mode)
        return ctx.prove_tables([(k, s, len(r)) for (k, r), s in zip(tabs, sinks)], luts)
    finally:
        for s in sinks:
            s.close()


def small_pies():
    """(name, context variant, log_blowup, tables, luts)"""
    K, PIN = backend.VARIANT_KAT, backend.VARIANT_PINNED
    pies = [("add-5000", K, 1, syn.config2_add_only(5000, 1), None)]
    act, luts = syn.activation_graph(50, 8, names=("sin",), ranges={"sin": (-800, 800)})
    mixed = sorted(syn.chain_graph(300, 3) + act, key=lambda t: t[0])   # Add + Mul + Recip + Sin + SinLookup (n_pre > 0) + Inputs
    pies.append(("chain+sin-lut", PIN, 1, mixed, luts))
    for n in (1, 16, 17, 1024, 1025):
        pies.append(("add-%d" % n, K, 1, syn.config2_add_only(n, n), None))
    pies.append(("add-300-blowup4", K, 2, syn.config2_add_only(300, 2), None))
    return [(nm, v, lb, [(k, np.ascontiguousarray(r, dtype=np.uint32)) for k, r in tabs], luts)
            for nm, v, lb, tabs, luts in pies]


# ------------------------------------------------------------------------------------------------ the checks
def check_byte_identity(lib):
    """item 1 (and the columns of item 2 on the way): every pie x chunking x push mode"""
    for name, variant, lb, tabs, luts in small_pies():
        ctx = ctx_for(lib, variant, lb)
        want = ctx.prove_tables([(k, r, len(r)) for k, r in tabs], luts)
        pinned = Pinned(lib, tabs)
        try:
            labels = [c[0] for c in chunkings(max(len(r) for _, r in tabs))]
            for label in labels:
                lengths_of = lambda n, label=label: dict(chunkings(n)).get(label) or one_chunk(n)   # noqa: E731
                for mode in MODES:
                    got = prove_from_sinks(ctx, tabs, lengths_of, mode, pinned, luts)
                    assert got == want, (name, label, mode)
        finally:
            pinned.free()


def check_columns_as_data(lib):
    """item 2: the finished column block, downloaded, against numpy - chunk borders inside, at and across the tiles"""
    ctx = ctx_for(lib)
    for n in (1, 15, 16, 17, 255, 256, 257, 700, 4097):
        for kind, rows in (syn.config2_add_only(n, n)[0], syn.chain_graph(n, n)[1]):
            rows = np.ascontiguousarray(rows, dtype=np.uint32)
            for label, lengths in chunkings(n):
                with ctx.row_sink(kind, n) as s:
                    fill(s, rows, lengths, "pageable").finish()
                    assert np.array_equal(s.columns(), padded_columns(lib, kind, rows)), (kind, n, label)


def check_compaction(lib):
    """item 3: capacity larger than needed by two powers of two and more"""
    ctx = ctx_for(lib)
    tabs = [(k, np.ascontiguousarray(r, dtype=np.uint32)) for k, r in syn.chain_graph(300, 4)]
    want = ctx.prove_tables([(k, r, len(r)) for k, r in tabs])
    for factor in (4, 16, 27):      # 512-row columns inside strides of 2048, 8192, 8192
        got = prove_from_sinks(ctx, tabs, primes_cycled, "pageable", None, capacity_of=lambda n: n * factor)
        assert got == want, factor


def check_mixed_pie(lib):
    """item 4: one sink table, one plain host table, one ROWS_ON_DEVICE table"""
    ctx = ctx_for(lib)
    (ka, ra), (km, rm), (kr, rr) = [(k, np.ascontiguousarray(r, dtype=np.uint32)) for k, r in syn.chain_graph(700, 5)]
    want = ctx.prove_tables([(ka, ra, len(ra)), (km, rm, len(rm)), (kr, rr, len(rr))])
    dev = ctx.upload(rr)
    try:
        with ctx.row_sink(ka, len(ra)) as s:
            fill(s, ra, primes_cycled(len(ra)), "pageable").finish()
            assert ctx.prove_tables([(ka, s, len(ra)), (km, rm, len(rm)), (kr, dev, len(rr))]) == want
        with ctx.row_sink(km, len(rm)) as s:          # ... and the sink in the middle of the pie
            fill(s, rm, tile_borders(len(rm)), "pageable").finish()
            assert ctx.prove_tables([(ka, ra, len(ra)), (km, s, len(rm)), (kr, dev, len(rr))]) == want
    finally:
        dev.free()


def _rc(call, *args):
    return int(call(*args))


def check_errors(lib, gpu=False):
    """item 5"""
    L, INV = lib.lib, backend.ERR_INVALID_ARGUMENT
    ctx = ctx_for(lib)
    kind, rows = syn.config2_add_only(600, 7)[0]
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    want = ctx.prove_tables([(kind, rows, len(rows))])
    lengths = [100, 156, 44, 300]
    # a non-canonical word in the first / a middle / the last chunk: finish refuses, reset + good rows prove
    for word in (P, 0xFFFFFFFF):
        for chunk in (0, 2, 3):
            bad = rows.copy()
            bad[sum(lengths[:chunk]) + lengths[chunk] // 2, 5] = word
            with ctx.row_sink(kind, len(rows)) as s:
                fill(s, bad, lengths, "pageable")
                t = backend.LmnTable()
                assert _rc(L.lmn_rows_finish, s.handle, C.byref(t)) == INV, (word, chunk)
                assert b"canonical" in L.lmn_last_error(None)
                assert _rc(L.lmn_rows_push, s.handle, rows.ctypes.data, 1) == INV     # a failed sink takes no rows
                s.reset()
                assert s.n_rows == 0
                fill(s, rows, lengths, "pageable").finish()
                assert ctx.prove_tables([(kind, s, len(rows))]) == want, (word, chunk)
    # the context is usable after a refused sink
    assert ctx.prove_tables([(kind, rows, len(rows))]) == want
    # beyond capacity: refused, the sink keeps what it had
    with ctx.row_sink(kind, len(rows)) as s:
        s.push(rows[:500])
        assert _rc(L.lmn_rows_push, s.handle, rows.ctypes.data, 101) == INV
        assert b"capacity" in L.lmn_last_error(None)
        assert s.n_rows == 500
        s.push(rows[500:]).finish()
        assert ctx.prove_tables([(kind, s, len(rows))]) == want
        # push / finish after finish without reset
        assert _rc(L.lmn_rows_push, s.handle, rows.ctypes.data, 1) == INV
        assert _rc(L.lmn_rows_finish, s.handle, C.byref(backend.LmnTable())) == INV
        # a sharded context refuses the table, and says so
        ctx.set_shard(0, 1, lambda buf, nbytes, stream: None)
        try:
            try:
                ctx.prove_tables([(kind, s, len(rows))])
                raise AssertionError("a sharded context took a LMN_TABLE_COLS_ON_DEVICE table")
            except backend.LuminairBackendError as e:
                assert e.code == INV and "sharded" in str(e)
        finally:
            ctx.clear_shard()
        assert ctx.prove_tables([(kind, s, len(rows))]) == want
        # columns that no live finished sink stands behind
        stale = (kind, s.table.rows, len(rows))
        s.reset()
        arr = (backend.LmnTable * 1)()
        arr[0].kind, arr[0].flags, arr[0].n_rows, arr[0].rows = stale[0], backend.TABLE_COLS_ON_DEVICE, stale[2], stale[1]
        out, out_len = C.POINTER(C.c_uint8)(), C.c_size_t()
        assert _rc(L.lmn_prove, ctx.handle, arr, 1, None, C.byref(out), C.byref(out_len)) == INV
    # zero rows at finish: the code lmn_prove gives for a table of zero rows
    arr = (backend.LmnTable * 1)()
    arr[0].kind, arr[0].flags, arr[0].n_rows, arr[0].rows = kind, 0, 0, rows.ctypes.data
    out, out_len = C.POINTER(C.c_uint8)(), C.c_size_t()
    empty = _rc(L.lmn_prove, ctx.handle, arr, 1, None, C.byref(out), C.byref(out_len))
    assert empty == backend.ERR_EMPTY_TRACE
    with ctx.row_sink(kind, 10) as s:
        assert _rc(L.lmn_rows_finish, s.handle, C.byref(backend.LmnTable())) == empty
        s.push(rows[:3]).finish()                      # and the sink goes on
    # arguments
    h = C.c_void_p()
    assert _rc(L.lmn_rows_open, None, kind, 10, C.byref(h)) == INV
    assert _rc(L.lmn_rows_open, ctx.handle, kind, 10, None) == INV
    assert _rc(L.lmn_rows_open, ctx.handle, 99, 10, C.byref(h)) == INV and not h.value
    assert _rc(L.lmn_rows_open, ctx.handle, kind, 0, C.byref(h)) == INV
    assert _rc(L.lmn_rows_open, ctx.handle, kind, (1 << 26) + 1, C.byref(h)) == INV
    assert _rc(L.lmn_rows_push, None, rows.ctypes.data, 1) == INV
    assert _rc(L.lmn_rows_push_pinned, None, rows.ctypes.data, 1) == INV
    assert _rc(L.lmn_rows_sync, None) == INV and _rc(L.lmn_rows_finish, None, None) == INV
    assert _rc(L.lmn_rows_reset, None) == INV and int(L.lmn_rows_count(None)) == 0
    L.lmn_rows_close(None)
    with ctx.row_sink(kind, 10) as s:
        assert _rc(L.lmn_rows_push, s.handle, None, 1) == INV
        assert _rc(L.lmn_rows_push, s.handle, rows.ctypes.data, 0) == INV
        assert _rc(L.lmn_rows_push_pinned, s.handle, None, 1) == INV
        assert _rc(L.lmn_rows_finish, s.handle, None) == INV
        if gpu:     # the runtime can tell: ordinary memory handed to the pinned form is refused, not copied slowly
            assert _rc(L.lmn_rows_push_pinned, s.handle, rows.ctypes.data, 5) == INV
            assert b"page-locked" in L.lmn_last_error(None)
            assert s.n_rows == 0
            lib.host_register(rows)                    # ... and registered memory is taken
            try:
                s.push_pinned(rows[2:9]).sync()
                assert s.n_rows == 7
            finally:
                lib.host_unregister(rows)


def check_reuse_and_pool(lib):
    """item 6: the same finished sink proved twice; two sinks of two pies in flight through submit / wait"""
    ctx = ctx_for(lib)
    ta = [(k, np.ascontiguousarray(r, dtype=np.uint32)) for k, r in syn.chain_graph(300, 11)]
    tb = [(k, np.ascontiguousarray(r, dtype=np.uint32)) for k, r in syn.config2_add_only(1500, 12)]
    want_a = ctx.prove_tables([(k, r, len(r)) for k, r in ta])
    want_b = ctx.prove_tables([(k, r, len(r)) for k, r in tb])
    sinks_a = [fill(ctx.row_sink(k, len(r)), r, primes_cycled(len(r)), "pageable").finish() for k, r in ta]
    sinks_b = [fill(ctx.row_sink(k, len(r)), r, tile_borders(len(r)), "pageable").finish() for k, r in tb]
    try:
        for _ in range(2):
            assert ctx.prove_tables([(s.kind, s, s.n_rows) for s in sinks_a]) == want_a
        pool = ProverPool(0, 2, library=lib)
        try:
            pies = [LuminairPie.from_tables(sinks_a), LuminairPie.from_tables(sinks_b)] * 2
            got = [p.to_bincode() for p in pool.prove_many(pies)]
            assert got == [want_a, want_b] * 2
        finally:
            pool.close()
    finally:
        for s in sinks_a + sinks_b:
            s.close()


# ---- GPU only
def _add_table(n, seed):
    kind, rows = syn.config2_add_only(n, seed)[0]
    return kind, np.ascontiguousarray(rows, dtype=np.uint32)


def check_config2a(lib):
    """BASELINE config 2a at full size: chunks of 4 096 * k rows, one ragged chunking, all three push modes"""
    ctx = ctx_for(lib)
    kind, rows = _add_table(1 << 20, 42)
    n = len(rows)
    want = ctx.prove_tables([(kind, rows, n)])
    pinned = Pinned(lib, [(kind, rows)])
    try:
        ragged = primes_cycled(100003) + [n - 100003]
        for label, lengths in (("4096", [4096] * (n // 4096)), ("65536", [65536] * 16), ("3x4096", [12288] * 85 + [n - 85 * 12288]),
                               ("ragged", ragged)):
            for mode in MODES:
                got = prove_from_sinks(ctx, [(kind, rows)], lambda _n: lengths, mode, pinned, check_columns=label == "ragged")
                assert got == want, (label, mode)
    finally:
        pinned.free()


def check_big_table(lib):
    """a 2^22-row table once (the staging ring wraps many times; a chunk far larger than a slot)"""
    ctx = ctx_for(lib)
    kind, rows = _add_table(1 << 22, 43)
    n = len(rows)
    want = ctx.prove_tables([(kind, rows, n)])
    got = prove_from_sinks(ctx, [(kind, rows)], lambda _n: [1000003, n - 1000003], "pageable", None, check_columns=False)
    assert got == want


def check_overlap(lib):
    """fill sink B while the proof of sink A is in flight on the same context, 8 alternations"""
    ctx = ctx_for(lib)
    n = 1 << 18
    tables = [_add_table(n, 100 + i) for i in range(8)]
    want = [ctx.prove_tables([(k, r, n)]) for k, r in tables]
    sinks = [ctx.row_sink(tables[0][0], n), ctx.row_sink(tables[0][0], n)]
    try:
        got = []
        fill(sinks[0], tables[0][1], [n // 16] * 16, "pageable").finish()
        for i in range(8):
            cur, nxt = sinks[i % 2], sinks[(i + 1) % 2]
            ctx.prove_submit([(cur.kind, cur, n)])
            if i + 1 < 8:        # the next pie's rows arrive while the proof runs
                fill(nxt.reset(), tables[i + 1][1], [n // 16] * 16, "pageable").finish()
            got.append(ctx.prove_wait())
        assert got == want
    finally:
        for s in sinks:
            s.close()


GPU_CHECKS = {
    "byte_identity": check_byte_identity, "columns_as_data": check_columns_as_data, "compaction": check_compaction,
    "errors": lambda lib: check_errors(lib, gpu=True), "config2a": check_config2a, "big_table": check_big_table,
    "overlap": check_overlap,
}

if __name__ == "__main__":
    GPU_CHECKS[sys.argv[2]](backend.Library(sys.argv[1]))
    print("ok", sys.argv[2])
