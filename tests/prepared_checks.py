"""Shared checks of the settings prepared once (`lmn_settings_prepare`, `lmn_prove_prepared`, `lmn_prove_submit_prepared`,
`lmn_batch_prove_prepared`; `backend.PreparedSettings`).  tests/test_prepared_emu.py runs them on the emulation build,
tests/test_gpu_prepared.py on the MI355X.

The yardstick is the existing path on the same pie: the bytes of `lmn_prove(tables, settings)`, which the GPU parity tests
tie to the oracle.  Every case also goes through `lmn_verify`, and the prepared root must be `commitments[0]` of the proof.

Shapes: the smallest at which tree 0 can still go wrong - a LUT of 2^4 rows (the minimum) for each of sin / exp2 / log2
alone; three LUTs of three sizes (2^5, 2^7, 2^6) next to the 256-row range check, so that columns join the tree at four
levels and the size sort moves them; two LUTs of equal size (stable order); the range check alone; no lookups at all."""
import ctypes as C
import hashlib
import threading

import numpy as np

from luminair_amd import backend, synthetic as syn
from luminair_amd.pie import LuminairPie, LuminairProof

PINNED = backend.VARIANT_PINNED
INVALID = backend.ERR_INVALID_ARGUMENT


def config(lib, log_blowup=1, **pcs):
    cfg = lib.default_config()
    cfg.protocol_variant = PINNED
    cfg.log_blowup = log_blowup
    for k, v in pcs.items():
        setattr(cfg, k, v)
    return cfg


def _range(name, log):
    """a fixed-point input range of exactly 2^log values"""
    return (1, 1 << log) if name == "log2" else (-(1 << (log - 1)), (1 << (log - 1)) - 1)


def _pie(tabs):
    return [(k, r, len(r)) for k, r in tabs]


def merge(*graphs):
    """the tables of several balanced graphs as one pie (logup sums add up; tables of one kind are concatenated)"""
    by_kind = {}
    for tabs in graphs:
        for k, rows in tabs:
            by_kind.setdefault(k, []).append(rows)
    return sorted(((k, np.concatenate(v)) for k, v in by_kind.items()), key=lambda kt: kt[0])


def lut_pie(sizes, n=20, seed=1, less_than=False):
    """sizes: {"sin" | "exp2" | "log2": log size}.  -> (pie, luts, lookups)"""
    names = tuple(sizes)
    tabs, luts = syn.activation_graph(n, seed, names=names, ranges={m: _range(m, sizes[m]) for m in names}) if names else ([], {})
    lookups = 0
    for m in names:
        lookups |= backend.LOOKUP_BITS[m]
        assert len(luts[m][0]) == 1 << sizes[m]
    if less_than:
        tabs = merge(tabs, syn.less_than_graph(n, seed + 100))
        lookups |= backend.LOOKUP_RANGE_CHECK
    return _pie(tabs), luts, lookups


CASES = {
    "sin_2^4": dict(sizes={"sin": 4}),
    "exp2_2^4": dict(sizes={"exp2": 4}),
    "log2_2^4": dict(sizes={"log2": 4}),
    "three_sizes_and_range_check": dict(sizes={"sin": 5, "exp2": 7, "log2": 6}, less_than=True),
    "two_equal_sizes": dict(sizes={"sin": 5, "exp2": 5}),
    "range_check_only": dict(sizes={}, less_than=True),
}


def commitment0(proof: bytes) -> bytes:
    return bytes(LuminairProof(proof).to_dict()["proof"]["commitments"][0])


def check_against_plain(lib, ctx, cfg, pie, luts, lookups, prepared=None):
    """prepared bytes == lmn_prove bytes, the proof verifies, the prepared root is commitments[0]"""
    want = ctx.prove_tables(pie, luts)
    own = prepared is None
    pp = prepared or backend.PreparedSettings(ctx.device, cfg, luts, lookups, lib)
    try:
        got = ctx.prove_tables(pie, prepared=pp)
        assert got == want
        assert pp.lookups == lookups
        assert pp.root == commitment0(got)
        lib.verify(got, config=cfg)
    finally:
        if own:
            pp.close()
    return want


def check_case(lib, name, log_blowup=1):
    cfg = config(lib, log_blowup)
    ctx = backend.Context(0, cfg, lib)
    try:
        pie, luts, lookups = lut_pie(**CASES[name])
        check_against_plain(lib, ctx, cfg, pie, luts, lookups)
    finally:
        ctx.close()


def check_no_lookups(lib):
    """lookups == 0: the empty tree, root = blake2s(""), bytes of lmn_prove with null settings"""
    cfg = config(lib)
    ctx = backend.Context(0, cfg, lib)
    try:
        pie = _pie(syn.config2_graph_faithful(40, 5))
        want = ctx.prove_tables(pie)
        with backend.PreparedSettings(0, cfg, None, 0, lib) as pp:
            assert pp.root == hashlib.blake2s(b"").digest()
            assert ctx.prove_tables(pie, prepared=pp) == want
            assert pp.root == commitment0(want)
        # through the C entry with a null settings pointer as well
        h = C.c_void_p()
        assert lib.lib.lmn_settings_prepare(0, C.byref(cfg), None, 0, C.byref(h)) == 0
        lib.lib.lmn_prepared_destroy(h)
    finally:
        ctx.close()


def check_config4(lib):
    """BASELINE config 4's own 2^17-row exp2 LUT: the size the feature is for"""
    cfg = config(lib)
    ctx = backend.Context(0, cfg, lib)
    try:
        tabs, luts = syn.config4_black_scholes_shape(1)
        assert len(luts["exp2"][0]) == 1 << 17
        check_against_plain(lib, ctx, cfg, _pie(tabs), luts, backend.LOOKUP_EXP2)
    finally:
        ctx.close()


def check_two_pies_in_a_row(lib):
    cfg = config(lib)
    ctx = backend.Context(0, cfg, lib)
    try:
        c = CASES["three_sizes_and_range_check"]
        pie_a, luts, lookups = lut_pie(seed=1, **c)
        pie_b, luts_b, _ = lut_pie(seed=2, **c)
        assert all(np.array_equal(luts[m][1], luts_b[m][1]) for m in luts)
        with backend.PreparedSettings(0, cfg, luts, lookups, lib) as pp:
            want_a = check_against_plain(lib, ctx, cfg, pie_a, luts, lookups, pp)
            want_b = check_against_plain(lib, ctx, cfg, pie_b, luts, lookups, pp)
            assert want_a != want_b
            assert ctx.prove_tables(pie_a, prepared=pp) == want_a
    finally:
        ctx.close()


def check_two_threads(lib):
    """one prepared object, two contexts on two threads at once"""
    cfg = config(lib)
    c = CASES["three_sizes_and_range_check"]
    pies = [lut_pie(seed=10 + i, **c) for i in range(2)]
    luts, lookups = pies[0][1], pies[0][2]
    ctxs = [backend.Context(0, cfg, lib) for _ in range(2)]
    try:
        want = [ctxs[i].prove_tables(pies[i][0], luts) for i in range(2)]
        got, errors = [None, None], []
        with backend.PreparedSettings(0, cfg, luts, lookups, lib) as pp:
            def run(i):
                try:
                    for _ in range(2):
                        got[i] = ctxs[i].prove_tables(pies[i][0], prepared=pp)
                        assert got[i] == want[i]
                except BaseException as e:   # noqa: BLE001 - reported by the main thread
                    errors.append(e)
            ths = [threading.Thread(target=run, args=(i,)) for i in range(2)]
            for t in ths:
                t.start()
            for t in ths:
                t.join()
        assert not errors, errors
        assert got == want
    finally:
        for x in ctxs:
            x.close()


def check_submit_wait(lib):
    """prove_submit_prepared on several contexts, then wait; lmn_prepared_destroy between submit and wait"""
    cfg = config(lib)
    c = CASES["two_equal_sizes"]
    pies = [lut_pie(seed=20 + i, **c) for i in range(3)]
    luts, lookups = pies[0][1], pies[0][2]
    ctxs = [backend.Context(0, cfg, lib) for _ in range(3)]
    try:
        want = [ctxs[i].prove_tables(pies[i][0], luts) for i in range(3)]
        pp = backend.PreparedSettings(0, cfg, luts, lookups, lib)
        for i in range(3):
            ctxs[i].prove_submit(pies[i][0], prepared=pp)
        assert [x.prove_wait() for x in ctxs] == want
        # the caller's reference goes away while the proofs are in flight: the library holds its own until the wait
        for i in range(3):
            ctxs[i].prove_submit(pies[i][0], prepared=pp)
        pp.close()
        assert [x.prove_wait() for x in ctxs] == want
        # and with everything prepared destroyed, the plain path is what it was
        assert ctxs[0].prove_tables(pies[0][0], luts) == want[0]
    finally:
        for x in ctxs:
            x.close()


def check_arena_growth(lib, big_rows=700):
    """a larger plain proof on the same context makes its arena move; the prepared object does not live in it"""
    cfg = config(lib)
    ctx = backend.Context(0, cfg, lib)
    try:
        pie, luts, lookups = lut_pie(**CASES["three_sizes_and_range_check"])
        big = _pie(syn.config2_graph_faithful(big_rows, 9))
        with backend.PreparedSettings(0, cfg, luts, lookups, lib) as pp:
            want = check_against_plain(lib, ctx, cfg, pie, luts, lookups, pp)
            ctx.prove_tables(big)
            assert ctx.prove_tables(pie, prepared=pp) == want
    finally:
        ctx.close()


def check_luts_overwritten(lib):
    """the caller's LUT arrays are free as soon as prepare returns"""
    cfg = config(lib)
    ctx = backend.Context(0, cfg, lib)
    try:
        pie, luts, lookups = lut_pie(**CASES["three_sizes_and_range_check"])
        want = ctx.prove_tables(pie, luts)
        mine = {m: (np.ascontiguousarray(a.copy(), dtype=np.uint32), np.ascontiguousarray(b.copy(), dtype=np.uint32))
                for m, (a, b) in luts.items()}
        with backend.PreparedSettings(0, cfg, mine, lookups, lib) as pp:
            for a, b in mine.values():
                a[:] = 0xdeadbeef
                b[:] = 0xffffffff
            assert ctx.prove_tables(pie, prepared=pp) == want
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- refusals
def _raw_prepare(lib, cfg, luts_c, lookups):
    """lmn_settings_prepare on hand-made lmn_lut structs -> (rc, text)"""
    arr = (backend.LmnLut * max(len(luts_c), 1))(*luts_c)
    st = backend.LmnSettings(0, len(luts_c), arr)
    h = C.c_void_p()
    rc = lib.lib.lmn_settings_prepare(0, C.byref(cfg), C.byref(st), lookups, C.byref(h))
    text = lib.lib.lmn_last_error(None).decode()
    if rc == 0:
        lib.lib.lmn_prepared_destroy(h)
    return rc, text


def _refused(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except backend.LuminairBackendError as e:
        assert e.code == INVALID, e
        assert str(e).split(" (code")[0].strip(), "refusal without a text"
        return str(e)
    raise AssertionError("accepted")


def check_prepare_refusals(lib):
    cfg = config(lib)
    col = np.arange(16, dtype=np.uint32)
    p = col.ctypes.data
    LS, LE = backend.LOOKUP_SIN, backend.LOOKUP_EXP2

    def lut(kind, log, c0=p, c1=p):
        return backend.LmnLut(kind, log, c0, c1)

    assert _raw_prepare(lib, cfg, [lut(0, 4)], LS)[0] == 0                          # the accepted form of what follows
    for what, luts_c, lookups in (("a sin bit without its LUT", [lut(1, 4)], LS | LE),
                                  ("a bit and no LUT at all", [], backend.LOOKUP_LOG2),
                                  ("a duplicate LUT", [lut(0, 4), lut(0, 4)], LS),
                                  ("a null column", [lut(0, 4, p, None)], LS),
                                  ("an unknown LUT kind", [lut(3, 4)], LS),
                                  ("log_size below 4", [lut(0, 3)], LS),
                                  ("log_size above the prover's limit", [lut(0, 29)], LS),
                                  ("unknown bits in lookups", [lut(0, 4)], LS | 16)):
        rc, text = _raw_prepare(lib, cfg, luts_c, lookups)
        assert rc == INVALID and text, (what, rc, text)
    # a non-canonical word, in either column, at the first and the last row: found on the device, named in the text
    for column in (0, 1):
        for row in (0, 15):
            bad = col.copy()
            bad[row] = (1 << 31) - 1
            cols = (bad, col) if column == 0 else (col, bad)
            text = _refused(backend.PreparedSettings, 0, cfg, {"exp2": cols}, LE, lib)
            assert "canonical" in text and "exp2_lut_%d" % column in text, text
    # no batch object, no batch: the main library, which has none, refuses every call of the batch entry it exports
    assert lib.lib.lmn_batch_prove_prepared(None, 0, None, 0, None, None, None, None) == INVALID
    ok = col.copy()
    ok[3] = (1 << 31) - 2                                                           # the largest canonical word passes
    backend.PreparedSettings(0, cfg, {"exp2": (ok, col)}, LE, lib).close()


def check_prove_refusals(lib, other_device=None, sharded=False):
    """every refusal at prove time: the code, a text, and a context that still proves"""
    cfg = config(lib)
    ctx = backend.Context(0, cfg, lib)
    try:
        pie, luts, lookups = lut_pie(**CASES["two_equal_sizes"])
        pp = backend.PreparedSettings(0, cfg, luts, lookups, lib)
        want = ctx.prove_tables(pie, prepared=pp)

        def still_proves():
            assert ctx.prove_tables(pie, prepared=pp) == want

        # the pie's lookup tables differ from `lookups`, in either direction
        more, _, _ = lut_pie(sizes={"sin": 5, "exp2": 5}, less_than=True)
        _refused(ctx.prove_tables, more, prepared=pp)
        still_proves()
        fewer, _, _ = lut_pie(sizes={"sin": 5})
        _refused(ctx.prove_tables, fewer, prepared=pp)
        still_proves()
        plain = _pie(syn.config2_graph_faithful(40, 5))
        _refused(ctx.prove_tables, plain, prepared=pp)
        with backend.PreparedSettings(0, cfg, None, 0, lib) as empty:
            _refused(ctx.prove_tables, pie, prepared=empty)
        still_proves()
        # a lookup table whose padded size is not its LUT's
        other_size, _, _ = lut_pie(sizes={"sin": 5, "exp2": 6})
        text = _refused(ctx.prove_tables, other_size, prepared=pp)
        assert "LUT" in text, text
        still_proves()
        # submit reports the same through wait
        ctx.prove_submit(fewer, prepared=pp)
        _refused(ctx.prove_wait)
        still_proves()
        # another log_blowup
        with backend.PreparedSettings(0, config(lib, 2), luts, lookups, lib) as pp2:
            text = _refused(ctx.prove_tables, pie, prepared=pp2)
            assert "log_blowup" in text, text
        still_proves()
        # a null handle, through the C entry
        arr, n, _st, _keep = ctx._marshal_tables(pie, None)
        out, out_len = C.POINTER(C.c_uint8)(), C.c_size_t()
        assert lib.lib.lmn_prove_prepared(ctx.handle, arr, n, None, C.byref(out), C.byref(out_len)) == INVALID
        assert lib.lib.lmn_last_error(ctx.handle)
        assert lib.lib.lmn_prove_submit_prepared(ctx.handle, arr, n, None) == INVALID
        still_proves()
        if other_device is not None:
            with backend.PreparedSettings(other_device, cfg, luts, lookups, lib) as far:
                text = _refused(ctx.prove_tables, pie, prepared=far)
                assert "device" in text, text
            still_proves()
        if sharded:
            # refused before any collective is called
            calls = []
            ctx.set_shard(0, 2, lambda buf, nbytes, stream: calls.append(nbytes))
            text = _refused(ctx.prove_tables, pie, prepared=pp)
            assert "sharded" in text and calls == [], (text, calls)
            ctx.clear_shard()
            still_proves()
        pp.close()
        _refused(ctx.prove_tables, pie, prepared=pp)                                # a closed Python object
        assert ctx.prove_tables(pie, luts) == want
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- batch
def _batch_counts(bp):
    c = bp.counters()
    return c["launches"], c["host_waits"], c["copy_launches"] + c["direct_copies"]


def check_batch(solo_lib, batch_so, members=(1, 2, 5)):
    """lmn_batch_prove_prepared == lmn_prove member by member, for case 2 and for a 2^6-row LUT pie; the batch counters of the
    same batch, prepared against unprepared: fewer launches, fewer host waits, fewer transfers"""
    from luminair_amd.batch import BatchProver
    cfg = config(solo_lib)
    solo = backend.Context(0, cfg, solo_lib)
    bp = BatchProver(0, max(members), protocol_variant=PINNED, library_path=batch_so)
    try:
        for shape in (CASES["three_sizes_and_range_check"], dict(sizes={"exp2": 6})):
            pies = [lut_pie(seed=30 + i, **shape) for i in range(max(members))]
            luts, lookups = pies[0][1], pies[0][2]
            want = [solo.prove_tables(p[0], luts) for p in pies]
            with bp.prepare(luts, lookups) as pp:
                assert pp.root == commitment0(want[0])
                for n in members:
                    batch = [p[0] for p in pies[:n]]
                    c0 = _batch_counts(bp)
                    assert bp.prove_batch(batch, luts) == want[:n]
                    c1 = _batch_counts(bp)
                    assert bp.prove_batch(batch, prepared=pp) == want[:n]
                    c2 = _batch_counts(bp)
                    plain = [b - a for a, b in zip(c0, c1)]
                    prep = [b - a for a, b in zip(c1, c2)]
                    print("batch of %d: launches / host waits / transfers  plain %s  prepared %s" % (n, plain, prep))
                    assert prep[0] < plain[0] and prep[1] < plain[1] and prep[2] < plain[2], (n, plain, prep)
    finally:
        bp.close()
        solo.close()


def check_batch_bad_member(solo_lib, batch_so):
    """a member with a bad trace fails alone; a prepared object of the other library is refused; the batch stays usable"""
    from luminair_amd.batch import BatchProver
    cfg = config(solo_lib)
    solo = backend.Context(0, cfg, solo_lib)
    bp = BatchProver(0, 3, protocol_variant=PINNED, library_path=batch_so)
    try:
        shape = CASES["two_equal_sizes"]
        pies = [lut_pie(seed=40 + i, **shape) for i in range(3)]
        luts, lookups = pies[0][1], pies[0][2]
        want = [solo.prove_tables(p[0], luts) for p in pies]
        pp = bp.prepare(luts, lookups)
        bad = [(k, r.copy(), n) for k, r, n in pies[1][0]]
        bad[0][1][3, 0] = (1 << 31) - 1                                             # a non-canonical word in member 1's first table
        n = 3
        arrs, keep = (C.POINTER(backend.LmnTable) * n)(), []
        for i, t in enumerate((pies[0][0], bad, pies[2][0])):
            arr, nt, _st, k = backend.Context._marshal_tables(None, t, None)
            keep.append((arr, k))
            arrs[i] = C.cast(arr, C.POINTER(backend.LmnTable))
        proofs, lens, rcs = (C.POINTER(C.c_uint8) * n)(), (C.c_size_t * n)(), (C.c_int * n)()
        rc = bp.lib.lib.lmn_batch_prove_prepared(bp.handle, n, arrs, nt, pp._handle_for(bp.lib), proofs, lens, rcs)
        assert rc == INVALID and list(rcs) == [0, INVALID, 0], (rc, list(rcs))
        assert bp.lib.lib.lmn_batch_last_error(bp.handle)
        got = [C.string_at(proofs[i], lens[i]) if proofs[i] else None for i in range(n)]
        for i in (0, 2):
            bp.lib.lib.lmn_free(proofs[i])
        assert got == [want[0], None, want[2]]
        # a null handle, and an object the other library made
        rc = bp.lib.lib.lmn_batch_prove_prepared(bp.handle, n, arrs, nt, None, proofs, lens, rcs)
        assert rc == INVALID and list(rcs) == [INVALID] * 3 and bp.lib.lib.lmn_batch_last_error(bp.handle)
        with backend.PreparedSettings(0, cfg, luts, lookups, solo_lib) as foreign:
            _refused(bp.prove_batch, [p[0] for p in pies], prepared=foreign)
            rc = bp.lib.lib.lmn_batch_prove_prepared(bp.handle, n, arrs, nt, foreign.handle, proofs, lens, rcs)
            assert rc == INVALID, rc
        # a batch whose log_blowup is not the object's: every member refuses, the batch stays usable
        with backend.PreparedSettings(0, config(bp.lib, 2), luts, lookups, bp.lib) as pp2:
            _refused(bp.prove_batch, [p[0] for p in pies], prepared=pp2)
        assert bp.prove_batch([p[0] for p in pies], prepared=pp) == want
        pp.close()
        assert bp.prove_batch([p[0] for p in pies], luts) == want
    finally:
        bp.close()
        solo.close()


# ---------------------------------------------------------------------------------------------- Python layer
def check_python_layer(solo_lib, batch_so):
    """Prover.prove / ProverPool.prove_many / BatchPool.prove_many with prepared= return the bytes they return without"""
    from luminair_amd.batch import BatchPool
    from luminair_amd.pie import CircuitSettings, RangeCheckLookup
    from luminair_amd.prover import Prover, ProverPool
    shape = CASES["three_sizes_and_range_check"]
    raw = [lut_pie(seed=50 + i, **shape) for i in range(4)]
    luts, lookups = raw[0][1], raw[0][2]
    pies = [LuminairPie.from_tables([(k, r) for k, r, _ in p[0]]) for p in raw]
    settings = CircuitSettings(lookups=dict(luts), range_check=RangeCheckLookup([8], 8, [0] * 256))
    prover = Prover(0, PINNED, solo_lib)
    pool = ProverPool(0, 2, PINNED, solo_lib)
    bpool = BatchPool(0, groups=2, slots=2, protocol_variant=PINNED, library_path=batch_so)
    try:
        want = [prover.prove(p, settings).to_bincode() for p in pies]
        with settings.prepare(0, prover.ctx.config, solo_lib) as pp:
            assert pp.lookups == lookups
            assert [prover.prove(p, prepared=pp).to_bincode() for p in pies] == want
            assert [x.to_bincode() for x in pool.prove_many(pies, prepared=pp)] == want
            assert [x.to_bincode() for x in pool.prove_many(pies, settings)] == want
        tables = [p[0] for p in raw]
        with bpool.prepare(luts, lookups) as bpp:
            assert bpool.prove_many(tables, prepared=bpp) == want
        assert bpool.prove_many(tables, luts) == want
    finally:
        prover.ctx.close()
        pool.close()
        bpool.close()
