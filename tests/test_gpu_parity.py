"""Parity tests proper: the HIP library on a real MI355X, called through the C ABI, against the
oracle (bit-exact: all arithmetic is integer / byte work) and the reference's known-answer proof."""
import numpy as np
import pytest

import luminair_amd
from luminair_amd import backend, synthetic as syn

pytestmark = pytest.mark.gpu


def _oracle_bytes(tabs):
    from oracle.proof import to_bincode
    from oracle.prover import prove
    return to_bincode(prove([(k, r.astype(np.uint64)) for k, r in tabs]))


def _gpu_bytes(prover, tabs):
    return prover.prove(luminair_amd.LuminairPie.from_tables(tabs)).to_bincode()


def test_gpu_reproduces_reference_kat(gpu_prover, kat_bytes):
    """BASELINE config 1: examples/simple, byte-identical to ui/demo/public/proof."""
    assert _gpu_bytes(gpu_prover, syn.simple_example()) == kat_bytes


@pytest.mark.parametrize("name,tabs", [
    ("single-row", syn.chain_graph(1, 6)),
    ("add-ragged-100", syn.config2_add_only(100, 1)),
    ("add-2^8", syn.config2_add_only(256, 2)),
    ("chain-300", syn.chain_graph(300, 3)),
    ("mixed-sizes", [(0, syn.chain_graph(64, 4)[0][1]), (1, syn.chain_graph(500, 5)[1][1])]),
    ("add-2^12", syn.config2_add_only(1 << 12, 6)),
    ("chain-2^13", syn.chain_graph(1 << 13, 7)),
    ("config3-small", syn.config3_mixed(14, 13, 13, 8)),
    ("add-2^16", syn.config2_add_only(1 << 16, 42)),
    ("mul-only-ragged", [syn.chain_graph(1000, 9)[1]]),
    ("recip-only", [syn.chain_graph(257, 10)[2]]),
    ("pow2-plus-one", syn.config2_add_only((1 << 10) + 1, 11)),
    ("pow2-minus-one", syn.config2_add_only((1 << 11) - 1, 12)),
    ("linear-layer", syn.linear_layer(64, 100, 13)),
    ("linear-layer+max", syn.linear_layer(33, 50, 14, True)),
])
def test_gpu_proof_equals_oracle_proof(gpu_prover, name, tabs):
    got = _gpu_bytes(gpu_prover, tabs)
    want = _oracle_bytes(tabs)
    if got != want:
        first = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
        pytest.fail("%s: proofs differ (len %d vs %d), first difference at byte %d" % (name, len(got), len(want), first))


@pytest.fixture(scope="module")
def c_oracle():
    from oracle.cbackend import CKernels
    return CKernels()


def test_gpu_full_size_2_20_equals_c_oracle_bytes(gpu_prover, c_oracle):
    """BASELINE config 2 at FULL size, byte-for-byte: GPU proof == proof of the plain-C restatement
    (itself pinned on the KAT and cross-checked against the numpy restatement)."""
    from oracle.proof import to_bincode
    from oracle.prover import prove
    tabs = syn.config2_add_only(1 << 20, 42)
    want = to_bincode(prove(tabs, kernels=c_oracle))
    got = _gpu_bytes(gpu_prover, tabs)
    assert got == want


@pytest.mark.gpu
@pytest.mark.parametrize("cols", ["8", "4"])
def test_gpu_transpose_inside_the_interpolation_switch(gpu_prover, c_oracle, cols, monkeypatch):
    """LMN_ROWS_FUSION=1 (off by default, docs/HISTORY.md round 6): k_fft_rows_fx instead of k_transpose_pad + the plain first
    inverse pass, logup fractions from the table's rows: config 2a at full size and a ragged mixed pie, byte-for-byte."""
    from oracle.proof import to_bincode
    from oracle.prover import prove
    monkeypatch.setenv("LMN_ROWS_FUSION", "1")
    monkeypatch.setenv("LMN_ROWS_FX_COLS", cols)
    for tabs in (syn.config2_add_only(1 << 20, 42), syn.config3_mixed(19, 18, 18, 8),
                 [(0, syn.chain_graph(300000, 4)[0][1]), (1, syn.chain_graph(70000, 5)[1][1])]):
        assert _gpu_bytes(gpu_prover, tabs) == to_bincode(prove(tabs, kernels=c_oracle))


def test_gpu_config3_mixed_2_20_total_rows_equals_c_oracle_bytes(gpu_prover, c_oracle):
    """Add 2^19 + Mul 2^18 + Recip 2^18 rows (config 3's shape at 1/4 scale), byte-for-byte."""
    from oracle.proof import to_bincode
    from oracle.prover import prove
    tabs = syn.config3_mixed(19, 18, 18, 8)
    assert _gpu_bytes(gpu_prover, tabs) == to_bincode(prove(tabs, kernels=c_oracle))


def test_gpu_linear_layer_2_19_rows_equals_c_oracle_bytes(gpu_prover, c_oracle):
    """BASELINE config 5's building block (Mul + SumReduce + Add) at 2 x 2^18 + 2^9 rows, byte-for-byte."""
    from oracle.proof import to_bincode
    from oracle.prover import prove
    tabs = syn.linear_layer(512, 512, 21)
    assert _gpu_bytes(gpu_prover, tabs) == to_bincode(prove(tabs, kernels=c_oracle))


def _sha(b):
    import hashlib
    return hashlib.sha256(b).hexdigest()


def test_gpu_config3_full_size_2_22_rows_equals_c_oracle_bytes(gpu_prover, c_oracle):
    """BASELINE config 3 at FULL size (Add 2^21 + Mul 2^20 + Recip 2^20 rows, three components in every
    commitment, mixed-size trees): the GPU proof and the C oracle's proof have the same SHA-256."""
    from oracle.proof import to_bincode
    from oracle.prover import prove
    tabs = syn.config3_mixed(21, 20, 20, 5)
    want = to_bincode(prove(tabs, kernels=c_oracle))
    got = _gpu_bytes(gpu_prover, tabs)
    assert len(got) == len(want) and _sha(got) == _sha(want)


def test_gpu_config2b_full_size_equals_c_oracle_bytes(gpu_prover_pinned, c_oracle):
    """BASELINE config 2b at FULL size (what gen_trace emits for one Add node at HEAD: Add 2^20 rows consumed with
    multiplicity -1 + the Inputs table of 2^21 rows; PINNED variant), byte-for-byte against the C oracle."""
    from oracle.channel import ProtocolVariant
    from oracle.proof import to_bincode
    from oracle.prover import prove
    tabs = syn.config2_graph_faithful(1 << 20, 42)
    want = to_bincode(prove(tabs, kernels=c_oracle, variant=ProtocolVariant.PINNED))
    got = _gpu_bytes(gpu_prover_pinned, tabs)
    assert len(got) == len(want) and _sha(got) == _sha(want)


def test_gpu_config5_full_size_2_24_rows_equals_c_oracle_bytes(gpu_prover, c_oracle):
    """BASELINE config 5 at FULL size (256 x (Mul + SumReduce + Add): Mul 2^23 + SumReduce 2^23 + Add 2^15 rows,
    composition LDE of 2^25 rows): SHA-256 of the GPU proof == SHA-256 of the C oracle's proof.  The oracle run is
    the long part (tens of seconds on the GPU box's host cores, ~25 GB of host memory)."""
    from oracle.proof import to_bincode
    from oracle.prover import prove
    tabs = syn.config5_linear_layers()
    got = _gpu_bytes(gpu_prover, tabs)
    want = to_bincode(prove(tabs, kernels=c_oracle))
    assert len(got) == len(want) and _sha(got) == _sha(want)


def test_gpu_device_resident_rows_give_same_proof(gpu_prover):
    tabs = syn.chain_graph(3000, 11)
    want = _gpu_bytes(gpu_prover, tabs)
    ctx = gpu_prover.ctx
    bufs = [ctx.upload(r) for _, r in tabs]
    got = ctx.prove_tables([(k, b, len(r)) for (k, r), b in zip(tabs, bufs)])
    for b in bufs:
        b.free()
    assert got == want


def test_gpu_full_size_add_2_20_verifies_and_is_deterministic(gpu_prover):
    """BASELINE config 2 at full size: size-independent properties — the proof verifies under the
    oracle's verifier (every Merkle path, the OODS identity, every FRI fold), is deterministic, and
    its main-trace root changes when one trace cell changes."""
    from oracle.proof import from_bincode
    from oracle.verifier import verify
    tabs = syn.config2_add_only(1 << 20, 42)
    a = _gpu_bytes(gpu_prover, tabs)
    b = _gpu_bytes(gpu_prover, tabs)
    assert a == b
    p = from_bincode(a, 8)
    assert p.claim[0] == 20
    verify(p)
    rows = tabs[0][1].copy()
    rows[12345, 9] = (int(rows[12345, 9]) + 1) % syn.P
    rows[12345, 11] = (int(rows[12345, 11]) + 1) % syn.P   # keep out = lhs + rhs
    c = from_bincode(_gpu_bytes(gpu_prover, [(0, rows)]), 8)
    verify(c)
    assert c.proof.commitments[1] != p.proof.commitments[1]


def test_gpu_config3_mixed_2_22_rows_verifies(gpu_prover):
    """BASELINE config 3: Add 2^21 + Mul 2^20 + Recip 2^20 rows, three components in one commitment."""
    from oracle.proof import from_bincode
    from oracle.verifier import verify
    p = from_bincode(_gpu_bytes(gpu_prover, syn.config3_mixed(21, 20, 20, 5)), 8)
    assert p.claim[:3] == [21, 20, 20]
    verify(p)


def test_gpu_largest_single_table_2_22_rows_verifies(gpu_prover):
    """Maximum size exercised: one Add table of 2^22 rows (LDE 2^23, composition LDE 2^24)."""
    from oracle.proof import from_bincode
    from oracle.verifier import verify
    p = from_bincode(_gpu_bytes(gpu_prover, syn.config2_add_only(1 << 22, 3)), 8)
    assert p.claim[0] == 22
    verify(p)


def test_gpu_two_contexts_concurrently(hip_lib_path):
    """Independent contexts (own stream + arena) proving at the same time give the same bytes."""
    from concurrent.futures import ThreadPoolExecutor
    provers = [luminair_amd.Prover(0) for _ in range(3)]
    tabs = [syn.chain_graph(1 << 12, 20 + i) for i in range(3)]
    want = [_gpu_bytes(provers[0], t) for t in tabs]
    with ThreadPoolExecutor(3) as ex:
        for _ in range(3):
            got = list(ex.map(lambda it: _gpu_bytes(it[0], it[1]), zip(provers, tabs)))
            assert got == want


def test_gpu_four_contexts_full_size_soak(hip_lib_path):
    """The bench's operating point: four contexts proving the 2^20-row trace concurrently from device-resident rows;
    every one of 4 x 40 proofs has the same bytes (wave-cooperative hashing, device channel and arenas do not
    interfere across contexts)."""
    import hashlib
    import threading
    tabs = syn.config2_add_only(1 << 20, 42)
    provers = [luminair_amd.Prover(0) for _ in range(4)]
    bufs = [[(k, p.ctx.upload(r), len(r)) for k, r in tabs] for p in provers]
    ref = hashlib.sha256(provers[0].ctx.prove_tables(bufs[0])).hexdigest()
    bad = []

    def work(i):
        for it in range(40):
            if hashlib.sha256(provers[i].ctx.prove_tables(bufs[i])).hexdigest() != ref:
                bad.append((i, it))

    ths = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert not bad
    for bl in bufs:
        for _, b, _ in bl:
            b.free()


def test_gpu_four_contexts_host_rows_shared_and_private_buffers(hip_lib_path):
    """The reference's calling convention (prover.rs:28-31,70: the pie is HOST data) at the bench's operating point:
    four contexts, one driver thread each, 40 proofs each of the 2^20-row trace handed over as host buffers - first
    all four contexts reading the SAME numpy buffer, then private copies, the first host-rows proof of every context
    growing its arena inside the concurrent region.  Every proof must equal the device-rows proof (BENCH_r02's
    `host_rows` ConstraintsNotSatisfied: tools/repro_host_rows.py)."""
    import hashlib
    import threading
    tabs = syn.config2_add_only(1 << 20, 42)
    provers = [luminair_amd.Prover(0) for _ in range(4)]
    dev = [(k, provers[0].ctx.upload(r), len(r)) for k, r in tabs]
    ref = hashlib.sha256(provers[0].ctx.prove_tables(dev)).hexdigest()
    for label, bufs in (("shared", [[(k, r, len(r)) for k, r in tabs] for _ in provers]),
                        ("private", [[(k, np.array(r, copy=True), len(r)) for k, r in tabs] for _ in provers])):
        bad = []

        def work(i):
            for it in range(40):
                try:
                    if hashlib.sha256(provers[i].ctx.prove_tables(bufs[i])).hexdigest() != ref:
                        bad.append((label, i, it, "bytes differ"))
                except Exception as e:  # noqa: BLE001
                    bad.append((label, i, it, str(e)))

        ths = [threading.Thread(target=work, args=(i,)) for i in range(4)]
        [t.start() for t in ths]
        [t.join() for t in ths]
        assert not bad, bad[:4]
    for _, b, _ in dev:
        b.free()


def test_gpu_host_rows_in_page_locked_memory(hip_lib_path):
    """`lmn_host_alloc` / `lmn_host_register`: trace rows in page-locked host memory (direct DMA, the upload call returns
    at once) give the same proof as device-resident rows - four contexts, one thread each, 12 proofs each, two of them
    reading ONE shared allocated buffer and two reading private arrays that were page-locked in place."""
    import hashlib
    import threading
    tabs = syn.config2_add_only(1 << 20, 42)
    provers = [luminair_amd.Prover(0) for _ in range(4)]
    lib = provers[0].ctx.lib
    dev = [(k, provers[0].ctx.upload(r), len(r)) for k, r in tabs]
    ref = hashlib.sha256(provers[0].ctx.prove_tables(dev)).hexdigest()
    pinned = []
    for k, r in tabs:
        a = lib.host_rows(r.shape, r.dtype)
        a.array[...] = r
        pinned.append(a)
    shared = [(k, a.array, len(a.array)) for (k, _), a in zip(tabs, pinned)]
    private = []
    for _ in range(2):
        arrs = [np.array(r, copy=True) for _, r in tabs]
        for x in arrs:
            lib.host_register(x)
        private.append(arrs)
    bufs = [shared, shared] + [[(k, x, len(x)) for (k, _), x in zip(tabs, arrs)] for arrs in private]
    bad = []

    def work(i):
        for it in range(12):
            try:
                if hashlib.sha256(provers[i].ctx.prove_tables(bufs[i])).hexdigest() != ref:
                    bad.append((i, it, "bytes differ"))
            except Exception as e:  # noqa: BLE001
                bad.append((i, it, str(e)))

    ths = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    for arrs in private:
        for x in arrs:
            lib.host_unregister(x)
    for a in pinned:
        a.free()
    for _, b, _ in dev:
        b.free()
    assert not bad, bad[:4]


def test_gpu_one_context_driven_by_several_threads_is_serialised(hip_lib_path):
    """Misuse made safe: calls on ONE context from several threads are serialised by the context's lock
    (include/luminair_hip.h) - round 2's bench put two pool workers into one context and got corrupted proofs and
    GPU memory faults.  Three threads x 8 proofs on one context, host rows and device rows mixed."""
    import threading
    tabs = syn.config2_add_only(1 << 16, 5)
    p = luminair_amd.Prover(0)
    dev = [(k, p.ctx.upload(r), len(r)) for k, r in tabs]
    host = [(k, r, len(r)) for k, r in tabs]
    want = p.ctx.prove_tables(dev)
    bad = []

    def work(i):
        for it in range(8):
            if p.ctx.prove_tables(dev if (i + it) & 1 else host) != want:
                bad.append((i, it))

    ths = [threading.Thread(target=work, args=(i,)) for i in range(3)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert not bad
    for _, b, _ in dev:
        b.free()


def test_gpu_error_behaviour(gpu_prover):
    with pytest.raises(luminair_amd.LuminairError) as e:
        gpu_prover.prove(luminair_amd.LuminairPie([luminair_amd.TraceTable(luminair_amd.TraceTableKind.Add,
                                                                            np.zeros((0, 15), np.uint32))]))
    assert e.value.variant == "TraceError(EmptyTrace)"
    bad = syn.config2_add_only(64, 9)[0][1].copy()
    bad[3, 11] ^= 1
    with pytest.raises(luminair_amd.LuminairError) as e:
        gpu_prover.prove(luminair_amd.LuminairPie.from_tables([(0, bad)]))
    assert e.value.variant == "ProverError(ConstraintsNotSatisfied)"
    bad = syn.config2_add_only(1 << 12, 9)[0][1].copy()
    bad[77, 10] = 0x7fffffff                                  # P itself is not a canonical M31 word
    with pytest.raises(luminair_amd.LuminairError):
        gpu_prover.prove(luminair_amd.LuminairPie.from_tables([(0, bad)]))
    # the context stays usable after an error
    assert len(_gpu_bytes(gpu_prover, syn.config2_add_only(64, 9))) > 1000


def test_gpu_level2_ops_match_oracle(gpu_prover):
    from oracle import fft
    from oracle.field import P, QM31
    from oracle.merkle import MerkleTree
    ctx = gpu_prover.ctx
    rng = np.random.default_rng(5)
    for log in (5, 12, 13, 17):
        ev = rng.integers(0, P, size=(3, 1 << log), dtype=np.uint64)
        co = ctx.interpolate(ev.astype(np.uint32))
        assert np.array_equal(co, fft.interpolate(ev).astype(np.uint32)), "interpolate log %d" % log
        lde = ctx.evaluate(co, log + 1)
        assert np.array_equal(lde, fft.evaluate(co.astype(np.uint64), log + 1).astype(np.uint32)), "evaluate %d" % log
    cols = [rng.integers(0, P, size=1 << k, dtype=np.uint64).astype(np.uint32) for k in (12, 12, 10, 12, 3)]
    assert ctx.merkle_root(cols) == MerkleTree(cols).root()
    cols = [rng.integers(0, P, size=1 << 14, dtype=np.uint64).astype(np.uint32) for _ in range(19)]
    assert ctx.merkle_root(cols) == MerkleTree(cols).root()
    assert ctx.merkle_root([]) == MerkleTree([]).root()
    pt = [int(v) for v in rng.integers(0, P, size=8)]
    for log in (4, 10, 16):
        c = rng.integers(0, P, size=1 << log, dtype=np.uint64)
        want = fft.eval_at_point(c, (QM31(*pt[:4]), QM31(*pt[4:])))
        assert ctx.eval_at_point(c.astype(np.uint32), pt) == want.v
    from level2_checks import check_evaluate_block, check_quotient_fold_grind_ops
    for log in (6, 13):
        check_quotient_fold_grind_ops(ctx, log)
    check_evaluate_block(ctx, logs=((5, 6), (12, 13), (15, 16), (19, 20), (20, 21)))


def test_gpu_device_handle_ops_match_oracle(gpu_prover):
    """Level 2 on device handles (lmn_col_* / lmn_tree_*): every op vs the oracle, plus the chained
    interpolate -> evaluate -> commit -> quotients -> folds pipeline with one upload and one download."""
    from level2_checks import check_device_handle_ops
    check_device_handle_ops(gpu_prover.ctx, 7)
    check_device_handle_ops(gpu_prover.ctx, 13)     # multi-pass FFT, fused Merkle kernel sizes


@pytest.mark.parametrize("seed,scale", [(0, 1), (1, 1), (2, 40), (3, 40), (4, 150), (5, 150)])
def test_gpu_random_pies_equal_c_oracle(gpu_prover_pinned, c_oracle, seed, scale):
    """Random component mixes with ragged sizes (up to ~10^5 rows): mixed-size Merkle trees, several
    composition sizes, tree-0 layouts; byte-for-byte against the C oracle."""
    from level2_checks import random_pie
    from oracle.channel import ProtocolVariant
    from oracle.proof import to_bincode
    from oracle.prover import prove
    tabs, luts = random_pie(seed, scale)
    got = gpu_prover_pinned.prove(luminair_amd.LuminairPie.from_tables(tabs), luminair_amd.CircuitSettings(luts))
    assert got.to_bincode() == to_bincode(prove(tabs, variant=ProtocolVariant.PINNED, kernels=c_oracle, luts=luts))


def test_gpu_device_trace_generation(gpu_prover):
    """§8f-3: Add / Mul / Recip `process_trace` on device tensors feeding lmn_prove without a host round trip."""
    from level2_checks import check_device_trace_generation
    for n in (1, 1000, (1 << 18) + 5):
        check_device_trace_generation(gpu_prover.ctx, n)
    from level2_checks import check_device_linear_layer
    check_device_linear_layer(gpu_prover.ctx)
    check_device_linear_layer(gpu_prover.ctx, n_out=300, dim=129, seed=5)


def test_gpu_device_graph_gen_trace_then_prove(hip_lib_path):
    """gen_trace on the device (DeviceGraph over lmn_trace_*) -> lmn_prove on device-resident tables -> lmn_verify."""
    from level2_checks import check_device_graph, check_device_remaining_ops
    from luminair_amd import backend
    check_device_graph(backend.Library(hip_lib_path))
    check_device_remaining_ops(backend.Library(hip_lib_path))


def test_gpu_config4_mlp_generated_and_proved_on_device(hip_lib_path):
    """BASELINE config 4 end to end on the GPU: the 2 -> 64 -> 64 -> 1 tanh MLP is executed by DeviceGraph
    (expanded views, constants, Exp2 LUT with its multiplicities), its device-resident tables are proved and the
    proof passes the verifier; the forward pass equals the numpy fixed-point reference."""
    from level2_checks import device_mlp
    from luminair_amd import backend
    lib = backend.Library(hip_lib_path)
    cfg = lib.default_config()
    cfg.protocol_variant = backend.VARIANT_PINNED
    ctx = backend.Context(0, cfg, lib)
    g, out, ref = device_mlp(ctx)
    tables, luts, bufs = g.gen_trace()
    assert np.array_equal(g.read(out), ref)
    assert [k for k, _, _ in tables] == [0, 1, 2, 5, 9, 10, 15]
    assert dict((k, n) for k, _, n in tables)[1] == 2 * 64 + 64 * 64 + 64 + 4 * 64      # Mul rows
    proof = ctx.prove_tables(tables, luts)
    lib.verify(proof, backend.VARIANT_PINNED)
    for b in bufs:
        b.free()
    ctx.close()


@pytest.mark.parametrize("log", [12, 13, 20, 22, 23, 24, 25])
def test_gpu_fft_tiled_equals_layerwise(gpu_prover, log):
    """Device-side differential check at full sizes: LDS-tiled passes vs one-layer-per-launch."""
    gpu_prover.ctx.fft_selftest(log, 2)


# ---- LuminAIR-HEAD claim layout (17 slots) + Inputs component: BASELINE config 2b "graph-faithful"
@pytest.fixture(scope="module")
def gpu_prover_pinned(hip_lib_path):
    from luminair_amd import backend
    return luminair_amd.Prover(0, protocol_variant=backend.VARIANT_PINNED)


def _oracle_bytes_pinned(tabs):
    from oracle.channel import ProtocolVariant
    from oracle.proof import to_bincode
    from oracle.prover import prove
    return to_bincode(prove([(k, r.astype(np.uint64)) for k, r in tabs], variant=ProtocolVariant.PINNED))


@pytest.mark.parametrize("name,tabs", [
    ("2b-100", syn.config2_graph_faithful(100, 3)),
    ("2b-2^12", syn.config2_graph_faithful(1 << 12, 4)),
    ("add-only-pinned", syn.config2_add_only(300, 5)),
    ("less-than+range-check-lut", syn.less_than_graph(1000, 6)),
    ("sqrt+rem", syn.sqrt_rem_graph(3000, 7)),
])
def test_gpu_pinned_variant_equals_oracle(gpu_prover_pinned, name, tabs):
    got = _gpu_bytes(gpu_prover_pinned, tabs)
    assert got == _oracle_bytes_pinned(tabs), name


def test_gpu_config2b_full_size_verifies(gpu_prover_pinned):
    """Add 2^20 rows (mult -1/-1/0) + Inputs 2^21 rows: mixed-size Merkle trees, logup sums cancel."""
    from oracle.channel import ProtocolVariant
    from oracle.proof import from_bincode
    from oracle.verifier import verify
    p = from_bincode(_gpu_bytes(gpu_prover_pinned, syn.config2_graph_faithful(1 << 20, 42)), 17)
    assert p.claim[0] == 20 and p.claim[15] == 21
    verify(p, ProtocolVariant.PINNED)


@pytest.mark.parametrize("name,kat_tabs,pinned_tabs", [
    # trees of 2^18 / 2^19 leaves: one / two register levels per lane are left out of the stored tree; the first FRI tree's
    # leaf level (2^19) is hashed by the launch of the level above it (the threshold of MerkleFold::below)
    ("add-2^17", syn.config2_add_only(1 << 17, 21), None),
    # two component sizes: a level with children AND columns is the start level of a launch that skips its register levels
    ("add-2^18 + mul-2^17", [(0, syn.chain_graph(1 << 18, 22)[0][1]), (1, syn.chain_graph(1 << 17, 23)[1][1])], None),
    # Inputs 2^19 rows over Add 2^18 rows: trace tree with a 7-column leaf level under a 15-column level, interaction tree
    # with a 4-column leaf level under an 8-column level - both fused into the upper level's launch
    ("2b: add-2^18 + inputs-2^19", None, syn.config2_graph_faithful(1 << 18, 24)),
])
def test_gpu_tree_storage_thresholds_equal_c_oracle_bytes(gpu_prover, gpu_prover_pinned, c_oracle, name, kat_tabs, pinned_tabs):
    """Sizes at which the Merkle storage form changes (MerkleCut depth 1 / 2 / 3, the fused leaf level): proof bytes
    against the C oracle - the decommitment of such a proof recomputes the tree nodes that were never written."""
    from oracle.channel import ProtocolVariant
    from oracle.proof import to_bincode
    from oracle.prover import prove
    if kat_tabs is not None:
        want = to_bincode(prove(kat_tabs, kernels=c_oracle))
        got = _gpu_bytes(gpu_prover, kat_tabs)
    else:
        want = to_bincode(prove(pinned_tabs, variant=ProtocolVariant.PINNED, kernels=c_oracle))
        got = _gpu_bytes(gpu_prover_pinned, pinned_tabs)
    assert len(got) == len(want) and _sha(got) == _sha(want), name


_TWIDDLE_LIFETIME_SCRIPT = r"""
import hashlib, sys
sys.path.insert(0, sys.argv[1])
import luminair_amd
from luminair_amd import synthetic as syn
sha = lambda p, t: hashlib.sha256(p.prove(luminair_amd.LuminairPie.from_tables(t)).to_bincode()).hexdigest()
small, big = syn.config2_add_only(1 << 10, 31), syn.config2_add_only(1 << 15, 32)
a = luminair_amd.Prover(0)
want_small = sha(a, small)                 # a builds the process's first set: enough for 2^10 rows
b = luminair_amd.Prover(0)
want_big = sha(b, big)                     # b needs a larger one and builds it
assert sha(a, small) == want_small         # a still works on the set it holds
assert sha(a, big) == want_big             # ... and moves to the larger set
b.ctx.close()                              # the builder of the larger set goes away
assert sha(a, big) == want_big and sha(a, small) == want_small
c = luminair_amd.Prover(0)
assert sha(c, big) == want_big
a.ctx.close()
assert sha(c, small) == want_small
c.ctx.close()
d = luminair_amd.Prover(0)                 # every holder is gone: the registry's weak reference has expired, d builds anew
assert sha(d, small) == want_small and sha(d, big) == want_big
print(want_small, want_big)
"""


def test_gpu_twiddle_sets_are_shared_and_outlive_their_builder(gpu_prover, root):
    """The twiddle tables are one set per device, shared by the contexts of the process and replaced by a larger set when a
    context needs one (context.cpp `ensure_twiddles`).  In a fresh process: a context keeps proving with the set it holds
    after the context that built it is gone, moves to a larger set built by someone else, a set is rebuilt after all of its
    holders are gone - and every context yields the bytes this process's prover gives for the same tables."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", _TWIDDLE_LIFETIME_SCRIPT, root], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got_small, got_big = r.stdout.split()[-2:]
    assert got_small == _sha(_gpu_bytes(gpu_prover, syn.config2_add_only(1 << 10, 31)))
    assert got_big == _sha(_gpu_bytes(gpu_prover, syn.config2_add_only(1 << 15, 32)))


def test_gpu_storage_and_fusion_switches_do_not_change_the_proof(gpu_prover, monkeypatch):
    """The forms this round replaced stay selectable for measurements (LMN_MERKLE_FULL: every tree level written;
    LMN_MERKLE_BELOW_MIN_LOG=99: separate leaf launch under a column level; LMN_NO_JOIN_FUSION: a joining quotient column
    folded by its own launches): each yields the bytes of the default form (which the other tests pin on the oracle)."""
    tabs = syn.config2_add_only(1 << 20, 42)
    want = _sha(_gpu_bytes(gpu_prover, tabs))
    for env in ({"LMN_MERKLE_FULL": "1"}, {"LMN_MERKLE_BELOW_MIN_LOG": "99"}, {"LMN_NO_JOIN_FUSION": "1"},
                {"LMN_NO_FOLD_FUSION": "1"},   # every FRI fold a launch of its own
                {"LMN_HOST_FS": "1"},    # round 5: the transcript of the commitment phases back on the host
                {"LMN_HOST_QUOT": "1"},  # round 6: the step in front of the quotient kernels back on the host (3 waits)
                {"LMN_CHAN_STEP_SEPARATE": "1"}):   # ... or on the device in launches of their own
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        assert _sha(_gpu_bytes(gpu_prover, tabs)) == want, env
        for k in env:
            monkeypatch.delenv(k)


def test_gpu_less_than_2_18_rows_equals_c_oracle_bytes(gpu_prover_pinned, c_oracle):
    """Add + LessThan (7 logup relations, range-check LUT in tree 0) + Inputs at 2^18 rows, byte-for-byte."""
    from oracle.channel import ProtocolVariant
    from oracle.proof import to_bincode
    from oracle.prover import prove
    tabs = syn.less_than_graph(1 << 18, 9)
    want = to_bincode(prove(tabs, variant=ProtocolVariant.PINNED, kernels=c_oracle))
    assert _gpu_bytes(gpu_prover_pinned, tabs) == want


@pytest.mark.parametrize("n", [50, 3000])
def test_gpu_lut_activations_equal_oracle(gpu_prover_pinned, n):
    """Sin / Exp2 / Log2 + SinLookup / Exp2Lookup / Log2Lookup: LUT columns handed over as settings data,
    two-column LUTs of three different sizes in tree 0, width-2 LUT relations."""
    from oracle.channel import ProtocolVariant
    from oracle.proof import to_bincode
    from oracle.prover import prove
    tabs, luts = syn.activation_graph(n, 11)
    got = gpu_prover_pinned.prove(luminair_amd.LuminairPie.from_tables(tabs), luminair_amd.CircuitSettings(luts))
    assert got.to_bincode() == to_bincode(prove(tabs, variant=ProtocolVariant.PINNED, luts=luts))
    from luminair_amd import backend
    luminair_amd.verify(got, protocol_variant=backend.VARIANT_PINNED)


def test_gpu_lut_activations_2_18_rows_equal_c_oracle_bytes(gpu_prover_pinned, c_oracle):
    from oracle.channel import ProtocolVariant
    from oracle.proof import to_bincode
    from oracle.prover import prove
    tabs, luts = syn.activation_graph(1 << 18, 12)
    got = gpu_prover_pinned.prove(luminair_amd.LuminairPie.from_tables(tabs), luminair_amd.CircuitSettings(luts))
    assert got.to_bincode() == to_bincode(prove(tabs, variant=ProtocolVariant.PINNED, kernels=c_oracle, luts=luts))


def test_gpu_config4_black_scholes_shape_equals_c_oracle_bytes(gpu_prover_pinned, c_oracle):
    """BASELINE config 4: 2 -> 64 -> 64 -> 1 tanh MLP shape; Add, Mul, Recip, SumReduce, Exp2, Exp2Lookup tables
    (all <= 2^13 rows except the 2^17-row LUT), byte-for-byte and through the product verifier."""
    from oracle.channel import ProtocolVariant
    from oracle.proof import to_bincode
    from oracle.prover import prove
    from luminair_amd import backend
    tabs, luts = syn.config4_black_scholes_shape(batch=1, seed=42)
    got = gpu_prover_pinned.prove(luminair_amd.LuminairPie.from_tables(tabs), luminair_amd.CircuitSettings(luts))
    assert got.to_bincode() == to_bincode(prove(tabs, variant=ProtocolVariant.PINNED, kernels=c_oracle, luts=luts))
    luminair_amd.verify(got, protocol_variant=backend.VARIANT_PINNED)


def test_gpu_config5_small_equals_oracle(gpu_prover):
    tabs = syn.config5_linear_layers(n_layers=5, n_out=6, dim=11, seed=3)
    assert _gpu_bytes(gpu_prover, tabs) == _oracle_bytes(tabs)


def test_gpu_config5_2_24_rows_verifies(gpu_prover):
    """BASELINE config 5 at full size: 256 x (Mul + SumReduce + Add), Mul 2^23 + SumReduce 2^23 + Add 2^15 rows.
    Too large for the oracle prover; checked through size-independent properties: the oracle verifier and the
    product verifier accept the proof (logup sums cancel, OODS identity, FRI, Merkle paths) and proving is
    deterministic."""
    from oracle.proof import from_bincode
    from oracle.verifier import verify
    tabs = syn.config5_linear_layers()
    assert sum(len(r) for _, r in tabs) == (1 << 24) + (1 << 15)
    pie = luminair_amd.LuminairPie.from_tables(tabs)
    a = gpu_prover.prove(pie)
    p = from_bincode(a.to_bincode(), 8)
    assert (p.claim[0], p.claim[1], p.claim[5]) == (15, 23, 23)
    verify(p)
    luminair_amd.verify(a)
    assert gpu_prover.prove(pie).to_bincode() == a.to_bincode()


def test_gpu_kat_era_sin_equals_oracle(gpu_prover):
    """The KAT-era transcript drew one LUT relation (sin): Sin + SinLookup in the 8-slot claim."""
    from oracle.proof import to_bincode
    from oracle.prover import prove
    tabs, luts = syn.activation_graph(500, 13, names=("sin",))
    tabs = [t for t in tabs if t[0] != 15]
    got = gpu_prover.prove(luminair_amd.LuminairPie.from_tables(tabs), luminair_amd.CircuitSettings(luts))
    assert got.to_bincode() == to_bincode(prove(tabs, luts=luts))


def test_gpu_proofs_pass_the_product_verifier(gpu_prover, gpu_prover_pinned, kat_bytes):
    """prove -> verify round trip through the C ABI only (the reference's own test strategy,
    crates/graph/src/tests/mod.rs:26-44), plus rejection of a tampered proof."""
    luminair_amd.verify(luminair_amd.LuminairProof(kat_bytes))
    proof = gpu_prover.prove(luminair_amd.LuminairPie.from_tables(syn.linear_layer(64, 100, 13)))
    luminair_amd.verify(proof)
    from luminair_amd import backend
    p2 = gpu_prover_pinned.prove(luminair_amd.LuminairPie.from_tables(syn.less_than_graph(1000, 6)))
    luminair_amd.verify(p2, protocol_variant=backend.VARIANT_PINNED)
    bad = bytearray(proof.to_bincode())
    bad[len(bad) // 2] ^= 1
    with pytest.raises(luminair_amd.LuminairError):
        luminair_amd.verify(luminair_amd.LuminairProof(bytes(bad)))


def test_gpu_level2_surface_alone_reproduces_proofs(hip_lib_path, kat_bytes):
    """VERDICT r2 missing #2: `lmn_col_*` / `lmn_tree_*` (incl. lmn_col_logup / lmn_col_composition) driven by the
    oracle's HOST logic reproduce the reference's known-answer bytes and the oracle's proofs on the MI355X -
    `lmn_prove` is not called (tests/level2_prover.py)."""
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from level2_prover import prove_with_level2_only
    from oracle.channel import ProtocolVariant
    ctx = luminair_amd.Prover(0).ctx
    got, calls = prove_with_level2_only(ctx, syn.simple_example())
    assert got == kat_bytes and calls["logup"] == 2 and calls["composition"] == 2
    got, calls = prove_with_level2_only(ctx, syn.simple_example(), fri_commit=True)    # FRI commit as one lmn_col_fri_commit call
    assert got == kat_bytes and calls["fri_commit"] == 1 and "fold_line" not in calls
    for tabs, variant in ((syn.chain_graph(1 << 12, 7), ProtocolVariant.KAT),
                          (syn.config3_mixed(13, 12, 12, 8), ProtocolVariant.KAT),
                          (syn.less_than_graph(3000, 5), ProtocolVariant.PINNED),
                          (syn.linear_layer(33, 50, 14, True), ProtocolVariant.KAT)):
        from oracle.proof import to_bincode
        from oracle.prover import prove
        want = to_bincode(prove([(k, r.astype(np.uint64)) for k, r in tabs], variant=variant))
        got, _ = prove_with_level2_only(ctx, tabs, variant)
        assert got == want
        got, calls = prove_with_level2_only(ctx, tabs, variant, fri_commit=True)
        assert got == want and calls["fri_commit"] == 1
        # and the whole-proof entry point agrees with both
        p = luminair_amd.Prover(0, protocol_variant=int(variant))
        assert p.prove(luminair_amd.LuminairPie.from_tables(tabs)).to_bincode() == want


def _producer_scenarios():
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import producer_scenarios as ps
    return ps


@pytest.mark.parametrize("idx", range(16))
def test_gpu_reference_expansion_scenarios(hip_lib_path, idx):
    """crates/graph/src/tests/expansions.rs:64-368 on the device-side producer: gen_trace on the MI355X, tables equal
    the numpy mirror, lmn_prove, lmn_verify (logup sums cancel), outputs equal (tests/producer_scenarios.py)."""
    from luminair_amd import backend
    ps = _producer_scenarios()
    ps.run_scenario(backend.default_library(), ps.EXPANSIONS[idx], 42 + idx)


def test_gpu_reference_op_shape_matrix(hip_lib_path):
    """crates/graph/src/tests/mod.rs:50-190 + tests/ops.rs: the binary shape matrix (3x4, 32x32, 17x13, scalar / row /
    column broadcast) for Add and Mul, the unary shape set, the three-way reductions of a (1, 4, 100) tensor, LessThan
    and Contiguous (sliced in the reference's own row rule, permuted, expanded)."""
    from luminair_amd import backend
    ps = _producer_scenarios()
    for build in ps.OPS:
        ps.run_scenario(backend.default_library(), build, 7)


@pytest.mark.parametrize("pow_bits,log_last_layer,n_queries,tabs", [
    (10, 3, 20, syn.chain_graph(1 << 13, 3)),
    (0, 5, 1, syn.config2_add_only(1 << 14, 1)),
    (7, 0, 64, syn.config3_mixed(14, 13, 13, 8)),
    (5, 10, 3, syn.config2_add_only(1 << 12, 5)),
    (16, 9, 300, syn.config2_add_only(1 << 16, 6)),
    (12, 2, 200, syn.linear_layer(64, 100, 13, True)),
])
def test_gpu_non_default_pcs_config_matches_oracle(hip_lib_path, c_oracle, pow_bits, log_last_layer, n_queries, tabs):
    """`lmn_config` other than PcsConfig::default() on the MI355X: byte-equal to the (C) oracle under the same config,
    accepted by `lmn_verify_with_config`, rejected by the default verifier."""
    from luminair_amd import backend
    from oracle.proof import to_bincode
    from oracle.prover import PcsConfig, prove
    p = luminair_amd.Prover(0, pow_bits=pow_bits, log_last_layer=log_last_layer, n_queries=n_queries)
    got = p.ctx.prove_tables([(k, r, len(r)) for k, r in tabs])
    want = to_bincode(prove([(k, r.astype(np.uint64)) for k, r in tabs],
                            PcsConfig(pow_bits=pow_bits, log_last_layer=log_last_layer, n_queries=n_queries), kernels=c_oracle))
    assert got == want
    backend.default_library().verify(got, backend.VARIANT_KAT, config=p.ctx.config)
    with pytest.raises(backend.LuminairBackendError):
        backend.default_library().verify(got, backend.VARIANT_KAT)


def test_gpu_single_table_2_24_rows_equals_c_oracle_bytes(hip_lib_path, c_oracle):
    """One Add table of 2^24 rows (16 x BASELINE config 2): every main / interaction column goes through three-pass
    transforms (LDE of 2^25 rows, composition LDE of 2^26 rows), 2^26-leaf trees, the coalesced logup scan with 2^17
    block totals - index widths the 2^23-row tables of config 5 do not reach.  SHA-256 against the C oracle's proof,
    and the product verifier accepts it.  Rows stay on the device (960 MiB of trace)."""
    from luminair_amd import backend
    from oracle.proof import to_bincode
    from oracle.prover import prove
    tabs = syn.config2_add_only(1 << 24, 7)
    p = luminair_amd.Prover(0)
    bufs = [(k, p.ctx.upload(r), len(r)) for k, r in tabs]
    got = p.ctx.prove_tables(bufs)
    assert p.ctx.prove_tables(bufs) == got                        # deterministic at this size too
    for _, b, _ in bufs:
        b.free()
    p.ctx.close()
    backend.default_library().verify(got, backend.VARIANT_KAT)
    want = to_bincode(prove(tabs, kernels=c_oracle))
    assert len(got) == len(want) and _sha(got) == _sha(want)


def test_gpu_maximum_table_size_2_25_rows(hip_lib_path):
    """The largest table lmn_prove accepts with the default PcsConfig: one Add table of 2^25 rows (LDE 2^26 rows,
    composition LDE and first FRI layer 2^27 rows, 2^27-leaf trees of 4 GiB per level, ~100 GB arena).  Too large for the
    oracle on a test budget: checked by determinism and by the product verifier (itself oracle-checked on the smaller
    sizes); one more row is refused (tests/test_emu_hostlogic.py checks the limits on the CPU)."""
    from luminair_amd import backend
    tabs = syn.config2_add_only(1 << 25, 11)
    p = luminair_amd.Prover(0)
    bufs = [(k, p.ctx.upload(r), len(r)) for k, r in tabs]
    got = p.ctx.prove_tables(bufs)
    assert p.ctx.prove_tables(bufs) == got
    with pytest.raises(backend.LuminairBackendError) as e:
        p.ctx.prove_tables([(k, b, n + 1) for k, b, n in bufs])
    assert e.value.code == backend.ERR_INVALID_ARGUMENT
    for _, b, _ in bufs:
        b.free()
    p.ctx.close()
    backend.default_library().verify(got, backend.VARIANT_KAT)


def test_gpu_prove_submit_wait_from_one_thread(hip_lib_path):
    """Eight contexts kept busy by ONE host thread with lmn_prove_submit / lmn_prove_wait (what a single-threaded
    Rust caller of the reference's `prove` would do): every proof equals the synchronous one, and the single thread
    reaches the multi-threaded throughput."""
    import time
    tabs = syn.config2_add_only(1 << 20, 42)
    provers = [luminair_amd.Prover(0) for _ in range(8)]
    bufs = [[(k, p.ctx.upload(r), len(r)) for k, r in tabs] for p in provers]
    want = provers[0].ctx.prove_tables(bufs[0])
    for p, b in zip(provers, bufs):
        p.ctx.prove_tables(b)
    rounds = 12
    t0 = time.perf_counter()
    for p, b in zip(provers, bufs):
        p.ctx.prove_submit(b)
    for r in range(rounds):
        for p, b in zip(provers, bufs):
            assert p.ctx.prove_wait() == want
            if r + 1 < rounds:
                p.ctx.prove_submit(b)
    dt = time.perf_counter() - t0
    rate = rounds * len(provers) / dt
    print("one host thread, 8 contexts, submit/wait: %.1f proofs/s" % rate)
    assert rate > 300            # the multi-threaded bench reaches ~500; a serial caller would get ~340
    for bl in bufs:
        for _, b, _ in bl:
            b.free()


def test_gpu_prover_pool_prove_many(hip_lib_path):
    """`ProverPool.prove_many` on the MI355X: 8 contexts, 24 different pies from one thread, proofs in input order and
    equal to the synchronous proofs."""
    pool = luminair_amd.ProverPool(0, n=8)
    pies = [luminair_amd.LuminairPie.from_tables(syn.chain_graph(3000 + 257 * i, i)) for i in range(24)]
    want = [pool.provers[0].prove(p).to_bincode() for p in pies]
    assert [p.to_bincode() for p in pool.prove_many(pies)] == want
    pool.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [
    backend.PV_MIX_U64_HASHED | backend.PV_POW_PREFIXED | backend.PV_MUL_ONE_SLOT | backend.PV_RECIP_NEG,
    backend.PV_DRAW_CTR_U32 | backend.PV_RECIP_TWO_SLOTS,
    backend.VARIANT_PINNED | backend.PV_SQRT_TWO_SLOTS | backend.PV_SQRT_NEG | backend.PV_REM_NEG | backend.PV_MUL_ONE_SLOT,
])
def test_gpu_protocol_flag_combinations_equal_oracle(hip_lib_path, c_oracle, flags):
    """Round 5: `protocol_variant` is a set of independent flags (encodings, proof-of-work form, slot count and sign of the
    un-vendored eval_fixed_* helpers).  Combinations away from KAT / PINNED: GPU bytes == C oracle bytes at 2^14 rows, the
    product verifier accepts them under the same flags and rejects them under a neighbouring combination."""
    from oracle.channel import ProtocolVariant
    from oracle.proof import to_bincode
    from oracle.prover import prove
    tabs = syn.sqrt_rem_graph(1 << 14, 4) if flags & backend.PV_CLAIM17 else syn.chain_graph(1 << 14, 5)
    p = luminair_amd.Prover(0, protocol_variant=flags)
    got = p.prove(luminair_amd.LuminairPie.from_tables(tabs)).to_bincode()
    assert got == to_bincode(prove(tabs, variant=ProtocolVariant(flags), kernels=c_oracle))
    luminair_amd.verify(luminair_amd.LuminairProof(got), protocol_variant=flags)
    with pytest.raises(luminair_amd.LuminairError):
        luminair_amd.verify(luminair_amd.LuminairProof(got), protocol_variant=flags ^ backend.PV_MIX_U64_HASHED)
    p.ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("log_blowup,tabs", [(2, syn.config3_mixed(16, 15, 15, 8)), (3, syn.chain_graph(1 << 14, 3)),
                                            (2, syn.config2_add_only(1 << 18, 6))])
def test_gpu_larger_blowups_match_oracle(hip_lib_path, c_oracle, log_blowup, tabs):
    """Blow-up 4 / 8 on the MI355X (the reference only uses blow-up 2): the composition phase evaluates the columns on the
    constraint domain from their coefficients; byte-equal to the C oracle, verified under the same config."""
    from oracle.proof import to_bincode
    from oracle.prover import PcsConfig, prove
    p = luminair_amd.Prover(0, log_blowup=log_blowup)
    got = p.ctx.prove_tables([(k, r, len(r)) for k, r in tabs])
    want = to_bincode(prove([(k, r.astype(np.uint64)) for k, r in tabs], PcsConfig(log_blowup=log_blowup), kernels=c_oracle))
    assert got == want
    backend.default_library().verify(got, backend.VARIANT_KAT, config=p.ctx.config)
    p.ctx.close()
