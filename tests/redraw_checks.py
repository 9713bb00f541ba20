"""A whole proof whose relation draws redraw (`ChanStep` kind 1: `mix_root(root 1)`, then one `draw_felts(2)` per relation
element set with a counter that runs on - a redraw in set i moves the counter of every later set).  Run against the
emulation build on CPU (tests/test_redraw_emu.py) and the HIP library on GPU (tests/test_gpu_redraw.py).

The pie: `synthetic.config2_graph_faithful` with 8 Add rows - Add consumes lhs and rhs with multiplicity -1 and an Inputs
table of 16 rows yields them with multiplicity 1 (LMN_PV_CLAIM17 gives Inputs its claim slot).  Both tables are padded to /
have 16 rows, the smallest there is, and the pie proves under the default configuration (last layer 2^0).  Its logup
fractions are built from the node relation's elements (z, alpha: the first set drawn), so the interaction trace, the
claimed sums, root 2, the composition and every byte behind them depend on what the kind-1 step drew:
`check_reference_depends_on_the_draws` asserts that the reference's bytes change when they do.  (A pie whose
multiplicities are all 0, `config2_add_only`, gives the same bytes whatever is drawn and would compare nothing.)  In one
Add row `lhs` and `out` move together by a free value v, and so does the Inputs row that yields that lhs: out - lhs - rhs = 0
and the logup balance hold for every v, the change is linear in v, so the committed LDE is base + v * delta and
tools/find_redraw.cpp (main-trace mode, `write_search_file` makes its input) can try 2^28 values of v.  The records of
tests/golden/transcript_redraw_seeds.json with mode "trace" hold the v found: per draw encoding one at which the first set
redraws and one at which the last set does, all with LMN_PV_LUT_DRAWS4 (five sets), so that a redraw in the first set moves
four later counters and one in the last set comes behind four accepted ones.  A fifth record holds a v at which one of the step's 40 accepted words equals P (no redraw; that coordinate of the set's
element is 0 in the oracle's own draw): the accept side of `qchan_draw_felts8`'s reduction.  Aiming it at the first set
alone would cost about 2^29 trials.

What the bytes witness, and what they do not: the first set's elements reach every byte, so a first-set redraw that the
library resolves to other words than the oracle (the draw at counter 1) gives other bytes, under LMN_HOST_FS=1 too, where
the host `Channel` is alone.  The pie has no lookup, so the elements of sets 1 .. 4 (sin, exp2, log2, range check) reach no
byte (asserted as well, so that this stays a stated fact): a last-set redraw is witnessed by the oracle's counting channel
and, in the library, by the host replay of the device transcript, which compares `qchan_draw_felts8` with host.h and throws
on a difference - a fault the two share in sets 1 .. 4 would pass.  Closing that needs a lookup relation in the pie: the
range check (the last set) has a table of 256 rows, some twenty times this search; a LUT of 16 rows would bring sets 1 .. 3
into the bytes and is the next step.  The same pie cannot go through `lmn_prove_prepared`, which prepares lookup tables.

Reference - never the library under test: oracle.prover.prove on a counting channel (tests/transcript_seeds.py), which must
have redrawn in exactly the recorded set, and only there in the whole proof, before the library is asked; oracle.verifier
must accept the proof.  Then `lmn_prove` returns the oracle's bytes by default (the step inside k_merkle_small), under
LMN_CHAN_STEP_SEPARATE=1 (k_chan_step), LMN_HOST_FS=1 (the host `Channel` alone) and LMN_HOST_QUOT=1; `lmn_verify` accepts
them; and the pie as the middle member of a three-member lock-step batch gives the same bytes while its neighbours, which do
not redraw, still equal their solo proofs.

Out of reach: the draws of kinds 2 and 3 and of k_quot_prepare.  Their digests depend on everything proved before them, so
a hit costs about 2^28 whole proofs; they call the same `qchan_draw_felts8` as kind 1, with a fresh counter.  Two
consecutive redraws (about 2^56 trials) are out of reach everywhere."""
import functools
import os
import struct
from contextlib import contextmanager

import numpy as np

import transcript_seeds as ts
from fri_checks import environment
from luminair_amd import backend, synthetic as syn

P = ts.P
ROWS, PIE_SEED, ROW, LHS_COL, OUT_COL, INPUT_VAL_COL = 8, 11, 5, 9, 11, 5
SWITCHES = ({}, {"LMN_CHAN_STEP_SEPARATE": 1}, {"LMN_HOST_FS": 1}, {"LMN_HOST_QUOT": 1})
# record name -> protocol variant (LMN_PV_*): five relation sets, and a claim slot for Inputs, in all
_V64 = backend.PV_LUT_DRAWS4 | backend.PV_CLAIM17
VARIANTS = {"add8 inputs first set": _V64, "add8 inputs first set u32": _V64 | backend.PV_DRAW_CTR_U32,
            "add8 inputs last set": _V64, "add8 inputs last set u32": _V64 | backend.PV_DRAW_CTR_U32,
            "add8 inputs word P": _V64}


def tables(v, seed=PIE_SEED):
    """the pie with lhs and out of Add's row ROW, and the Inputs row that yields that lhs, moved by v"""
    (add_kind, add), (inp_kind, inp) = syn.config2_graph_faithful(ROWS, seed)
    add, inp = add.copy(), inp.copy()
    assert inp[ROW, INPUT_VAL_COL] == add[ROW, LHS_COL]      # Inputs rows 0 .. ROWS - 1 yield the lhs values, in order
    for rows, col in ((add, LHS_COL), (add, OUT_COL), (inp, INPUT_VAL_COL)):
        rows[ROW, col] = (int(rows[ROW, col]) + v) % P
    return [(add_kind, add), (inp_kind, inp)]


@contextmanager
def counting_channels():
    """oracle.prover builds its channel itself: hand it the counting one"""
    import oracle.prover as op
    made = []

    class Counting(ts.CountingChannel):
        burn_before = None      # a set: two counter values are skipped before its draw, so it and every later set draw other words

        def __init__(self, variant):
            super().__init__(variant)
            self.sets = 0
            made.append(self)

        def draw_felts(self, n):
            if n == 2:          # the kind-1 step's draws are the proof's first of this form
                if self.sets == self.burn_before:
                    self.n_sent += 2        # two: one alone would only do what a redraw in that set does
                self.sets += 1
            return super().draw_felts(n)
    old, op.Blake2sChannel = op.Blake2sChannel, Counting
    try:
        yield made
    finally:
        op.Blake2sChannel = old


def oracle_run(tabs, variant, burn_before=None):
    """-> (proof bytes, the draws of the kind-1 step [(counter, words)], every rejected draw of the proof [(mixes, counter)],
    the trace, the eight coordinates of each set as the oracle's draw_felts(2) returned them)"""
    from oracle.channel import ProtocolVariant
    from oracle.proof import to_bincode
    from oracle.prover import prove
    from oracle.verifier import VerificationError, verify
    with counting_channels() as made:
        import oracle.prover as op
        op.Blake2sChannel.burn_before = burn_before
        proof, tr = prove([(k, r.astype(np.uint64)) for k, r in tabs], variant=ProtocolVariant(variant), want_trace=True)
    ch, = made
    g = ch.digest_after.index(tr.digests["root1"]) + 1
    try:        # the pie is still valid: the prover's own degree check is not the only witness
        verify(proof, ProtocolVariant(variant))
    except VerificationError:
        assert burn_before is not None
        tr.digests["refused by the verifier"] = b"1"
    sets = [f for m, f in ch.felts if m == g]
    assert ch.sets >= len(sets) and (tuple(tr.z.v) + tuple(tr.alpha_rel.v)) == sets[0]
    return to_bincode(proof), [(c, w) for m, c, w in ch.draws if m == g], [(m - g, c) for m, c, _ in ch.redraws()], tr, sets


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's proof of the record's pie, once per record; the oracle redrew in the recorded set and nowhere else"""
    rec, variant = ts.trace_record(name), VARIANTS[name]
    assert rec["encoding"] == (37 if variant & backend.PV_DRAW_CTR_U32 else 64) and rec["n_draws"] == 5, rec
    want, step, rejected, tr, sets = oracle_run(tables(rec["value"]), variant)
    c0 = rec["counters"][0]
    assert len(sets) == rec["n_draws"], (name, len(sets))
    if rec["event"] != "redraw":    # an accepted word at the reduction's edge: P -> 0 in a relation element
        assert not rejected and [c for c, _ in step] == list(range(rec["n_draws"])), (name, rejected)
        assert [(c,) + e for c, w in step for e in ts.events(w, 8)] == [(c0, rec["event"], rec["word_index"], int(rec["word_value"], 16))], name
        assert c0 == rec["set"], name
        assert sets[rec["set"]][rec["word_index"]] == (0 if rec["event"] == "reduce-edge" else P - 1), name     # the oracle's own element
        assert tr.roots[1].hex() == rec["root"], name
        return want
    assert rejected, "%s: the reference did not redraw - the seed no longer fits the protocol" % name
    assert rejected == [(0, c0)], "%s: the reference redrew at (mixes after root 1, counter) %s" % (name, rejected)
    assert c0 == rec["set"] and [c for c, _ in step] == list(range(rec["n_draws"] + 1)), (name, step)
    assert step[c0][1][rec["word_index"]] == int(rec["word_value"], 16) and tr.roots[1].hex() == rec["root"], name
    return want


def accepted(step):
    """the counters of the step's accepted draws"""
    return [c for c, w in step if all(x < 2 * P for x in w)]


def check_reference_depends_on_the_draws(name):
    """The comparison with the oracle's bytes sees the draws under test: the reference's proof of the record's pie changes when
    the first set draws other words (two counter values skipped before it), so a library that resolves the step otherwise
    cannot return the same bytes.  Skipping them before the second set moves sets 1 .. 4 alone and changes nothing: the pie
    has no lookup (the module docstring says what witnesses those sets)."""
    rec, variant, want = ts.trace_record(name), VARIANTS[name], reference(name)
    first = 1 if (rec["set"], rec["event"]) == (0, "redraw") else 0       # the counter of the first set's accepted draw
    moved, step, _, tr, _ = oracle_run(tables(rec["value"]), variant, burn_before=0)
    assert accepted(step)[0] == 2 != first and moved != want, name
    # and the oracle's verifier, which draws for itself, refuses a proof built from other elements
    assert "refused by the verifier" in tr.digests, "%s: a proof built from other relation elements verifies" % name
    later, step, _, tr, _ = oracle_run(tables(rec["value"]), variant, burn_before=1)
    assert accepted(step)[:2] == [first, first + 3], (name, accepted(step))
    assert later == want and "refused by the verifier" not in tr.digests, \
        "%s: the elements of sets 1 .. 4 reach the proof's bytes now: say so in the module docstring" % name


@functools.lru_cache(maxsize=None)
def neighbour(variant, seed):
    """a pie of the same shape that does not redraw"""
    tabs = tables(0, seed)
    want, _, rejected, _, _ = oracle_run(tabs, variant)
    assert not rejected, seed
    return tabs, want


def _pie(tabs):
    return [(k, r, len(r)) for k, r in tabs]


def check_prove(lib, name):
    rec, variant, want = ts.trace_record(name), VARIANTS[name], reference(name)
    cfg = lib.default_config()
    cfg.protocol_variant = variant
    ctx = backend.Context(0, cfg, lib)
    try:
        pie = _pie(tables(rec["value"]))
        for env in SWITCHES:
            base = {k: None for s in SWITCHES for k in s}
            with environment(**{**base, **env}):
                got = ctx.prove_tables(pie)
            assert got == want, "%s (%s): lmn_prove differs from the oracle's proof" % (name, env or "default")
    finally:
        ctx.close()
    lib.verify(want, variant)


def check_batch(lib, batch_so, name):
    from luminair_amd.batch import BatchProver
    rec, variant, want = ts.trace_record(name), VARIANTS[name], reference(name)
    (t0, w0), (t2, w2) = neighbour(variant, 21), neighbour(variant, 22)
    bp = BatchProver(0, 3, protocol_variant=variant, library_path=batch_so)
    try:
        got = bp.prove_batch([_pie(t0), _pie(tables(rec["value"])), _pie(t2)])
    finally:
        bp.close()
    assert got[1] == want, "%s: the redrawing member of the batch differs from the oracle's proof" % name
    assert got[0] == w0 and got[2] == w2, "%s: a member next to the redrawing one differs from its solo proof" % name


# ----------------------------------------------------------------------------- the searcher's input
def write_search_file(path, name):
    """tools/find_redraw.cpp main-trace mode: the digest after the claims, the base LDE and the LDE of the unit change, in the
    leaf order of tree 1 (one table: the table's column order)"""
    from oracle.channel import ProtocolVariant
    from oracle.prover import prove
    variant = VARIANTS[name]
    tabs = tables(0)
    _, tr = prove([(k, r.astype(np.uint64)) for k, r in tabs], variant=ProtocolVariant(variant), want_trace=True)
    base = [np.asarray(e, dtype=np.uint64) for e in tr.trees[1].evals]
    _, tr1 = prove([(k, r.astype(np.uint64)) for k, r in tables(1)], variant=ProtocolVariant(variant), want_trace=True)
    delta = [(np.asarray(e, dtype=np.uint64) + np.uint64(P) - b) % np.uint64(P) for b, e in zip(base, tr1.trees[1].evals)]   # the unit change
    n = len(base[0])
    assert all(len(c) == n for c in base + delta) and len(base) == len(delta)    # one leaf size: the searcher's Merkle tree
    moved = tables(12345)
    _, tr2 = prove([(k, r.astype(np.uint64)) for k, r in moved], variant=ProtocolVariant(variant), want_trace=True)
    for b, d, e in zip(base, delta, tr2.trees[1].evals):     # linear in v
        assert np.array_equal((b + np.uint64(12345) * d) % np.uint64(P), np.asarray(e, dtype=np.uint64))
    assert tr2.digests["claims"] == tr.digests["claims"]
    with open(path, "wb") as f:
        f.write(struct.pack("<3I", 0x4c4d4e52, 37 if variant & backend.PV_DRAW_CTR_U32 else 64, 5))
        f.write(tr.digests["claims"])
        f.write(struct.pack("<2I", n.bit_length() - 1, len(base)))
        for c in base + delta:
            f.write(np.asarray(c, dtype="<u4").tobytes())
    return tr2.roots[1].hex()


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if len(sys.argv) == 3 and sys.argv[1] in VARIANTS:
        print("root at v = 12345 (compare with `find_redraw trace-root %s 12345`): %s" % (sys.argv[2], write_search_file(sys.argv[2], sys.argv[1])))
    else:
        sys.exit("usage: redraw_checks.py <%s> <file to write>" % " | ".join('"%s"' % n for n in VARIANTS))
