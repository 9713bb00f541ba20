"""Every record of tests/golden/transcript_redraw_seeds.json (tools/find_redraw.cpp) against plain hashlib.blake2s, and
oracle/channel.py's draw loop against the same: no library is loaded.  A record names where its event happens - a redraw (a
word >= 2P = 0xFFFFFFFE), the accepted word 0xFFFFFFFD (-> P - 1) or a word P among words 0..3 (-> 0): it must happen exactly
there and nowhere else in the record's transcript, and the oracle's channel must use the counters and return the
coordinates that hashlib's words give.  Every other redraw test (tests/fri_checks.py REDRAW_CASES, tests/redraw_checks.py)
starts from these records.  Two consecutive redraws would cost about 2^56 trials and are out of reach."""
import hashlib

import pytest

import transcript_seeds as ts

P = ts.P
RECORDS = ts.load()


def reduce_word(w):
    assert w < 2 * P
    return w - P if w >= P else w


def walk(rec, digest, n_draws):
    """one transcript step by hashlib alone: n_draws accepted draws from `digest` -> [(counter, words, accepted)]"""
    out, ctr = [], 0
    while sum(a for _, _, a in out) < n_draws:
        w = ts.draw_words(digest, ctr, rec["encoding"])
        out.append((ctr, w, all(x < 0xFFFFFFFE for x in w)))
        ctr += 1
        assert ctr <= n_draws + 1, "%s: more than one redraw in one step" % rec["name"]
    return out


def check_step(rec, draws, here, used=4):
    """the event of the record lies in this step (`here`) at the recorded counter, index and value; nothing else anywhere"""
    met = [(c,) + e for c, w, _ in draws for e in ts.events(w, used)]
    if not here:
        assert not met and all(a for _, _, a in draws), (rec["name"], met)
        return
    want = (rec["counters"][0], rec["event"], rec["word_index"], int(rec["word_value"], 16))
    assert want in met, (rec["name"], met)
    assert all(m[0] == want[0] and m[1] == want[1] for m in met), (rec["name"], met)
    rejected = [c for c, _, a in draws if not a]
    assert rejected == ([want[0]] if rec["event"] == "redraw" else []), (rec["name"], rejected)
    if rec["event"] == "redraw":
        assert rec["counters"] == [want[0], want[0] + 1] and int(rec["word_value"], 16) in ts.REJECTED


@pytest.mark.parametrize("rec", [r for r in RECORDS if r["mode"] == "chain"], ids=lambda r: "%s_tree_%d" % (r["name"].replace(" ", "_"), r["layer"]))
def test_chain_record(rec):
    """mix_root(r_i); draw_felt() over the record's roots from its start digest"""
    d, want_alphas = bytes.fromhex(rec["digest"]), []
    for j, root in enumerate(rec["roots"]):
        d = hashlib.blake2s(d + bytes.fromhex(root)).digest()
        draws = walk(rec, d, 1)
        check_step(rec, draws, j == rec["layer"])
        assert [c for c, _, _ in draws] == (rec["counters"] if j == rec["layer"] else [0])
        want_alphas.append(tuple(reduce_word(x) for x in draws[-1][1][:4]))
    a = want_alphas[rec["layer"]]
    if rec["event"] == "accept-edge" and rec["word_index"] < 4:
        assert a[rec["word_index"]] == P - 1
    if rec["event"] == "reduce-edge":
        assert a[rec["word_index"]] == 0
    ch = ts.CountingChannel(ts.variant_of(rec))
    ch.digest = bytes.fromhex(rec["digest"])
    got = []
    for root in rec["roots"]:
        ch.mix_root(bytes.fromhex(root))
        got.append(tuple(int(v) for v in ch.draw_felt().v))
    assert got == want_alphas and ch.digest == d
    ts.check_chain(rec, ch, len(rec["roots"]), rec["name"])


@pytest.mark.parametrize("rec", [r for r in RECORDS if r["mode"] == "trace"], ids=lambda r: r["name"].replace(" ", "_"))
def test_trace_record(rec):
    """the kind-1 step: mix_root(root 1) into the digest after the claims, then n_draws draw_felts(2) on a running counter"""
    d = hashlib.blake2s(bytes.fromhex(rec["claims_digest"]) + bytes.fromhex(rec["root"])).digest()
    draws = walk(rec, d, rec["n_draws"])
    check_step(rec, draws, True, 8)
    accepted = [(c, w) for c, w, a in draws if a]
    assert rec["counters"][0] == rec["set"]
    if rec["event"] == "redraw":
        # the redraw is in set `set`: that many accepted draws lie before it, and every later set's counter is one higher
        assert [c for c, _ in accepted] == [s + (s >= rec["set"]) for s in range(rec["n_draws"])]
    else:
        assert [c for c, _ in accepted] == list(range(rec["n_draws"])) and rec["counters"] == [rec["set"]]
    ch = ts.CountingChannel(ts.variant_of(rec))
    ch.digest = bytes.fromhex(rec["claims_digest"])
    ch.mix_root(bytes.fromhex(rec["root"]))
    for s in range(rec["n_draws"]):
        z, alpha = ch.draw_felts(2)
        w = [reduce_word(x) for x in accepted[s][1]]
        assert (tuple(int(v) for v in z.v), tuple(int(v) for v in alpha.v)) == (tuple(w[:4]), tuple(w[4:])), (rec["name"], s)
        if s == rec["set"] and rec["event"] != "redraw":
            assert w[rec["word_index"]] == (0 if rec["event"] == "reduce-edge" else P - 1)
    assert [(c, list(w)) for _, c, w in ch.draws] == [(c, w) for c, w, _ in draws]
    assert ch.n_sent == rec["n_draws"] + (rec["event"] == "redraw")


def test_records_cover_both_encodings_and_every_event():
    chain = [r for r in RECORDS if r["mode"] == "chain"]
    assert {(r["encoding"], r["event"]) for r in chain} == {(e, ev) for e in (64, 37) for ev in ("redraw", "accept-edge", "reduce-edge")}
    redraws = [r for r in chain if r["event"] == "redraw"]
    assert {int(r["word_value"], 16) for r in redraws} == set(ts.REJECTED)
    assert {r["word_index"] >= 4 for r in redraws} == {False, True}      # words draw_felt never uses force the redraw too
    trace = [r for r in RECORDS if r["mode"] == "trace"]
    assert {(r["encoding"], r["set"]) for r in trace if r["event"] == "redraw"} == {(64, 0), (37, 0), (64, 4), (37, 4)}
    assert {r["set"] for r in trace if r["event"] == "redraw"} == {0, 4} and "reduce-edge" in {r["event"] for r in trace}
