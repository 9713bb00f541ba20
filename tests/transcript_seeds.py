"""The records of tests/golden/transcript_redraw_seeds.json (found by tools/find_redraw.cpp) and the counting channel every
redraw test asks before it asks the library: inputs at which `draw_base_felts` takes its rare paths - a redraw (a word
>= 2P; about 2^-28 per draw), the largest accepted word 0xFFFFFFFD (-> P - 1) and a word equal to P (-> 0).  Nothing here
loads a library: hashlib and oracle/channel.py only.  Two consecutive redraws (about 2^56 trials) are out of reach."""
import hashlib
import json
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.channel import Blake2sChannel, ProtocolVariant          # noqa: E402

P = 2 ** 31 - 1
REJECTED = (0xFFFFFFFE, 0xFFFFFFFF)
ACCEPT_EDGE, REDUCE_EDGE = 0xFFFFFFFD, P
SEEDS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transcript_redraw_seeds.json")


class CountingChannel(Blake2sChannel):
    """oracle.channel.Blake2sChannel that records every draw: `draws` = [(mixes so far, counter, the eight words)], and what
    every draw_felts call returned: `felts` = [(mixes so far, the coordinates of the elements)]"""

    def __init__(self, variant=ProtocolVariant.KAT):
        super().__init__(variant)
        self.mixes, self.draws, self.digest_after, self.felts = 0, [], [], []

    def draw_felts(self, n):
        out = super().draw_felts(n)
        self.felts.append((self.mixes, tuple(int(v) for q in out for v in q.v)))
        return out

    def _update(self, d):
        super()._update(d)
        self.mixes += 1
        self.digest_after.append(d)

    def draw_random_bytes(self):
        ctr = self.n_sent
        b = super().draw_random_bytes()
        self.draws.append((self.mixes, ctr, tuple(int.from_bytes(b[4 * i:4 * i + 4], "little") for i in range(8))))
        return b

    def redraws(self):
        """the draws that were rejected"""
        return [d for d in self.draws if any(w >= 2 * P for w in d[2])]


LIMIT = 120         # seconds; a case takes a few, on a loaded machine some tens
_SPINNING = []      # the cases whose call never answered: their threads still run, inside contexts later tests share


def bounded(limit, fn, *args):
    """fn(*args) on a thread of its own, for the emulation build only: a draw loop that never ends - the counter not advanced
    on a redraw - fails the test after `limit` seconds where it would hang the run.  The thread is left spinning until the
    process ends, possibly inside a context that a fixture hands to later tests, so every later call fails at once, naming
    the case that hung: one wait per run, and no context is used from two threads.  On a device the same fault is an
    endless kernel, and nothing of this kind is done there.  A call that returns costs no wait."""
    assert not _SPINNING, "not run: %s gave no answer and its thread still runs in this process" % _SPINNING[0]
    box = {}

    def run():
        try:
            box["value"] = fn(*args)
        except BaseException as e:      # handed to the caller
            box["error"] = e
    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(limit)
    if t.is_alive():
        _SPINNING.append("%s%r" % (getattr(fn, "__name__", fn), tuple(getattr(a, "id", a) for a in args if isinstance(a, str) or hasattr(a, "id"))))
        raise AssertionError("no answer within %d s: a draw loop that never accepts (is the counter advanced on a redraw?)" % limit)
    if "error" in box:
        raise box["error"]
    return box.get("value")


def load():
    with open(SEEDS_PATH) as f:
        return json.load(f)["records"]


def chain_record(name, layer):
    hits = [r for r in load() if r["mode"] == "chain" and r["name"] == name and r["layer"] == layer]
    assert len(hits) == 1, "tests/golden/transcript_redraw_seeds.json: %d records for %r layer %d" % (len(hits), name, layer)
    return hits[0]


def trace_record(name):
    hits = [r for r in load() if r["mode"] == "trace" and r["name"] == name]
    assert len(hits) == 1, "tests/golden/transcript_redraw_seeds.json: %d records for %r" % (len(hits), name)
    return hits[0]


def variant_of(rec):
    return ProtocolVariant.DRAW_CTR_U32 if rec["encoding"] == 37 else ProtocolVariant.KAT


def draw_words(digest, ctr, encoding):
    """plain hashlib: the eight words of draw number `ctr`"""
    tail = ctr.to_bytes(8, "little") + bytes(24) if encoding == 64 else ctr.to_bytes(4, "little") + b"\0"
    b = hashlib.blake2s(digest + tail).digest()
    return [int.from_bytes(b[4 * i:4 * i + 4], "little") for i in range(8)]


def events(words, used=4):
    """what a draw's words meet: ("redraw" | "accept-edge" | "reduce-edge", index, value) each; `used`: how many of the
    words become coordinates (draw_felt: 4, draw_felts(2): 8) - a word P among the others is reduced and dropped"""
    out = []
    for k, w in enumerate(words):
        if w in REJECTED:
            out.append(("redraw", k, w))
        elif w == ACCEPT_EDGE:
            out.append(("accept-edge", k, w))
        elif w == REDUCE_EDGE and k < used:
            out.append(("reduce-edge", k, w))
    return out


def check_chain(rec, chan, n_layers, what):
    """`chan`: the CountingChannel a chain `mix_root; draw_felt` of n_layers layers ran on, from a digest set by hand.  The
    event lies exactly where the record says and nowhere else."""
    per = [[] for _ in range(n_layers)]
    for mixes, ctr, words in chan.draws:
        per[mixes - 1].append((ctr, words))
    for l, ds in enumerate(per):
        ctrs = [c for c, _ in ds]
        met = [(c,) + e for c, w in ds for e in events(w)]
        if l != rec["layer"]:
            assert ctrs == [0] and not met, "%s: layer %d drew at counters %s and met %s" % (what, l, ctrs, met)
            continue
        assert met, "%s: the reference met no %s at layer %d - the seed no longer fits the protocol" % (what, rec["event"], l)
        assert ctrs == rec["counters"], "%s: layer %d drew at counters %s, the record has %s" % (what, l, ctrs, rec["counters"])
        assert (rec["counters"][0], rec["event"], rec["word_index"], int(rec["word_value"], 16)) in met, (what, met)
        assert all(m[0] == rec["counters"][0] and m[1] == rec["event"] for m in met), (what, met)
