#!/usr/bin/env python3
"""What preparing a circuit's settings once is worth on BASELINE config 4 (the 2-64-64-1 tanh MLP with its 2^17-row exp2 LUT).

Three figures per run, in one process on one box:

  solo     latency of one proof on one context: p50 / min / max of 31 proofs after 5 warm-ups (the prepared form adds
           `solo_in_turn_p50_ms`: the unchanged and the prepared path proof by proof in turn on one context)
  batch16  proofs/s of one lock-step group of 16 (the argument arrays marshalled once, as a C caller has them)
  groups2  proofs/s of two such groups driven at once by one thread each, as DESIGN.md section 8 quotes them

in one of three forms:

  parent    the package tree of the PARENT commit (--parent DIR: a checkout of it with its libraries built), driven through
            entry points the parent has: `Context.prove_tables(pie, luts)`, `BatchProver.prove_batch(marshalled)`
  plain     this tree, the same entry points: the existing path, which the feature must have left alone
  prepared  this tree, `PreparedSettings` once and `prepared=` on every proof

  prepared_rate.py --parent DIR --out profiles/prepared_settings_rate.json    parent, plain, prepared alternating, five
                                                              rounds, every run a child process under its own time limit;
                                                              stops at the first failure
  prepared_rate.py --one FORM [--parent DIR]                  one run, one JSON line

Expected, not promised (written into the file, nothing is tuned to it): the prepared form's slowest run beats the parent's
fastest, for solo latency and for both batch throughputs; and plain agrees with parent within the spread of the parent's
own runs."""
import argparse
import json
import os
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("parent", "plain", "prepared")
ROUNDS = 5
SOLO_WARMUP, SOLO_PROOFS = 5, 31
BATCH = 16
CHILD_LIMIT_S = 240


def measure(form, parent_dir):
    sys.path.insert(0, parent_dir if form == "parent" else ROOT)
    from luminair_amd import backend, synthetic as syn
    from luminair_amd.batch import BATCH_LIB, BatchProver
    assert os.path.dirname(os.path.dirname(os.path.abspath(backend.__file__))) == os.path.abspath(sys.path[0])
    tabs, luts = syn.config4_black_scholes_shape()
    pie = [(k, r, len(r)) for k, r in tabs]
    lib = backend.default_library()
    cfg = lib.default_config()
    cfg.protocol_variant = backend.VARIANT_PINNED
    ctx = backend.Context(0, cfg, lib)
    want = ctx.prove_tables(pie, luts)
    lib.verify(want, backend.VARIANT_PINNED)
    out = {"form": form}

    if form == "prepared":
        t0 = time.perf_counter()
        pp = backend.PreparedSettings(0, cfg, luts, backend.LOOKUP_EXP2, lib)
        out["prepare_ms"] = round((time.perf_counter() - t0) * 1e3, 3)

        def solo():
            return ctx.prove_tables(pie, prepared=pp)
    else:
        def solo():
            return ctx.prove_tables(pie, luts)
    same = solo() == want
    for _ in range(SOLO_WARMUP):
        solo()
    ms = []
    for _ in range(SOLO_PROOFS):
        t0 = time.perf_counter()
        solo()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    out["solo_ms"] = {"p50": round(ms[len(ms) // 2], 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}
    if form == "prepared":
        # the two paths in ONE process, proof by proof in turn: free of the run-to-run spread of a process's p50
        turn = {"plain": [], "prepared": []}
        for _ in range(SOLO_PROOFS):
            for name, kw in (("plain", {"luts": luts}), ("prepared", {"prepared": pp})):
                t0 = time.perf_counter()
                ctx.prove_tables(pie, **kw)
                turn[name].append((time.perf_counter() - t0) * 1e3)
        out["solo_in_turn_p50_ms"] = {k: round(sorted(v)[len(v) // 2], 4) for k, v in turn.items()}
        pp.close()
    ctx.close()

    pies = [pie] * BATCH
    for groups in (1, 2):
        bps = [BatchProver(0, BATCH, protocol_variant=backend.VARIANT_PINNED) for _ in range(groups)]
        bpp = backend.PreparedSettings(0, cfg, luts, backend.LOOKUP_EXP2, backend.Library(BATCH_LIB)) if form == "prepared" else None
        kw = {"prepared": bpp} if bpp is not None else {}
        ms_ = [bp.marshal(pies, luts) for bp in bps]
        for bp, m in zip(bps, ms_):
            same = same and bp.prove_batch(m, **kw) == [want] * BATCH
            bp.prove_batch(m, **kw)
        reps = max(5, 1200 // (BATCH * groups)) * 2
        start = threading.Barrier(groups + 1)
        bad = []

        def drive(bp, m):
            start.wait()
            for _ in range(reps):
                if bp.prove_batch(m, **kw)[0] != want:
                    bad.append(1)

        ths = [threading.Thread(target=drive, args=(bp, m)) for bp, m in zip(bps, ms_)]
        for t in ths:
            t.start()
        start.wait()
        t0 = time.perf_counter()
        for t in ths:
            t.join()
        dt = time.perf_counter() - t0
        same = same and not bad
        out["batch16_proofs_per_s" if groups == 1 else "groups2_proofs_per_s"] = round(BATCH * groups * reps / dt, 1)
        if groups == 1:
            c = bps[0].counters()
            out["batch16_counters_total"] = {k: c[k] for k in ("launches", "host_waits", "copy_launches", "direct_copies")}
        for bp in bps:
            bp.close()
        if bpp is not None:
            bpp.close()
    out["bytes_identical_to_lmn_prove"] = bool(same)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", choices=FORMS)
    ap.add_argument("--parent", default=None, help="package tree of the parent commit, built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prepared_settings_rate.json"))
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    args = ap.parse_args()
    if args.one:
        if args.one == "parent" and not args.parent:
            ap.error("--one parent needs --parent DIR")
        print(json.dumps(measure(args.one, os.path.abspath(args.parent) if args.parent else None)), flush=True)
        return 0
    if not args.parent:
        ap.error("--parent DIR: the baseline is the parent commit")
    runs = []
    for rnd in range(args.rounds):
        for form in FORMS:
            r = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--one", form,
                                "--parent", args.parent], capture_output=True, text=True)
            if r.returncode != 0:
                print("%s, round %d failed (exit %d): %s" % (form, rnd, r.returncode, r.stderr[-2000:]), flush=True)
                return 1                      # nothing more is started on the GPU after a failure
            runs.append(dict(json.loads(r.stdout.strip().splitlines()[-1]), round=rnd))
            print(json.dumps(runs[-1]), flush=True)

    def col(form, key):
        return [r[key]["p50"] if key == "solo_ms" else r[key] for r in runs if r["form"] == form]

    summary, accept = {}, {}
    for key in ("solo_ms", "batch16_proofs_per_s", "groups2_proofs_per_s"):
        summary[key] = {f: [min(col(f, key)), max(col(f, key))] for f in FORMS}
        par, pre, pla = col("parent", key), col("prepared", key), col("plain", key)
        faster = (lambda a, b: a < b) if key == "solo_ms" else (lambda a, b: a > b)
        worst_pre = max(pre) if key == "solo_ms" else min(pre)
        best_par = min(par) if key == "solo_ms" else max(par)
        accept[key] = {"prepared_slowest_beats_parent_fastest": faster(worst_pre, best_par),
                       "plain_within_parent_spread": min(par) - (max(par) - min(par)) <= sum(pla) / len(pla)
                       <= max(par) + (max(par) - min(par))}
    doc = {"what": "BASELINE config 4 (tanh MLP 2-64-64-1, 2^17-row exp2 LUT) on one MI355X: solo latency (p50 / min / max of %d "
                   "proofs, ms), proofs/s of one lock-step group of %d and of two groups at once; parent = the parent commit's "
                   "tree, plain = this tree through the same entry points, prepared = PreparedSettings once and prepared= "
                   "per proof; the three forms alternate, every run is listed in order" % (SOLO_PROOFS, BATCH),
           "rounds": args.rounds, "runs": runs, "ranges_min_max": summary, "expected_not_promised": accept}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"ranges_min_max": summary, "expected_not_promised": accept}), flush=True)
    print("wrote", args.out, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
