#!/usr/bin/env python3
"""Rate of `lmn_verify_many` against a loop of `lmn_verify_with_config` on one host thread, on one MI355X box
(profiles/verify_many_rate.json).

Shapes: the 32x32 benchmark shape (`synthetic.config2_graph_faithful(1024, seed)`: Add 2^10 rows + Inputs 2^11 rows) at the
default config (3 queries) and at 70 queries, PINNED protocol variant (as bench.py proves this shape).  16 different proofs per shape are made on the GPU and cycled to n.
Forms, alternating within every round:
  verify_many   one `lmn_verify_many` call over n = 1, 64 and 1024 proofs (raw C call on prebuilt argument arrays)
  host_loop     n calls of `lmn_verify_with_config` on the calling thread over the same proofs
Per form and n: proofs/s (wall clock around calls that end in the library's own wait), host CPU time per proof
(`time.process_time`: the whole process, so a busy-polling wait counts), and - for verify_many - launches and host waits
per call from lmn_ctx_counter 18 and 19.  The reference of every figure is the host loop in the same process.

Usage: verify_many_rate.py [--rounds N] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from luminair_amd import backend, synthetic as syn  # noqa: E402

N_DISTINCT = 16
SIZES = (1, 64, 1024)


def make_proofs(lib, n_queries):
    cfg = lib.default_config()
    cfg.n_queries = n_queries
    cfg.protocol_variant = backend.VARIANT_PINNED   # the Inputs component has a claim slot under this variant only
    ctx = backend.Context(0, cfg, lib)
    try:
        return cfg, [ctx.prove_tables([(k, r, len(r)) for k, r in syn.config2_graph_faithful(1024, 100 + i)])
                     for i in range(N_DISTINCT)]
    finally:
        ctx.close()


def timed(f, n):
    c0, t0 = time.process_time(), time.perf_counter()
    f()
    t1, c1 = time.perf_counter(), time.process_time()
    return {"proofs_per_s": n / (t1 - t0), "host_cpu_us_per_proof": 1e6 * (c1 - c0) / n}


def measure(lib, ctx, cfg, proofs, n, rounds):
    L = lib.lib
    batch = [proofs[i % len(proofs)] for i in range(n)]
    ptrs = (C.c_char_p * n)(*batch)
    lens = (C.c_size_t * n)(*[len(p) for p in batch])
    res = (backend.LmnVerifyResult * n)()
    reps = max(1, 2048 // n)   # enough work per timed window

    def many():
        for _ in range(reps):
            rc = L.lmn_verify_many(ctx.handle, ptrs, lens, n, None, C.byref(cfg), res)
            assert rc == 0, rc

    def loop():
        for _ in range(reps):
            for p in batch:
                assert L.lmn_verify_with_config(p, len(p), None, C.byref(cfg)) == 0
    many()   # warm-up: code objects, the context's verify buffers
    assert all(r.rc == 0 and r.stage == 1 for r in res), [(r.rc, r.stage) for r in res][:4]
    loop()
    before = [ctx.counter(k) for k in (18, 19)]
    runs = {"verify_many": [], "host_loop": []}
    for _ in range(rounds):
        runs["verify_many"].append(timed(many, n * reps))
        runs["host_loop"].append(timed(loop, n * reps))
    after = [ctx.counter(k) for k in (18, 19)]
    calls = rounds * reps
    out = {"n": n, "calls_per_window": reps, "rounds": rounds,
           "launches_per_call": (after[0] - before[0]) / calls, "host_waits_per_call": (after[1] - before[1]) / calls}
    for form, rs in runs.items():
        out[form] = {k: {"median": statistics.median(r[k] for r in rs), "min": min(r[k] for r in rs), "max": max(r[k] for r in rs)}
                     for k in ("proofs_per_s", "host_cpu_us_per_proof")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_many_rate.json"))
    args = ap.parse_args()
    lib = backend.default_library()
    doc = {"tool": "tools/verify_many_rate.py", "shape": "32x32 benchmark shape: Add 2^10 rows + Inputs 2^11 rows",
           "distinct_proofs": N_DISTINCT, "reference": "host_loop: lmn_verify_with_config on one host thread, same process, alternating",
           "configs": []}
    for n_queries in (3, 70):
        cfg, proofs = make_proofs(lib, n_queries)
        ctx = backend.Context(0, cfg, lib)
        try:
            rows = [measure(lib, ctx, cfg, proofs, n, args.rounds) for n in SIZES]
        finally:
            ctx.close()
        doc["configs"].append({"n_queries": n_queries, "proof_bytes": len(proofs[0]), "sizes": rows})
        for r in rows:
            print(json.dumps({"n_queries": n_queries, "n": r["n"],
                              "verify_many_proofs_per_s": round(r["verify_many"]["proofs_per_s"]["median"]),
                              "host_loop_proofs_per_s": round(r["host_loop"]["proofs_per_s"]["median"]),
                              "verify_many_cpu_us": round(r["verify_many"]["host_cpu_us_per_proof"]["median"], 1),
                              "host_loop_cpu_us": round(r["host_loop"]["host_cpu_us_per_proof"]["median"], 1),
                              "launches": r["launches_per_call"], "waits": r["host_waits_per_call"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
