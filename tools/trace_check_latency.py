#!/usr/bin/env python3
"""What `lmn_trace_check` costs next to `lmn_prove` of the same pie: BASELINE config 2a (2^20 Add rows) resident in HBM and
as host rows, both calls on the same build in the same session, alternating, after a warm-up of each.  Writes
profiles/trace_check_latency.json (median and minimum wall time per call, milliseconds).

    python tools/trace_check_latency.py [--reps 10] [--log-rows 20] [--out profiles/trace_check_latency.json]

`--lut-rows N` adds a LUT pie (Sin / Exp2 / Log2 on N rows each, LUT sets in the generic tuple tables) measured the same way:
the figure behind the choice of how the three LUT element sets are aggregated."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from luminair_amd import backend, synthetic as syn    # noqa: E402


def alternate(ctx, tables, luts, reps):
    check, prove = [], []
    ctx.check_trace(tables, luts)
    ctx.prove_tables(tables, luts)
    for _ in range(reps):
        t0 = time.perf_counter()
        rep = ctx.check_trace(tables, luts)
        t1 = time.perf_counter()
        ctx.prove_tables(tables, luts)
        t2 = time.perf_counter()
        assert rep.ok, rep.summary
        check.append((t1 - t0) * 1e3)
        prove.append((t2 - t1) * 1e3)
    f = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3)}   # noqa: E731
    return {"trace_check": f(check), "prove": f(prove),
            "check_over_prove": round(statistics.median(check) / statistics.median(prove), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--log-rows", type=int, default=20)
    ap.add_argument("--lut-rows", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "trace_check_latency.json"))
    args = ap.parse_args()
    lib = backend.default_library()
    cfg = lib.default_config()
    cfg.protocol_variant = backend.VARIANT_PINNED
    ctx = backend.Context(0, cfg, lib)
    tabs = syn.config2_add_only(1 << args.log_rows)
    out = {"pie": "config 2a: Add, 2^%d rows" % args.log_rows, "reps": args.reps}
    bufs = [ctx.upload(r) for _, r in tabs]
    out["resident"] = alternate(ctx, [(k, b, len(r)) for (k, r), b in zip(tabs, bufs)], None, args.reps)
    for b in bufs:
        b.free()
    out["host_rows"] = alternate(ctx, [(k, r, len(r)) for k, r in tabs], None, args.reps)
    if args.lut_rows:
        act, luts = syn.activation_graph(args.lut_rows)
        out["lut_pie"] = dict(alternate(ctx, [(k, r, len(r)) for k, r in act], luts, args.reps),
                              pie="activation_graph(%d): Sin, Exp2, Log2 and their lookup tables" % args.lut_rows)
    ctx.close()
    print(json.dumps(out))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
