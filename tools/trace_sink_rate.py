#!/usr/bin/env python3
"""What filling row sinks from the device producers is worth: `DeviceGraph.gen_trace(columns=True)` (the producers write
column-major sink tables, `lmn_rows_append_*`, and the proof starts without `k_transpose_pad`) against `gen_trace()` (row
tables, transposed by the proof's first launch), on one MI355X.

Workloads: `add20` - a 2^20-element Add graph (two inputs, one add); `mulsum18` - a 2^18-element Mul + SumReduce graph.

Every measurement is one child process (`... run`); the orchestrator (no sub-command) runs, for each workload and each of
solo / 8 in flight / 24 in flight, a warm-up process of each form and then the two forms alternating `--rounds` times, and
lists every run in the JSON it writes (`--out`, profiles/trace_sink_rate.json):

  solo      latency from the first producer call to the proof bytes (median and every sample), one context
  in flight pies per second with N pies in flight, each on its own context (one thread per context) with reused sinks and
            slabs; waiting calls per pie as the binding makes them

With `--profile` it also takes, in runs of their own, `rocprofv3 --kernel-trace --stats` (the producers' kernel durations and
the `k_transpose_pad` time of each form) and `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` (HBM bytes per pie; no tracing
is combined with the counters).  The tool stops at the first child that does not end cleanly."""
import argparse
import csv
import glob
import json
import os
import sqlite3
import statistics
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = ("add20", "mulsum18")


def build_graph(ctx, workload, seed):
    from luminair_amd.graph import DeviceGraph
    rng = np.random.default_rng(seed)
    g = DeviceGraph(ctx)
    if workload == "add20":
        n = 1 << 20
        x, y = g.input(rng.integers(-(1 << 20), 1 << 20, size=n)), g.input(rng.integers(-(1 << 20), 1 << 20, size=n))
        g.output(g.add(x, y))
    elif workload == "mulsum18":
        shape = (1 << 9, 1 << 9)                      # 2^18 elements, 2^9 groups of 2^9
        x, y = g.input(rng.integers(-4096, 4097, size=shape)), g.input(rng.integers(-4096, 4097, size=shape))
        g.output(g.sum_reduce(g.mul(x, y), axis=1))
    else:
        raise SystemExit("unknown workload %r" % workload)
    return g


class Pies:
    """one context's stream of pies: gen_trace, prove, give the slab back, keep the sinks"""

    def __init__(self, lib, workload, columns, seed):
        from luminair_amd import backend
        cfg = lib.default_config()
        cfg.protocol_variant = backend.VARIANT_PINNED           # the variant in which the Inputs component exists
        self.ctx = backend.Context(0, cfg, lib)
        self.g = build_graph(self.ctx, workload, seed)
        self.columns, self.sinks, self.waiting_calls = columns, None, None

    def one(self):
        t0 = time.perf_counter()
        if self.columns:
            tables, luts, bufs = self.g.gen_trace(columns=True, sinks=self.sinks)
            self.sinks = self.g.sinks_of(bufs)
        else:
            tables, luts, bufs = self.g.gen_trace()
        proof = self.ctx.prove_tables(tables, luts)
        dt = time.perf_counter() - t0
        if self.waiting_calls is None:      # the staging upload, one finish per sink table, the proof
            self.waiting_calls = {"upload": 1, "rows_finish": len(self.sinks or {}), "prove": 1}
        for b in bufs:
            if not self.columns or b.__class__.__name__ != "_SinkLease":
                b.free()
        return dt, proof

    def close(self):
        for s in (self.sinks or {}).values():
            s.close()
        self.ctx.close()


def run_child(args):
    from luminair_amd import backend
    lib = backend.default_library()
    columns = bool(args.columns)
    workers = [Pies(lib, args.workload, columns, 100 + i) for i in range(args.inflight)]
    proofs = [w.one()[1] for w in workers for _ in range(args.warmup)][-1:]   # every context warm
    res = {"workload": args.workload, "columns": columns, "inflight": args.inflight, "pies_per_context": args.pies,
           "proof_bytes": len(proofs[0]) if proofs else None, "waiting_calls_per_pie": workers[0].waiting_calls}
    if args.inflight == 1:
        lat = [workers[0].one()[0] for _ in range(args.pies)]
        res.update(latency_ms_median=1e3 * statistics.median(lat), latency_ms_min=1e3 * min(lat),
                   latency_ms=[round(1e3 * v, 4) for v in lat])
    else:
        start = threading.Barrier(args.inflight + 1)
        errors = []

        def loop(w):
            start.wait()
            try:
                for _ in range(args.pies):
                    w.one()
            except Exception as e:           # noqa: BLE001 - reported by the parent thread
                errors.append(repr(e))

        threads = [threading.Thread(target=loop, args=(w,)) for w in workers]
        for t in threads:
            t.start()
        start.wait()
        t0 = time.perf_counter()
        for t in threads:
            t.join()
        dt = time.perf_counter() - t0
        if errors:
            raise SystemExit("worker failed: %s" % errors[0])
        res.update(seconds=dt, pies=args.inflight * args.pies, pies_per_s=args.inflight * args.pies / dt)
    for w in workers:
        w.close()
    print("RESULT " + json.dumps(res), flush=True)


def child_cmd(workload, columns, inflight, pies, warmup):
    return [sys.executable, os.path.abspath(__file__), "run", "--workload", workload, "--columns", str(int(columns)),
            "--inflight", str(inflight), "--pies", str(pies), "--warmup", str(warmup)]


def run_process(cmd, limit):
    """one child under its own time limit; raises (and so ends the tool) unless it exits 0"""
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, cwd=ROOT)
    if p.returncode != 0:
        raise SystemExit("child ended with %d: %s\n%s" % (p.returncode, " ".join(cmd), (p.stdout + p.stderr)[-3000:]))
    for line in p.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    return None


def _short(name):
    return name.split("(")[0].split("<")[0].replace("void ", "").replace("lmn::", "")


def kernel_stats(out_dir):
    """{short kernel name: (calls, total ns)} of a rocprofv3 --kernel-trace --stats run, from its CSV files or - where the
    profiler wrote its database form instead - from the `kernels` view of that"""
    stats = {}

    def add(name, calls, ns):
        c, t = stats.get(_short(name), (0, 0))
        stats[_short(name)] = (c + calls, t + ns)

    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            add(r["Name"], int(r["Calls"]), int(r["TotalDurationNs"]))
    if not stats:
        for path in glob.glob(os.path.join(out_dir, "**", "*_results.db"), recursive=True):
            for name, calls, ns in sqlite3.connect(path).execute("select name, count(*), sum(duration) from kernels group by name"):
                add(name, int(calls), int(ns))
    return stats


def counter_sum(out_dir, counter):
    total, rows = 0.0, 0
    for path in glob.glob(os.path.join(out_dir, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if r["Counter_Name"] == counter:
                total += float(r["Counter_Value"])
                rows += 1
    if not rows:
        for path in glob.glob(os.path.join(out_dir, "**", "*_results.db"), recursive=True):
            for v, k in sqlite3.connect(path).execute("select sum(value), count(*) from counters_collection where counter_name = ?",
                                                      (counter,)):
                total, rows = total + float(v or 0.0), rows + int(k)
    return total, rows


PRODUCERS = ("k_trace_elementwise", "k_trace_reduce", "k_trace_lut", "k_sink_")   # row forms, column forms


def profile(workload, columns, scratch, pies=6, warmup=2, parse_only=False):
    """kernel durations and HBM bytes per pie of one form, solo: three runs of their own"""
    tag = "%s_%s" % (workload, "cols" if columns else "rows")
    n = pies + warmup
    out = {"workload": workload, "columns": columns, "pies_in_run": n}
    d = os.path.join(scratch, tag + "_trace")
    if not parse_only:
        run_process(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] +
                    child_cmd(workload, columns, 1, pies, warmup), 400)
    st = kernel_stats(d)
    prod = {k: v for k, v in st.items() if k.startswith(PRODUCERS)}
    out["producer_kernels_us_per_pie"] = {k: round(t / 1e3 / n, 2) for k, (c, t) in sorted(prod.items())}
    out["producers_us_per_pie"] = round(sum(t for _, t in prod.values()) / 1e3 / n, 2)
    tp = [v for k, v in st.items() if k.startswith("k_transpose_pad")]
    out["transpose_pad_launches_per_pie"] = sum(c for c, _ in tp) / n
    out["transpose_pad_us_per_pie"] = round(sum(t for _, t in tp) / 1e3 / n, 2)
    out["rows_chunk_us_per_pie"] = round(sum(t for k, (c, t) in st.items() if k.startswith("k_rows_chunk")) / 1e3 / n, 2)
    out["all_kernels_us_per_pie"] = round(sum(t for _, t in st.values()) / 1e3 / n, 2)
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):                 # counters in a run of their own, nothing traced beside them
        d = os.path.join(scratch, "%s_%s" % (tag, counter.lower()))
        if not parse_only:
            run_process(["rocprofv3", "--pmc", counter, "--output-format", "csv", "-d", d, "--"] +
                        child_cmd(workload, columns, 1, pies, warmup), 400)
        total, rows = counter_sum(d, counter)
        out[counter.lower() + "_kib_per_pie_raw"] = round(total / n, 1) if rows else None
    if out["fetch_size_kib_per_pie_raw"] is not None and out["write_size_kib_per_pie_raw"] is not None:
        # MI355X: FETCH_SIZE reports half the bytes of wide coalesced reads (tools/pmc_summary.py)
        out["hbm_mb_per_pie_corrected"] = round((2 * out["fetch_size_kib_per_pie_raw"] + out["write_size_kib_per_pie_raw"])
                                                * 1024 / 1e6, 1)
    return out


def orchestrate(args):
    result = {"tool": "tools/trace_sink_rate.py", "rounds": args.rounds, "note": "one process per run; per workload and mode a "
              "warm-up run of each form, then rows / columns alternating; every run is listed", "runs": [], "summary": {}}
    modes = [("solo", 1, args.solo_pies), ("inflight8", 8, args.pies), ("inflight24", 24, args.pies)]
    if args.parse_profiles:          # the timed runs were made before: keep them, add the profiles
        modes = []
        if args.out and os.path.exists(args.out):
            result = json.load(open(args.out))
    for workload in args.workloads:
        for mode, inflight, pies in modes:
            for columns in (False, True):
                r = run_process(child_cmd(workload, columns, inflight, max(2, pies // 4), 2), 400)
                r.update(mode=mode, warmup_run=True)
                result["runs"].append(r)
            per_form = {False: [], True: []}
            for _ in range(args.rounds):
                for columns in (False, True):
                    r = run_process(child_cmd(workload, columns, inflight, pies, 2), 400)
                    r.update(mode=mode, warmup_run=False)
                    result["runs"].append(r)
                    per_form[columns].append(r["latency_ms_median"] if inflight == 1 else r["pies_per_s"])
            key = "latency_ms_median" if inflight == 1 else "pies_per_s"
            rows_v, cols_v = per_form[False], per_form[True]
            result["summary"]["%s/%s" % (workload, mode)] = {
                "figure": key, "rows": rows_v, "columns": cols_v,
                "rows_median": statistics.median(rows_v), "columns_median": statistics.median(cols_v),
                "columns_over_rows": statistics.median(cols_v) / statistics.median(rows_v),
                "rows_spread": (max(rows_v) - min(rows_v)) / statistics.median(rows_v),
                "columns_spread": (max(cols_v) - min(cols_v)) / statistics.median(cols_v)}
            print(workload, mode, json.dumps(result["summary"]["%s/%s" % (workload, mode)]), flush=True)
            if args.out:
                json.dump(result, open(args.out, "w"), indent=1)
    if args.profile or args.parse_profiles:
        result["profiles"] = []
        for workload in args.workloads:
            for columns in (False, True):
                result["profiles"].append(profile(workload, columns, args.scratch, parse_only=args.parse_profiles))
                print(json.dumps(result["profiles"][-1]), flush=True)
                if args.out:
                    json.dump(result, open(args.out, "w"), indent=1)
    if args.out:
        json.dump(result, open(args.out, "w"), indent=1)
    print(json.dumps(result["summary"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd")
    run = sub.add_parser("run")
    run.add_argument("--workload", choices=WORKLOADS, required=True)
    run.add_argument("--columns", type=int, required=True)
    run.add_argument("--inflight", type=int, default=1)
    run.add_argument("--pies", type=int, default=20)
    run.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=WORKLOADS)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pies", type=int, default=12, help="pies per context of an in-flight run")
    ap.add_argument("--solo-pies", type=int, default=40)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--parse-profiles", action="store_true",
                    help="read the rocprofv3 output an earlier --profile run left in --scratch and add it to --out; runs nothing")
    ap.add_argument("--scratch", default=os.path.join(ROOT, "build", "trace_sink_prof"),
                    help="where the rocprofv3 runs write (build/ is ignored by git)")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.cmd == "run":
        run_child(args)
    else:
        orchestrate(args)


if __name__ == "__main__":
    main()
