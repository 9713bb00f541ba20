#!/usr/bin/env python3
"""What the FRI close on the device is worth ("Proof of work"; results in profiles/fri_close_latency.json).

BASELINE config 2a (one Add table of 2^20 rows), n_queries 70, pow_bits {16, 20, 24}: solo latency (median of --solo-reps
proofs, default 5) and proofs/s with 24 in flight, in alternating runs of
  this-device  this tree under LMN_DEVICE_FRI_CLOSE=1: the transcript is closed on the device, two host waits per proof
  this         this tree, default switches: the host close, three waits
  parent       with --parent-tree DIR, a built checkout of the commit to compare with
each run in a process of its own (the trees' packages bind different symbol lists).  The proofs of all must be the same
bytes.  --bench adds the default bench command (bench.py --gpus 1 --steps 20 --warmup 5) of this tree and the parent's,
alternating as well: its launch sequence does not change, so the two must lie within each other's spread.

Usage: fri_close_latency.py [--parent-tree DIR] [--alternations N] [--solo-reps N] [--bench] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POW_BITS = [16, 20, 24]
IN_FLIGHT, N_PROOFS, SOLO_REPS = 24, 48, 5


def worker(tree, solo_reps):
    """child process: the measurements of one run with the package and libraries of `tree`"""
    sys.path.insert(0, tree)
    import luminair_amd
    from luminair_amd import synthetic as syn
    pie = luminair_amd.LuminairPie.from_tables(syn.config2_add_only(1 << 20, 5))
    rows = []
    for pb in POW_BITS:
        row = dict(pow_bits=pb)
        solo = luminair_amd.ProverPool(0, 1, pow_bits=pb, n_queries=70)
        try:
            got = solo.prove_many([pie])                      # warm-up
            lat = []
            for _ in range(solo_reps):
                t = time.perf_counter()
                solo.prove_many([pie])
                lat.append(time.perf_counter() - t)
            row["solo_ms"] = [round(1e3 * x, 3) for x in lat]
            row["sha256"] = hashlib.sha256(got[0].to_bincode() if hasattr(got[0], "to_bincode") else bytes(got[0])).hexdigest()
        finally:
            solo.close()
        pool = luminair_amd.ProverPool(0, IN_FLIGHT, pow_bits=pb, n_queries=70)
        try:
            pool.prove_many([pie] * IN_FLIGHT)                # warm-up
            t = time.perf_counter()
            pool.prove_many([pie] * N_PROOFS)
            row["proofs_per_s"] = round(N_PROOFS / (time.perf_counter() - t), 1)
        finally:
            pool.close()
        rows.append(row)
    print("RESULT " + json.dumps(rows), flush=True)


def run_worker(tree, device_close, solo_reps):
    env = dict(os.environ)
    env.pop("LMN_DEVICE_FRI_CLOSE", None)
    if device_close:
        env["LMN_DEVICE_FRI_CLOSE"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tree, str(solo_reps)], capture_output=True,
                       text=True, env=env, cwd=tree)
    if r.returncode != 0:
        raise SystemExit("worker failed in %s:\n%s" % (tree, r.stderr[-3000:]))
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def run_bench(tree):
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                       capture_output=True, text=True, cwd=tree)
    if r.returncode != 0:
        raise SystemExit("bench failed in %s:\n%s" % (tree, r.stderr[-3000:]))
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return {k: line[k] for k in ("value", "unit", "ms_per_proof", "prove_latency_ms", "prove_latency_p95_ms")}


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--worker":
        return worker(sys.argv[2], int(sys.argv[3]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", help="a built checkout of the commit to compare with")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--solo-reps", type=int, default=SOLO_REPS)
    ap.add_argument("--bench", action="store_true", help="also alternate the default bench command of both trees")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri_close_latency.json"))
    a = ap.parse_args()
    runs = [("this-device", ROOT, True), ("this", ROOT, False)]
    if a.parent_tree:
        runs.append(("parent", os.path.abspath(a.parent_tree), False))
    res = dict(cpus_available=len(os.sched_getaffinity(0)), shape="config 2a: Add 2^20 rows, 70 queries", in_flight=IN_FLIGHT,
               proofs_timed=N_PROOFS, solo_reps=a.solo_reps, alternations=[])
    for alt in range(a.alternations):
        entry = {}
        for name, tree, device_close in runs:
            entry[name] = run_worker(tree, device_close, a.solo_reps)
            for row in entry[name]:
                row["solo_median_ms"] = round(statistics.median(row["solo_ms"]), 3)
            print(alt, name, json.dumps([(r["pow_bits"], r["solo_median_ms"], r["proofs_per_s"]) for r in entry[name]]), flush=True)
        for i, pb in enumerate(POW_BITS):
            assert len({entry[name][i]["sha256"] for name, _, _ in runs}) == 1, ("proof bytes differ", pb)
        res["alternations"].append(entry)
    summary = []
    for i, pb in enumerate(POW_BITS):
        row = dict(pow_bits=pb)
        for name, _, _ in runs:
            solo = [e[name][i]["solo_median_ms"] for e in res["alternations"]]
            tput = [e[name][i]["proofs_per_s"] for e in res["alternations"]]
            row[name] = dict(solo_ms=solo, solo_ms_median=round(statistics.median(solo), 3), proofs_per_s=tput,
                             proofs_per_s_median=round(statistics.median(tput), 1))
        summary.append(row)
        print(json.dumps(row), flush=True)
    res["summary"] = summary
    if a.bench:
        res["default_bench"] = []
        for alt in range(a.alternations):
            entry = {"this": run_bench(ROOT)}
            if a.parent_tree:
                entry["parent"] = run_bench(os.path.abspath(a.parent_tree))
            res["default_bench"].append(entry)
            print("bench", alt, json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
