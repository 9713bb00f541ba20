#!/usr/bin/env python3
"""What planning a proof's openings on the device is worth (results in
profiles/open_queries_latency.json).  BASELINE config 2a (one Add table of 2^20 rows), pow_bits 16, n_queries 3 and 70.
Every run goes in a process of its own under its own time limit; the order of the legs rotates from one alternation to the
next, so that no leg always runs first.

  proofs      solo latency (median of --reps proofs) and proofs/s with 24 in flight, in three legs:
                this-both    this tree under LMN_DEVICE_FRI_CLOSE=1 LMN_DEVICE_DECOMMIT=1: one host wait behind the quotients
                this-close   this tree under LMN_DEVICE_FRI_CLOSE=1 alone: host plan, gather, a second wait
                parent       with --parent-tree, a built checkout of the parent commit under LMN_DEVICE_FRI_CLOSE=1
              The proofs of all legs must be the same bytes.
  host-plan   the host's planning time inside `lmn_prove` - the LMN_HOST_PROFILE marks "pow+queries" -> "decommit planned"
              - under LMN_DEVICE_FRI_CLOSE=1 on the parent (on this tree without --parent-tree): a run of its own, because the
              marks print.
  openings    level 2, this tree: the 20 trees of such a proof (2^21-row query domain; 15-, 4-, 4- and 2-column trees, FRI
              layers 2^21 .. 2^6) opened with ONE `lmn_open_queries` call and with one `lmn_tree_decommit` per tree (groups
              expanded beforehand, FRI witness values not fetched); timed are the C calls alone.
  bench       with --bench, the default bench command (bench.py --gpus 1 --steps 20 --warmup 5) of this tree and the
              parent's: the default launch sequence does not change, so the two must lie within each other's spread.

Usage: open_queries_latency.py [--parent-tree DIR] [--alternations N] [--reps N] [--bench] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERIES = [3, 70]
TOP = 21
STEP_TIMEOUT = 240
IN_FLIGHT, N_PROOFS = 24, 48


def worker_openings(tree, reps):
    sys.path.insert(0, tree)
    import numpy as np
    from luminair_amd import backend
    ctx = backend.Context(0, None, backend.default_library())
    rng = np.random.default_rng(1)
    P = (1 << 31) - 1
    shapes = [[(15, TOP)], [(4, TOP)], [(4, TOP)], [(2, TOP - 1)]] + [[(4, lg)] for lg in range(TOP, 5, -1)]
    flags = [0, 0, 0, 0] + [backend.OPEN_FRI_PAIRS] * (TOP - 5)
    items = []
    for shape in shapes:
        handles = [ctx.col_from_cpu(rng.integers(0, P, size=(n, 1 << lg), dtype=np.uint64).astype(np.uint32)) for n, lg in shape]
        items.append((ctx.commit(handles), handles, [lg for _, lg in shape]))
    rows = []
    for nq in QUERIES:
        positions = sorted({int(x) for x in rng.integers(0, 1 << TOP, size=nq)})
        pos = ctx.positions_from_cpu(positions, TOP)
        groups = []
        for (tree_, handles, logs), fl in zip(items, flags):
            g = {}
            for lg in logs:
                folded = sorted({p >> (TOP - lg) for p in positions})
                g[lg] = sorted({q ^ b for q in folded for b in (0, 1)}) if fl else folded
            groups.append(g)
        call = [(t, h, fl) for (t, h, _), fl in zip(items, flags)]
        got = ctx.open_queries(pos, call)                        # warm-up, and the comparison
        for (t, h, _), g, o in zip(items, groups, got):
            vals, hw, cw = t.decommit(h, g)
            assert vals.tolist() == o.queried_values.tolist() and hw == o.hash_witness and cw.tolist() == o.column_witness.tolist()
        # timed: the C calls themselves, their arguments built beforehand and their results released unread
        import ctypes as C
        L = ctx.lib.lib
        c_items = (backend.LmnOpenItem * len(call))()
        arrs = []
        for k, (t, h, fl) in enumerate(call):
            arrs.append((C.c_void_p * len(h))(*[c.handle for c in h]))
            c_items[k] = backend.LmnOpenItem(t.handle, arrs[-1], len(h), fl)
        res = (backend.LmnOpening * len(call))()
        dec_args = []
        for k, g in enumerate(groups):
            logs = np.array(list(g), dtype=np.uint32)
            counts = np.array([len(q) for q in g.values()], dtype=np.uint32)
            flat = np.array([p for q in g.values() for p in q], dtype=np.uint32)
            dec_args.append((c_items[k].tree, arrs[k], len(arrs[k]), logs, counts, flat))
        one, many = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            rc = L.lmn_open_queries(ctx.handle, pos.handle, c_items, len(call), res)
            one.append(time.perf_counter() - t0)
            assert rc == 0
            for r in res:
                for name in ("queried_values", "hash_witness", "column_witness", "fri_witness"):
                    if getattr(r, name):
                        L.lmn_free(getattr(r, name))
            dt = 0.0
            for tree_h, arr, n_cols, logs, counts, flat in dec_args:
                v, hs, w = C.c_void_p(), C.c_void_p(), C.c_void_p()
                nv, nh, nw = C.c_size_t(), C.c_size_t(), C.c_size_t()
                t0 = time.perf_counter()
                rc = L.lmn_tree_decommit(ctx.handle, tree_h, arr, n_cols, logs.ctypes.data, counts.ctypes.data, len(logs),
                                         flat.ctypes.data, C.byref(v), C.byref(nv), C.byref(hs), C.byref(nh), C.byref(w), C.byref(nw))
                dt += time.perf_counter() - t0
                assert rc == 0
                for ptr in (v, hs, w):
                    if ptr.value:
                        L.lmn_free(ptr)
            many.append(dt)
        rows.append(dict(n_queries=nq, trees=len(items), open_queries_us=round(1e6 * statistics.median(one), 1),
                         tree_decommit_per_tree_us=round(1e6 * statistics.median(many), 1),
                         opened_hashes=sum(len(o.hash_witness) for o in got)))
        pos.free()
    print("RESULT " + json.dumps(rows), flush=True)


def worker_host_plan(tree, reps):
    sys.path.insert(0, tree)
    import luminair_amd
    from luminair_amd import synthetic as syn
    pie = luminair_amd.LuminairPie.from_tables(syn.config2_add_only(1 << 20, 5))
    rows = []
    for nq in QUERIES:
        pool = luminair_amd.ProverPool(0, 1, pow_bits=16, n_queries=nq)
        try:
            got = pool.prove_many([pie])                          # warm-up
            print("MARK begin %d" % nq, file=sys.stderr, flush=True)
            lat = []
            for _ in range(reps):
                t = time.perf_counter()
                pool.prove_many([pie])
                lat.append(time.perf_counter() - t)
            print("MARK end %d" % nq, file=sys.stderr, flush=True)
            rows.append(dict(n_queries=nq, solo_median_ms=round(1e3 * statistics.median(lat), 3),
                             sha256=hashlib.sha256(got[0].to_bincode() if hasattr(got[0], "to_bincode") else bytes(got[0])).hexdigest()))
        finally:
            pool.close()
        if os.environ.get("LMN_HOST_PROFILE"):
            continue                                               # (the marks print: no throughput figure from this run)
        pool = luminair_amd.ProverPool(0, IN_FLIGHT, pow_bits=16, n_queries=nq)
        try:
            pool.prove_many([pie] * IN_FLIGHT)                    # warm-up
            t = time.perf_counter()
            pool.prove_many([pie] * N_PROOFS)
            rows[-1]["proofs_per_s"] = round(N_PROOFS / (time.perf_counter() - t), 1)
        finally:
            pool.close()
    print("RESULT " + json.dumps(rows), flush=True)


def run_worker(kind, tree, reps, env_extra):
    env = dict(os.environ)
    for k in ("LMN_DEVICE_FRI_CLOSE", "LMN_DEVICE_DECOMMIT", "LMN_HOST_PROFILE"):
        env.pop(k, None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", kind, tree, str(reps)], capture_output=True,
                       text=True, env=env, cwd=tree, timeout=STEP_TIMEOUT)
    if r.returncode != 0:
        raise SystemExit("%s worker failed in %s:\n%s" % (kind, tree, r.stderr[-3000:]))
    rows = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    if kind == "host-plan":                                       # the marks between MARK begin / end, per query count
        at, plan = None, {}
        for ln in r.stderr.splitlines():
            m = re.match(r"MARK (begin|end) (\d+)", ln)
            if m:
                at = int(m.group(2)) if m.group(1) == "begin" else None
            m = re.match(r"\[host\] decommit planned\s+\+\s*([0-9.]+) us", ln)
            if m and at is not None:
                plan.setdefault(at, []).append(float(m.group(1)))
        for row in rows:
            us = plan.get(row["n_queries"], [])
            row["host_plan_us_median"] = round(statistics.median(us), 1) if us else None
            row["host_plan_samples"] = len(us)
    return rows


def run_bench(tree):
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                       capture_output=True, text=True, cwd=tree, timeout=STEP_TIMEOUT)
    if r.returncode != 0:
        raise SystemExit("bench failed in %s:\n%s" % (tree, r.stderr[-3000:]))
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return {k: line[k] for k in ("value", "unit", "ms_per_proof", "prove_latency_ms", "prove_latency_p95_ms")}


def main():
    if len(sys.argv) == 5 and sys.argv[1] == "--worker":
        return {"openings": worker_openings, "host-plan": worker_host_plan}[sys.argv[2]](sys.argv[3], int(sys.argv[4]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", help="a built checkout of the commit to compare with")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--bench", action="store_true", help="also alternate the default bench command of both trees")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "open_queries_latency.json"))
    a = ap.parse_args()
    parent = os.path.abspath(a.parent_tree) if a.parent_tree else None
    res = dict(cpus_available=len(os.sched_getaffinity(0)), shape="config 2a: Add 2^20 rows, pow_bits 16; query domain 2^21",
               reps=a.reps, alternations=[])

    def flush():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    close, both = {"LMN_DEVICE_FRI_CLOSE": "1"}, {"LMN_DEVICE_FRI_CLOSE": "1", "LMN_DEVICE_DECOMMIT": "1"}
    legs = [("this-both", ROOT, both), ("this-close", ROOT, close)] + ([("parent", parent, close)] if parent else [])
    for alt in range(a.alternations):
        entry = {}
        order = legs[alt % len(legs):] + legs[:alt % len(legs)]   # no leg always runs first
        entry["order"] = [name for name, _, _ in order]
        for name, tree, env in order:
            entry[name] = run_worker("host-plan", tree, a.reps, env)
        for i in range(len(QUERIES)):
            assert len({entry[name][i]["sha256"] for name, _, _ in legs}) == 1, ("proof bytes differ", QUERIES[i])
        entry["host_plan"] = run_worker("host-plan", parent or ROOT, a.reps, dict(close, LMN_HOST_PROFILE="1"))
        entry["openings"] = run_worker("openings", ROOT, a.reps, {})
        if a.bench:
            benches = [("bench_this", ROOT)] + ([("bench_parent", parent)] if parent else [])
            for name, tree in (benches if alt % 2 == 0 else benches[::-1]):
                entry[name] = run_bench(tree)
        res["alternations"].append(entry)
        print(alt, json.dumps(entry)[:1500], flush=True)
        flush()
    summary = {}
    for i, nq in enumerate(QUERIES):
        row = {}
        for name, _, _ in legs:
            solo = [e[name][i]["solo_median_ms"] for e in res["alternations"]]
            tput = [e[name][i]["proofs_per_s"] for e in res["alternations"]]
            row[name] = dict(solo_ms=solo, solo_ms_median=round(statistics.median(solo), 3), proofs_per_s=tput,
                             proofs_per_s_median=round(statistics.median(tput), 1))
        plan = [e["host_plan"][i]["host_plan_us_median"] for e in res["alternations"] if e["host_plan"][i]["host_plan_us_median"] is not None]
        row["host_plan_us"] = plan
        for key in ("open_queries_us", "tree_decommit_per_tree_us"):
            row[key] = round(statistics.median(e["openings"][i][key] for e in res["alternations"]), 1)
        summary["n_queries %d" % nq] = row
    if a.bench:
        for leg in ("bench_this", "bench_parent"):
            xs = [e[leg]["value"] for e in res["alternations"] if leg in e]
            if xs:
                summary[leg] = dict(values=xs, median=statistics.median(xs), unit=res["alternations"][0][leg]["unit"])
    res["summary"] = summary
    print(json.dumps(summary), flush=True)
    flush()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
