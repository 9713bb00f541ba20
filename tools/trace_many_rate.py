#!/usr/bin/env python3
"""What the trace producers cost in front of a lock-step batch, one pie at a time against one launch per node.

Two graphs - the 3-node 32x32 Add graph (the reference's benchmark shape) and the 32-node tanh MLP 2-64-64-1 (BASELINE
config 4) - at 1, 16, 64 and 192 members.  Per (graph, members), in one process on one box:

  loop   `DeviceGraph.gen_trace` once per member - what the library offered before `lmn_trace_many_*` - ended by one
         4-byte download as the wait.  Each member's slab goes back to the context's cache before the next member, so no
         run of the loop pays an allocation: the figure is launches and staging only, which favours the loop.
  many   `DeviceGraph.gen_trace_many`, from its first producer call to the download of the refused counters.

The two forms alternate, three rounds each after one warm-up of each, and every run is reported.  Then the time of one
`BatchProver.prove_batch` of the same members, fed from the device-resident tables `gen_trace_many` left (one warm-up, three
runs): the producers' share of a batch before and after.

  trace_many_rate.py --out profiles/trace_many_rate.json      every (graph, members) in a child process of its own under
                                                              its own time limit; stops at the first failure
  trace_many_rate.py --one GRAPH MEMBERS                      one measurement, one JSON line

Acceptance (written into the file, nothing is tuned to it): at 64 and 192 members the many form's slowest run is faster
than the loop's fastest run, for both graphs."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

GRAPHS = ("add32", "mlp64")
MEMBERS = (1, 16, 64, 192)
ROUNDS = 3
CHILD_LIMIT_S = 240


def build_graph(name, ctx, n_members, seed=5):
    """(graph for gen_trace_many, feeds, per-member graphs for the loop)"""
    from luminair_amd.graph import DeviceGraph
    from trace_many_checks import mlp_graph
    rng = np.random.default_rng(seed)
    if name == "add32":
        a = rng.integers(-(1 << 20), 1 << 20, size=(n_members, 32, 32))
        b = rng.integers(-(1 << 20), 1 << 20, size=(n_members, 32, 32))

        def make(m, per_member):
            g = DeviceGraph(ctx)
            ta, tb = g.input(a[m], per_member=per_member), g.input(b[m], per_member=per_member)
            g.output(g.add(ta, tb))
            return g, {ta: a, tb: b}
    else:
        x = rng.integers(-2048, 2048, size=(n_members, 2))

        def make(m, per_member):
            g, x_in, _, _ = mlp_graph(ctx, x[m], widths=(2, 64, 64, 1), per_member=per_member)
            return g, {x_in: x}
    many, feeds = make(0, True)
    return many, feeds, [make(m, False)[0] for m in range(n_members)]


def measure(name, n_members):
    from luminair_amd import backend
    from luminair_amd.batch import BATCH_LIB, BatchProver
    lib = backend.Library(BATCH_LIB)          # one library produces and proves
    cfg = lib.default_config()
    cfg.protocol_variant = backend.VARIANT_PINNED
    ctx = backend.Context(0, cfg, lib)
    many, feeds, singles = build_graph(name, ctx, n_members)

    def run_loop():
        t0 = time.perf_counter()
        last = None
        for g in singles:
            if last is not None:
                last.free()                   # back to the context's one-slot cache: the next lease allocates nothing
            tables, _, bufs = g.gen_trace()
            last = bufs[0]
        ctx.download(tables[0][1].view(0, 4))
        dt = time.perf_counter() - t0
        last.free()
        return dt * 1e3

    def run_many(keep=False):
        t0 = time.perf_counter()
        pies, luts, bufs, refused = many.gen_trace_many(n_members, feeds)
        dt = time.perf_counter() - t0
        assert refused == [0] * n_members, refused
        if keep:
            return dt * 1e3, pies, luts, bufs
        for b in bufs:
            b.free()
        return dt * 1e3

    run_loop()
    run_many()
    loop_ms, many_ms = [], []
    for _ in range(ROUNDS):
        loop_ms.append(run_loop())
        many_ms.append(run_many())
    _, pies, luts, bufs = run_many(keep=True)
    bp = BatchProver(0, n_members, protocol_variant=backend.VARIANT_PINNED)
    marshalled = bp.marshal(pies, luts)
    proofs = bp.prove_batch(marshalled)
    assert all(proofs)
    lib.verify(proofs[-1], backend.VARIANT_PINNED)
    prove_ms = []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        bp.prove_batch(marshalled)
        prove_ms.append((time.perf_counter() - t0) * 1e3)
    bp.close()
    for b in bufs:
        b.free()
    ctx.close()
    return {"graph": name, "members": n_members, "nodes": len(many.nodes), "producer_calls_loop": len(many.nodes) * n_members,
            "producer_calls_many": len(many.nodes), "loop_ms": [round(v, 3) for v in loop_ms],
            "many_ms": [round(v, 3) for v in many_ms], "prove_batch_ms": [round(v, 3) for v in prove_ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=2, metavar=("GRAPH", "MEMBERS"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_many_rate.json"))
    ap.add_argument("--graphs", default=",".join(GRAPHS))
    ap.add_argument("--members", default=",".join(str(m) for m in MEMBERS))
    args = ap.parse_args()
    if args.one:
        print(json.dumps(measure(args.one[0], int(args.one[1]))), flush=True)
        return 0
    results = []
    for name in args.graphs.split(","):
        for m in (int(v) for v in args.members.split(",")):
            r = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--one",
                                name, str(m)], capture_output=True, text=True)
            if r.returncode != 0:
                print("%s x %d failed (exit %d): %s" % (name, m, r.returncode, r.stderr[-2000:]), flush=True)
                return 1                      # nothing more is started on the GPU after a failure
            results.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(json.dumps(results[-1]), flush=True)
    accept = {"%s x %d" % (r["graph"], r["members"]): max(r["many_ms"]) < min(r["loop_ms"])
              for r in results if r["members"] >= 64}
    doc = {"what": "wall ms from the first producer call to the end-of-graph download; loop = gen_trace per member (slab "
                   "reused, no allocation), many = gen_trace_many; prove_batch_ms = one BatchProver.prove_batch of the same "
                   "members on the device-resident tables; every run listed in order",
           "rounds": ROUNDS, "results": results, "many_slowest_beats_loop_fastest_at_64_and_192": accept}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
