#!/usr/bin/env python3
"""What `lmn_tree_decommit` / `lmn_col_gather` are worth to a prover built on the level-2 handles: the time to open a
committed tree at the drawn queries, one MI355X, one context per child process, the two forms alternating.

  a  what such a prover had to do before: every committed column through `lmn_col_to_cpu`, every layer through
     `lmn_tree_layer_to_cpu`, then the walk on the host copies (the oracle's `MerkleTree.decommit`)
  b  `lmn_tree_decommit`: the walk plans on the host, one launch gathers, one transfer brings the opening back

for a tree of BASELINE config 2a's trace-tree size with a second size in it (15 columns of 2^21 rows + 4 of 2^20) and for
a 2^16-row tree of the same shape; and `lmn_col_gather` of 1 000 positions against the whole-column download of a
2^21-row secure column.  Both forms must return the same opening.  Each case runs in a child process with a time limit;
the parent prints one JSON line and, with --out, writes it to a file (profiles/level2_decommit.json).  Bytes over the
link are counted from the call's arguments and results; launches per call is the number the code makes (one
`k_tree_decommit` / `k_col_gather`, level2.cpp), not a measurement."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from luminair_amd import backend                      # noqa: E402

P = (1 << 31) - 1
CASES = {"tree_2_21": (21, 600), "tree_2_16": (16, 300), "gather_2_21": (21, 300)}


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
            "samples": [round(x, 4) for x in v]}


def fold(positions, n):
    out = []
    for p in positions:
        if not out or out[-1] != p >> n:
            out.append(p >> n)
    return out


def tree_case(top, rounds, warmup):
    from oracle.merkle import MerkleTree
    lib = backend.default_library()
    ctx = backend.Context(0, None, lib)
    L = lib.lib
    rng = np.random.default_rng(top)
    shape = [(15, top), (4, top - 1)]
    host = [rng.integers(0, P, size=(nc, 1 << lg), dtype=np.uint64).astype(np.uint32) for nc, lg in shape]
    handles = [ctx.col_from_cpu(a) for a in host]
    tree = ctx.commit(handles)
    drawn = sorted({int(x) for x in rng.integers(0, 1 << top, size=ctx.config.n_queries)})
    queries = {top: drawn, top - 1: fold(drawn, 1)}
    col_bufs = [np.empty_like(a) for a in host]
    layer_bufs = [np.empty((1 << k, 8), dtype=np.uint32) for k in range(top + 1)]

    def form_a():
        t0 = time.perf_counter()
        for h, buf in zip(handles, col_bufs):
            ctx._check(L.lmn_col_to_cpu(ctx.handle, h.handle, buf.ctypes.data))
        for k, buf in enumerate(layer_bufs):
            ctx._check(L.lmn_tree_layer_to_cpu(ctx.handle, tree.handle, k, buf.ctypes.data))
        t1 = time.perf_counter()
        mt = object.__new__(MerkleTree)             # the walk alone: the tree is the device's, not rebuilt
        mt.sorted_columns = [c for buf in col_bufs for c in buf]
        mt.layers = layer_bufs
        v, h, w = mt.decommit(queries)
        t2 = time.perf_counter()
        return (t2 - t0, t1 - t0), (v, h, w)

    def form_b():
        t0 = time.perf_counter()
        v, h, w = tree.decommit(handles, queries)
        return (time.perf_counter() - t0, 0.0), (v.tolist(), h, w.tolist())

    a_ms, a_dl_ms, b_ms = [], [], []
    opening = None
    for r in range(warmup + rounds):
        (ta, tdl), oa = form_a()
        (tb, _), ob = form_b()
        assert oa == ob, "the two forms disagree"
        opening = ob
        if r >= warmup:
            a_ms.append(ta * 1e3)
            a_dl_ms.append(tdl * 1e3)
            b_ms.append(tb * 1e3)
    nv, nh, nw = len(opening[0]), len(opening[1]), len(opening[2])
    n_ptrs = top + 1 + sum(nc for nc, _ in shape)
    res = {"log_size": top, "columns": shape, "n_queries": len(drawn), "unit": "ms",
           "a_download_all_then_host_walk": stats(a_ms), "a_of_which_downloads": stats(a_dl_ms), "b_lmn_tree_decommit": stats(b_ms),
           "a_bytes_to_host": int(sum(a.nbytes for a in host) + sum(b.nbytes for b in layer_bufs)), "a_bytes_to_device": 0,
           "b_bytes_to_host": 4 * nv + 32 * nh + 4 * nw, "b_bytes_to_device": 8 * n_ptrs + 8 * (nv + nh + nw),
           "b_outputs": {"queried_values": nv, "hashes": nh, "column_witness_words": nw},
           "b_launches_per_call": 1, "b_transfers_to_host_per_call": 1}
    tree.free()
    for h in handles:
        h.free()
    ctx.close()
    return res


def gather_case(top, rounds, warmup):
    lib = backend.default_library()
    ctx = backend.Context(0, None, lib)
    rng = np.random.default_rng(top + 100)
    host = rng.integers(0, P, size=(4, 1 << top), dtype=np.uint64).astype(np.uint32)
    h = ctx.col_from_cpu(host)
    pos = rng.integers(0, 1 << top, size=1000).astype(np.uint32)
    buf = np.empty_like(host)
    a_ms, b_ms = [], []
    for r in range(warmup + rounds):
        t0 = time.perf_counter()
        ctx._check(lib.lib.lmn_col_to_cpu(ctx.handle, h.handle, buf.ctypes.data))
        want = buf[:, pos]
        t1 = time.perf_counter()
        got = h.gather(pos)
        t2 = time.perf_counter()
        assert np.array_equal(got, want)
        if r >= warmup:
            a_ms.append((t1 - t0) * 1e3)
            b_ms.append((t2 - t1) * 1e3)
    res = {"log_size": top, "columns": 4, "positions": len(pos), "unit": "ms", "a_whole_column_download": stats(a_ms),
           "b_lmn_col_gather": stats(b_ms), "a_bytes_to_host": int(host.nbytes), "b_bytes_to_host": int(4 * 4 * len(pos)),
           "b_bytes_to_device": int(4 * len(pos)), "b_launches_per_call": 1, "b_transfers_to_host_per_call": 1}
    h.free()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    ap.add_argument("--child", choices=sorted(CASES))
    args = ap.parse_args()
    if args.child:
        top = CASES[args.child][0]
        fn = gather_case if args.child.startswith("gather") else tree_case
        print("RESULT " + json.dumps(fn(top, args.rounds, args.warmup)))
        return 0
    result = {"tool": "level2_decommit_latency", "rounds": args.rounds, "warmup": args.warmup}
    for name, (_, seconds) in CASES.items():     # a case that fails or runs out of time ends the run: nothing is tried twice
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--rounds", str(args.rounds),
                            "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=seconds)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write("%s failed (%d)\n%s\n" % (name, r.returncode, r.stderr[-4000:]))
            return 1
        result[name] = json.loads(lines[-1][7:])
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
