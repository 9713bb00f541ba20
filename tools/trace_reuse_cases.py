#!/usr/bin/env python3
"""Trace reuse (LMN_TRACE_REUSE, docs/HISTORY.md "Trace reuse") measured where the benchmark cannot: bench.py proves the same
buffers again and again, this tool alternates TWO pies on every context - resident rows, 24 contexts, one driver thread per
context and the counting of bench.py's throughput().

  --case honest  two pies of one graph whose lhs, rhs and out differ (one model, two inputs): the graph's 12 of 15 columns
                 are skipped in every proof, the value columns never are - the rate should be the benchmark's
  --case cost    two valid graphs of one shape (other ids, indices and multiplicities): every candidate column differs every
                 time - what a context that never sees a graph twice pays; compare with --reuse 0.  The library backs off
                 after two such proofs (docs/SWITCHES.md), so the timed proofs show the back-off at work: none is compared
  --case same    one pie, as bench.py

Prints one JSON line: proofs/s, and per proof the candidate columns compared and skipped (lmn_ctx_counter 20 / 21)."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("honest", "cost", "same"), default="honest")
    ap.add_argument("--reuse", type=int, default=1, help="LMN_TRACE_REUSE for this process")
    ap.add_argument("--log-rows", type=int, default=20)
    ap.add_argument("--inflight", type=int, default=24)
    ap.add_argument("--steps", type=int, default=20, help="timed proofs per context")
    ap.add_argument("--warmup", type=int, default=4, help="untimed proofs per context")
    args = ap.parse_args()
    os.environ["LMN_TRACE_REUSE"] = str(args.reuse)
    from luminair_amd import backend, synthetic as syn
    lib = backend.default_library()
    n = 1 << args.log_rows
    rng = np.random.default_rng(1)
    lhs, rhs = rng.integers(-2048, 2048, size=(2, n))
    first = syn.add_rows(lhs, rhs)
    if args.case == "honest":
        lhs2, rhs2 = rng.integers(-2048, 2048, size=(2, n))
        second = syn.add_rows(lhs2, rhs2)
    elif args.case == "cost":
        # another graph of the same shape whose rows satisfy the AIR as well, so that both pies are proved to the end: other
        # node ids and consumer counts, indices that start at 1, and is_last the other way round (the transitions are
        # statements about one row: next_idx = idx + 1 wherever is_last is 0).  All 12 graph columns differ.
        second = syn.add_rows(lhs, rhs, node=5, lhs_id=3, rhs_id=4, mults=(2, 3, 4))
        second[:, 3] = (second[:, 3] + 1) % syn.P
        second[:, 4] ^= 1
        second[:, 8] = (second[:, 8] + 1) % syn.P
        assert all(not np.array_equal(first[:, c], second[:, c]) for c in (0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 14))
    else:
        second = first
    ctxs = [backend.Context(0, lib.default_config(), lib) for _ in range(args.inflight)]
    bufs = [[[(0, c.upload(rows), n)] for rows in (first, second)] for c in ctxs]
    start = threading.Barrier(args.inflight + 1)
    errors = []
    c0 = [(0, 0)] * args.inflight

    def prove(i, k):
        ctxs[i].prove_tables(bufs[i][k & 1])       # (both pies are valid: an error ends the run)

    def drive(i):
        try:
            for k in range(args.warmup):
                prove(i, k)
            c0[i] = (ctxs[i].counter(20), ctxs[i].counter(21))
            start.wait()
            for k in range(args.warmup, args.warmup + args.steps):
                prove(i, k)
        except BaseException as e:  # noqa: BLE001 - reported below
            errors.append(e)
            start.abort()

    threads = [threading.Thread(target=drive, args=(i,)) for i in range(args.inflight)]
    for t in threads:
        t.start()
    try:
        start.wait()
    except threading.BrokenBarrierError:
        pass
    t0 = time.perf_counter()
    for t in threads:
        t.join()
    dt = time.perf_counter() - t0
    if errors:
        raise errors[0]
    proofs = args.steps * args.inflight
    compared = sum(c.counter(20) - a for c, (a, _) in zip(ctxs, c0))
    skipped = sum(c.counter(21) - b for c, (_, b) in zip(ctxs, c0))
    print(json.dumps({"case": args.case, "LMN_TRACE_REUSE": args.reuse, "log_rows": args.log_rows, "inflight": args.inflight,
                      "proofs": proofs, "value": proofs / dt, "unit": "proofs/s",
                      "columns_compared_per_proof": compared / proofs, "columns_skipped_per_proof": skipped / proofs}))


if __name__ == "__main__":
    main()
