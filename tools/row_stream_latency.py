#!/usr/bin/env python3
"""What a row sink is worth to a caller that produces its trace rows on the host: the time from "last row produced" to
proof bytes, BASELINE config 2a (one Add table of 2^20 rows, 60 MiB), one context, one process, the forms alternating.

  A  the yardstick: `lmn_prove` on plain host rows - the whole table is uploaded and transposed in front of the proof
  B  the producer pushes its rows in 16 equal chunks as it goes (`lmn_rows_push_pinned` / `lmn_rows_push`), then
     `lmn_rows_finish` + `lmn_prove`
  C  the floor: rows already resident in HBM (LMN_TABLE_ROWS_ON_DEVICE)

The producer is modelled as a host memcpy of each chunk into the buffer the prover is given, so A and B do the same host
work; A and B are measured with page-locked rows (`lmn_host_alloc`) and with pageable rows.  Prints one JSON line and, with
--out, writes it to a file (profiles/row_stream_latency.json)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from luminair_amd import backend, synthetic as syn   # noqa: E402

CHUNKS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    args = ap.parse_args()
    n = 1 << args.log_rows
    lib = backend.default_library()
    ctx = backend.Context(0, None, lib)
    kind, rows = syn.config2_add_only(n, 42)[0]
    src = np.ascontiguousarray(rows, dtype=np.uint32)
    pinned = lib.host_rows(src.shape)
    pageable = np.empty_like(src)
    dev = ctx.upload(src)
    sink = ctx.row_sink(kind, n)
    step = n // CHUNKS
    want = ctx.prove_tables([(kind, src, n)])

    def produce(buf, i):
        buf[i * step:(i + 1) * step] = src[i * step:(i + 1) * step]

    def form_a(buf):
        for i in range(CHUNKS):
            produce(buf, i)
        t0 = time.perf_counter()
        proof = ctx.prove_tables([(kind, buf, n)])
        return time.perf_counter() - t0, proof

    def form_b(buf, push):
        sink.reset()
        for i in range(CHUNKS):
            produce(buf, i)
            if i == CHUNKS - 1:
                t0 = time.perf_counter()           # the last row exists; what follows is what the caller waits for
            push(buf[i * step:(i + 1) * step])
        sink.finish()
        proof = ctx.prove_tables([(kind, sink, n)])
        return time.perf_counter() - t0, proof

    def form_c():
        t0 = time.perf_counter()
        proof = ctx.prove_tables([(kind, dev, n)])
        return time.perf_counter() - t0, proof

    forms = {
        "A_pinned": lambda: form_a(pinned.array),
        "B_pinned": lambda: form_b(pinned.array, sink.push_pinned),
        "A_pageable": lambda: form_a(pageable),
        "B_pageable": lambda: form_b(pageable, sink.push),
        "C_resident": form_c,
    }
    samples = {k: [] for k in forms}
    for r in range(args.warmup + args.rounds):
        for name, f in forms.items():
            dt, proof = f()
            assert proof == want, name
            if r >= args.warmup:
                samples[name].append(dt * 1e3)
    result = {"tool": "row_stream_latency", "rows": n, "chunks": CHUNKS, "rounds": args.rounds, "unit": "ms"}
    for name, v in samples.items():
        result[name] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
                        "samples": [round(x, 4) for x in v]}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sink.close()
    dev.free()
    pinned.free()
    ctx.close()


if __name__ == "__main__":
    main()
