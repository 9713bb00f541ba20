#!/usr/bin/env python3
"""Proof of work on the device against the host loop ("Proof of work"; results in profiles/).

1. Grind rate of `Context.grind` (k_pow_grind) at pow_bits 28 - 32 on seeded digests, all three forms: nonces examined
   (to the end of the window that held the answer) per second of wall time around the call - launches and waits
   included, so a lower bound on the kernel's rate - as a fraction of roofline.BLAKE2S_PEAK_GCOMP.
2. Crossover: `Context.grind` (device) against `Library.grind` (host loop) at pow_bits 4 - 14.
3. BASELINE config 2a (one Add table of 2^20 rows), n_queries 70: solo latency and proofs/s with 24 in flight at pow_bits
   {5, 10, 16, 20, 24, 26}, device path (LMN_POW_DEVICE_MIN_BITS=0) and host path (=41) alternating.  The host path's
   throughput is measured up to pow_bits 20 only (at 24 / 26 a host grind is seconds per proof).

Usage: pow_latency.py [--out FILE] [--quick]

--batch measures the lock-step batch library's grind instead (results in profiles/pow_batch_latency.json):

4. The reference's benchmark shape (32x32 Add, PINNED variant) in batches of 64 at pow_bits {5, 16, 20, 24}: seconds per
   batch and proofs/s, median over the batches of alternating runs of this tree's library and - with --parent-tree DIR, a
   built checkout of the commit to compare with - that tree's, each run in a process of its own (the two packages bind
   different symbol lists).  The proofs of both must be the same bytes.
5. `Context.grind_many` (k_grind_many) on 64 digests at pow_bits 20 against 64 calls of `Context.grind` (k_pow_grind), all
   three forms: seconds, and nonces/s counted as the sum of (nonce + 1) - the nonces a perfect search examines, the same
   numerator for both - next to each path's own count to the end of the window that held each answer (section 1's).
   --grind-lib LABEL=PATH repeats this section on another build of the main library (e.g. one with another
   POW_WINDOWS_PER_WAIT).

Usage: pow_latency.py --batch [--parent-tree DIR] [--grind-lib LABEL=PATH ...] [--out FILE] [--quick]
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
sys.path.insert(0, ROOT)
import luminair_amd                                      # noqa: E402
from luminair_amd import backend, roofline, synthetic as syn   # noqa: E402

FORMS = {"kat": backend.VARIANT_KAT, "hashed": 0x4, "prefixed": 0x10}
WINDOW_LOG = 24          # kernels.h POW_WINDOW_LOG (the default cap; LMN_POW_WINDOW_LOG changes it)


def _digest(i):
    return hashlib.sha256(b"pow latency digest %d" % i).digest()


def examined(nonce, pow_bits, window_log):
    w = 1 << min(window_log, max(11, pow_bits + 1))
    return (nonce // w + 1) * w


def grind_rate(ctx, bits, n_digests, window_log):
    out = []
    for form, v in FORMS.items():
        for pb in bits:
            n_tot, t_tot = 0, 0.0
            for i in range(n_digests):
                d = _digest(1000 * pb + i)
                t = time.perf_counter()
                nonce = ctx.grind(d, pb, v)
                t_tot += time.perf_counter() - t
                n_tot += examined(nonce, pb, window_log)
            g = n_tot / t_tot / 1e9
            out.append(dict(form=form, pow_bits=pb, digests=n_digests, nonces=n_tot, seconds=round(t_tot, 4),
                            gnonce_per_s=round(g, 2), fraction_of_peak=round(g / roofline.BLAKE2S_PEAK_GCOMP, 3)))
            print(json.dumps(out[-1]), flush=True)
    return out


def crossover(ctx, lib, bits, reps):
    out = []
    for pb in bits:
        dev, host = [], []
        for i in range(reps):
            d = _digest(50000 + 100 * pb + i)
            t = time.perf_counter()
            a = ctx.grind(d, pb, backend.VARIANT_KAT)
            dev.append(time.perf_counter() - t)
            t = time.perf_counter()
            b = lib.grind(d, pb, backend.VARIANT_KAT)
            host.append(time.perf_counter() - t)
            assert a == b, (pb, i, a, b)
        out.append(dict(pow_bits=pb, device_ms=round(1e3 * statistics.median(dev), 4),
                        host_ms=round(1e3 * statistics.median(host), 4)))
        print(json.dumps(out[-1]), flush=True)
    return out


def _pool(pow_bits, min_bits, n):
    os.environ["LMN_POW_DEVICE_MIN_BITS"] = str(min_bits)    # read when a context is created
    try:
        return luminair_amd.ProverPool(0, n, pow_bits=pow_bits, n_queries=70)
    finally:
        os.environ.pop("LMN_POW_DEVICE_MIN_BITS", None)


def proofs(pow_list, n_inflight, n_proofs, solo_reps):
    pie = luminair_amd.LuminairPie.from_tables(syn.config2_add_only(1 << 20, 5))
    out = []
    for pb in pow_list:
        for path, min_bits in (("device", 0), ("host", 41)):
            row = dict(pow_bits=pb, path=path)
            solo = _pool(pb, min_bits, 1)
            try:
                solo.prove_many([pie])                       # warm-up
                reps = solo_reps if (path == "device" or pb <= 20) else 2
                lat = []
                for _ in range(reps):
                    t = time.perf_counter()
                    solo.prove_many([pie])
                    lat.append(time.perf_counter() - t)
                row["solo_ms"] = round(1e3 * statistics.median(lat), 3)
                row["solo_reps"] = reps
            finally:
                solo.close()
            if path == "device" or pb <= 20:
                pool = _pool(pb, min_bits, n_inflight)
                try:
                    pool.prove_many([pie] * n_inflight)      # warm-up
                    t = time.perf_counter()
                    pool.prove_many([pie] * n_proofs)
                    row["proofs_per_s"] = round(n_proofs / (time.perf_counter() - t), 1)
                finally:
                    pool.close()
            else:
                row["proofs_per_s"] = None                   # not measured (seconds of host grinding per proof)
            out.append(row)
            print(json.dumps(row), flush=True)
    return out


def batch_worker(tree, pow_bits, n_batches, slots=64):
    """child process: `n_batches` timed batches of `slots` 32x32 Add pies with the package and libraries of `tree`"""
    sys.path.insert(0, tree)                  # ahead of this file's own tree
    for m in [m for m in sys.modules if m.split(".")[0] == "luminair_amd"]:
        del sys.modules[m]
    from luminair_amd import backend as be, synthetic as sy
    from luminair_amd.batch import BatchProver
    pies = [[(k, r, len(r)) for k, r in sy.config2_graph_faithful(1024, 100 + i)] for i in range(slots)]
    bp = BatchProver(0, slots, protocol_variant=be.VARIANT_PINNED, pow_bits=pow_bits)
    try:
        marshalled = bp.marshal(pies)
        got = bp.prove_batch(marshalled)          # warm-up: twiddles, code objects
        secs = []
        for _ in range(n_batches):
            t = time.perf_counter()
            bp.prove_batch(marshalled)
            secs.append(time.perf_counter() - t)
        c = bp.counters()
    finally:
        bp.close()
    print("RESULT " + json.dumps(dict(seconds=secs, sha256=hashlib.sha256(b"".join(got)).hexdigest(),
                                      grinds=c.get("grinds"), grind_rounds=c.get("grind_rounds"))), flush=True)


def batch_proofs(pow_list, parent_tree, n_batches, alternations, slots=64):
    trees = [("this", ROOT)] + ([("parent", os.path.abspath(parent_tree))] if parent_tree else [])
    out = []
    for pb in pow_list:
        runs = {name: [] for name, _ in trees}
        sha = {}
        rounds = {}
        for _ in range(alternations):
            for name, tree in trees:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--batch-worker", tree, str(pb), str(n_batches)],
                                   capture_output=True, text=True, check=True)
                res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
                runs[name] += res["seconds"]
                sha[name] = res["sha256"]
                rounds[name] = (res["grinds"], res["grind_rounds"])
        assert len(set(sha.values())) == 1, sha       # the same proofs from both libraries
        row = dict(pow_bits=pb, batch=slots, batches_each=n_batches * alternations)
        for name, _ in trees:
            med = statistics.median(runs[name])
            row[name] = dict(ms_per_batch=round(1e3 * med, 3), proofs_per_s=round(slots / med, 1),
                             min_ms=round(1e3 * min(runs[name]), 3), max_ms=round(1e3 * max(runs[name]), 3))
        row["grinds_and_rounds_so_far"] = rounds["this"]
        if parent_tree:
            row["parent_over_this"] = round(row["parent"]["ms_per_batch"] / row["this"]["ms_per_batch"], 2)
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def examined_many(nonces, pow_bits, window_log, windows_per_wait=8):
    """grind_many's rounds replayed on the host: nonces examined when every digest is counted to the end of the window that
    held its answer (the count `examined` makes for the solo path), and the rounds (= host waits)"""
    pending, base, total, rounds = list(nonces), 0, 0, 0
    while pending:
        lg = (len(pending) - 1).bit_length()
        w = 1 << max(11, min(pow_bits + 1, window_log - lg))
        end = base + windows_per_wait * w
        total += sum(min(end, (x // w + 1) * w) - base for x in pending)
        pending = [x for x in pending if x >= end]
        base, rounds = end, rounds + 1
    return total, rounds


def grind_many_rate(label, lib_path, pow_bits, n, reps):
    lib = backend.Library(lib_path) if lib_path else backend.default_library()
    ctx = backend.Context(0, lib.default_config(), lib)
    out = []
    try:
        for form, v in FORMS.items():
            ds = [_digest(7000 + i) for i in range(n)]
            want = ctx.grind_many(ds, pow_bits, v)                     # warm-up
            assert [ctx.grind(d, pow_bits, v) for d in ds[:4]] == want[:4]
            tm, ts = [], []
            for _ in range(reps):
                t = time.perf_counter()
                ctx.grind_many(ds, pow_bits, v)
                tm.append(time.perf_counter() - t)
                t = time.perf_counter()
                for d in ds:
                    ctx.grind(d, pow_bits, v)
                ts.append(time.perf_counter() - t)
            useful = sum(x + 1 for x in want)
            solo_examined = sum(examined(x, pow_bits, WINDOW_LOG) for x in want)
            many_examined, rounds = examined_many(want, pow_bits, WINDOW_LOG)
            m, s = statistics.median(tm), statistics.median(ts)
            out.append(dict(library=label, form=form, pow_bits=pow_bits, n=n, reps=reps, useful_nonces=useful,
                            grind_many_ms=round(1e3 * m, 4), n_grind_calls_ms=round(1e3 * s, 4),
                            grind_many_rounds=rounds,
                            grind_many_useful_gnonce_per_s=round(useful / m / 1e9, 2),
                            grind_many_examined_gnonce_per_s=round(many_examined / m / 1e9, 2),
                            n_grind_calls_useful_gnonce_per_s=round(useful / s / 1e9, 2),
                            n_grind_calls_examined_gnonce_per_s=round(solo_examined / s / 1e9, 2)))
            print(json.dumps(out[-1]), flush=True)
    finally:
        ctx.close()
    return out


def main_batch(a):
    res = dict(cpus_available=len(os.sched_getaffinity(0)))
    res["grind_many_vs_n_grind_calls"] = grind_many_rate("this", None, 20, 64, 5 if a.quick else 9)
    for spec in a.grind_lib or []:
        label, path = spec.split("=", 1)
        res["grind_many_vs_n_grind_calls"] += grind_many_rate(label, path, 20, 64, 5 if a.quick else 9)
    res["batch_of_64_32x32_add"] = batch_proofs([5, 16, 20, 24], a.parent_tree, 3, 2)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


def main():
    if len(sys.argv) == 5 and sys.argv[1] == "--batch-worker":
        return batch_worker(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer digests and proofs")
    ap.add_argument("--batch", action="store_true", help="the lock-step batch library's grind and grind_many (sections 4, 5)")
    ap.add_argument("--parent-tree", help="--batch: a built checkout of the commit to compare the batch library with")
    ap.add_argument("--grind-lib", action="append", help="--batch: LABEL=PATH of another main library for section 5")
    a = ap.parse_args()
    if a.batch:
        a.out = a.out or os.path.join(ROOT, "profiles", "pow_batch_latency.json")
        return main_batch(a)
    a.out = a.out or os.path.join(ROOT, "profiles", "pow_latency.json")
    lib = backend.default_library()
    ctx = backend.Context(0)
    ctx.grind(_digest(0), 8, 0)   # warm-up
    res = dict(window_log=WINDOW_LOG, peak_gcomp=roofline.BLAKE2S_PEAK_GCOMP)
    res["grind_rate"] = grind_rate(ctx, [28, 30, 32] if a.quick else [28, 29, 30, 31, 32], 2 if a.quick else 4, WINDOW_LOG)
    res["crossover"] = crossover(ctx, lib, list(range(4, 15)), 9)
    ctx.close()
    res["config2a"] = proofs([5, 10, 16, 20, 24, 26], 24, 48 if a.quick else 96, 5 if a.quick else 9)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
