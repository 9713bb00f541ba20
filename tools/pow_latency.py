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
"""
import argparse
import hashlib
import json
import os
import statistics
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pow_latency.json"))
    ap.add_argument("--quick", action="store_true", help="fewer digests and proofs")
    a = ap.parse_args()
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
