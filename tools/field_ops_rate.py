#!/usr/bin/env python3
"""The rate of `lmn_col_batch_inverse` (M31, one column) and `lmn_col_batch_inverse_secure` (QM31) on one MI355X against
`lmn_device_copy` of the same bytes, and the sweep over E (elements per lane of k_batch_inverse_m / k_batch_inverse_q)
that the constants BATCH_INV_E_M31 / BATCH_INV_E_QM31 of kernels_trace.hip were chosen by.

Per size (2^20, 2^24, 2^26 rows) and form: warm up, enqueue K calls with n_zero_out == NULL, end with one
`lmn_col_to_cpu` of a 1-element handle as the wait; K doubles until a run lasts 50 ms; median of 5 runs.  The yardstick,
`lmn_device_copy` of the bytes the op reads (and so writes), runs in the same loop of the same process, alternating with
the op.  Reported: elements/s, GB/s by algorithmic bytes (8 per M31 element, 32 per QM31 element: read once, written
once) and the op's rate over the copy's.  The result at 2^20 rows is checked by the defining identity.

  field_ops_rate.py --build-sweep DIR     (needs hipcc, no GPU) copies csrc to DIR/<label>/ for every E pair, rewrites
                                          the two constants, builds libluminair_hip.so there and writes DIR/sweep.json
                                          with each build's registers and vector instructions per element
  field_ops_rate.py [--sweep DIR] --out profiles/field_ops_rate.json
                                          (needs the GPU) measures the in-tree library, and every library of the sweep;
                                          each library in a child process of its own

Nothing is gated: the op is new, there is no earlier figure."""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from luminair_amd import backend                      # noqa: E402

P = (1 << 31) - 1
LOGS = (20, 24, 26)
SWEEP = ((4, 2), (8, 4), (16, 8))                     # (E of the M31 kernel, E of the QM31 kernel) per scratch build
MIN_RUN_S = 0.05
RUNS = 5
KERNELS = {"m31": "k_batch_inverse_m", "qm31": "k_batch_inverse_q"}


# ----------------------------------------------------------------------------- the emitted code (no GPU)
def constants_of(src_text):
    return {f: int(re.search(r"BATCH_INV_E_%s = (\d+);" % f.upper(), src_text).group(1)) for f in KERNELS}


def isa_of(csrc):
    """registers and vector instructions of the two kernels as hipcc emits them for gfx950 from csrc/kernels_trace.hip"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(csrc, "kernels_trace.hip")
    out = os.path.join(csrc, "kernels_trace.field_ops.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S", src, "-o", out],
                   check=True, cwd=csrc, capture_output=True, text=True)
    asm = open(out).read()
    os.remove(out)
    e = constants_of(open(src).read())
    res = {}
    for form, kname in KERNELS.items():
        m = re.search(r"\.name:\s+(\S*%s\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                      r"\s+\.sgpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n" % kname, asm)
        start = asm.find("\n%s:" % m.group(1))
        body = asm[start:asm.find(".Lfunc_end", start)]
        n_v = len(re.findall(r"^\s+v_\w+", body, re.M))
        res[form] = {"E": e[form], "vgpr": int(m.group(4)), "sgpr": int(m.group(3)), "scratch_bytes": int(m.group(2)),
                     "vector_instructions": n_v, "vector_instructions_per_element": round(n_v / e[form], 1)}
    return res


def build_sweep(out_dir):
    csrc = os.path.join(ROOT, "luminair_amd", "csrc")
    out_dir = os.path.abspath(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    entries = [{"label": "chosen", "lib": None, "isa": isa_of(csrc)}]
    for em, eq in SWEEP:
        label = "m%d_q%d" % (em, eq)
        tree = os.path.join(out_dir, label)
        shutil.rmtree(tree, ignore_errors=True)
        # the objects travel with their times: only kernels_trace.o is compiled again
        shutil.copytree(csrc, os.path.join(tree, "luminair_amd", "csrc"), ignore=shutil.ignore_patterns("*.so", "*.b.o"))
        shutil.copytree(os.path.join(ROOT, "include"), os.path.join(tree, "include"))
        kt = os.path.join(tree, "luminair_amd", "csrc", "kernels_trace.hip")
        text = open(kt).read()
        text = re.sub(r"BATCH_INV_E_M31 = \d+;", "BATCH_INV_E_M31 = %d;" % em, text)
        text = re.sub(r"BATCH_INV_E_QM31 = \d+;", "BATCH_INV_E_QM31 = %d;" % eq, text)
        open(kt, "w").write(text)
        subprocess.run(["make", "-C", os.path.dirname(kt), "-j8", "ARCH=gfx950", "libluminair_hip.so"], check=True,
                       capture_output=True, text=True)
        lib = os.path.join(label, "libluminair_hip.so")
        shutil.copy(os.path.join(os.path.dirname(kt), "libluminair_hip.so"), os.path.join(out_dir, lib))
        entries.append({"label": label, "lib": lib, "isa": isa_of(os.path.dirname(kt))})
        shutil.rmtree(os.path.join(tree, "luminair_amd"))
        shutil.rmtree(os.path.join(tree, "include"))
    with open(os.path.join(out_dir, "sweep.json"), "w") as f:
        json.dump(entries, f, indent=1)
    print(json.dumps(entries))
    return 0


# ----------------------------------------------------------------------------- the measurement (GPU)
def measure(lib_path, logs):
    lib = backend.Library(lib_path)
    ctx = backend.Context(0, None, lib)
    L = lib.lib
    rng = np.random.default_rng(2031)
    one = ctx.col_zeros(1, 0)
    word = np.empty((1, 1), dtype=np.uint32)

    def wait():
        ctx._check(L.lmn_col_to_cpu(ctx.handle, one.handle, word.ctypes.data))

    def timed(fn, k):
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        wait()
        return time.perf_counter() - t0

    def calibrate(fn):
        k = 1
        while timed(fn, k) < MIN_RUN_S:
            k *= 2
        return k

    out = []
    for log in logs:
        host = rng.integers(0, P, size=(4, 1 << log), dtype=np.uint32)
        for form, ncols, entry in (("m31", 1, L.lmn_col_batch_inverse), ("qm31", 4, L.lmn_col_batch_inverse_secure)):
            x = host[:ncols]
            src, dst = ctx.col_from_cpu(x), ctx.col_zeros(ncols, log)
            nbytes = 4 * ncols << log
            sp, dp = src.device_ptr, dst.device_ptr

            def op():
                ctx._check(entry(ctx.handle, src.handle, dst.handle, None))

            def copy():
                ctx._check(L.lmn_device_copy(ctx.handle, dp, sp, nbytes))

            copy()
            wait()
            assert np.array_equal(dst.to_cpu(), x), "the yardstick copy did not copy"
            k_op, k_copy = calibrate(op), calibrate(copy)          # the calibration runs are the warm-up
            t_op, t_copy = [], []
            for _ in range(RUNS):
                t_op.append(timed(op, k_op) / k_op)
                t_copy.append(timed(copy, k_copy) / k_copy)
            if log == 20:
                op()
                got = dst.to_cpu().astype(np.uint64)
                if form == "m31":
                    assert np.array_equal((got * x.astype(np.uint64)) % P, (x != 0).astype(np.uint64)), "x * out != 1"
                else:
                    sys.path.insert(0, os.path.join(ROOT, "tests"))
                    import field_ops_checks
                    field_ops_checks.check_qm31_result(got, x, "field_ops_rate")
            n = 1 << log
            m_op, m_copy = statistics.median(t_op), statistics.median(t_copy)
            out.append({"form": form, "log_size": log, "bytes_read_and_written": 2 * nbytes, "calls_per_run": k_op,
                        "copies_per_run": k_copy, "op_us": [round(t * 1e6, 2) for t in t_op],
                        "copy_us": [round(t * 1e6, 2) for t in t_copy], "op_median_us": round(m_op * 1e6, 2),
                        "copy_median_us": round(m_copy * 1e6, 2), "elements_per_s": round(n / m_op),
                        "op_GB_per_s": round(2 * nbytes / m_op / 1e9, 1), "copy_GB_per_s": round(2 * nbytes / m_copy / 1e9, 1),
                        "op_rate_over_copy_rate": round(m_copy / m_op, 3)})
            src.free()
            dst.free()
    one.free()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-sweep", metavar="DIR")
    ap.add_argument("--sweep", metavar="DIR", help="a directory written by --build-sweep: its libraries are measured too")
    ap.add_argument("--logs", default=",".join(str(v) for v in LOGS))
    ap.add_argument("--out")
    ap.add_argument("--child", metavar="LIB")
    args = ap.parse_args()
    logs = [int(v) for v in args.logs.split(",")]
    if args.build_sweep:
        return build_sweep(args.build_sweep)
    if args.child:
        print("RESULT " + json.dumps(measure(args.child, logs)))
        return 0
    entries = [{"label": "chosen", "lib": None, "isa": None}]
    if args.sweep:
        entries = json.load(open(os.path.join(args.sweep, "sweep.json")))
    result = {"tool": "field_ops_rate", "min_run_ms": MIN_RUN_S * 1e3, "runs": RUNS, "yardstick": "lmn_device_copy of the same bytes",
              "builds": []}
    for e in entries:                        # a build that fails or runs out of time ends the run: nothing is tried twice
        path = os.path.join(args.sweep, e["lib"]) if e["lib"] else backend.DEFAULT_LIB
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--logs", args.logs],
                           capture_output=True, text=True, timeout=240)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write("%s failed (%d)\n%s\n" % (e["label"], r.returncode, r.stderr[-4000:]))
            return 1
        result["builds"].append({"label": e["label"], "emitted_code": e["isa"], "cases": json.loads(lines[-1][7:])})
        for c in result["builds"][-1]["cases"]:
            print("%-8s %-5s 2^%d  op %9.2f us  copy %9.2f us  %7.1f GB/s  x%.3f of the copy" % (
                e["label"], c["form"], c["log_size"], c["op_median_us"], c["copy_median_us"], c["op_GB_per_s"],
                c["op_rate_over_copy_rate"]), flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
