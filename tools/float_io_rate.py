#!/usr/bin/env python3
"""What the host round trip of a float graph input costs: `gen_trace` of a graph whose cost is its inputs - one float32 weight
tensor of --log-n elements (default 2^20) that lives in HBM as a torch tensor, consumed by one Add with a one-element bias.

Two paths, in one process on one GPU, alternating call by call:

  device   `input_float(weight)`: the tensor is read where it lies, converted inside the launch that writes its Inputs rows
  host     what a caller does on the interface without float inputs: `weight.cpu()`, the rounding rule in numpy
           (floor(|x| * 4096 + 0.5) with the sign put back), then `input(int32 array)` - staged and uploaded by gen_trace

Each timed call builds the graph, runs `gen_trace` and ends in one download of a word of the output tensor, which waits
for the context's stream - so the window covers everything from the torch tensor to finished rows.  --warmup calls of each
path first (code objects, the slab cache, torch's allocator), then --reps timed calls of each, in turn.  The rows of the two
paths are compared once, word for word.  No threshold: the file says which path was faster.

  float_io_rate.py --out profiles/float_io_rate.json"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "float_io_rate.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from luminair_amd import backend
    from luminair_amd.graph import DeviceGraph
    if not torch.cuda.is_available():
        print("float_io_rate: no GPU - nothing is measured", file=sys.stderr)
        return 1
    n = 1 << args.log_n
    ctx = backend.Context(0, None, backend.default_library())
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    weight = torch.randn(n, device="cuda:0", dtype=torch.float32, generator=gen) * 4.0
    torch.cuda.synchronize()

    def build_device(g):
        return g.input_float(weight)

    def build_host(g):
        x = weight.cpu().numpy().astype(np.float64)
        return g.input((np.sign(x) * np.floor(np.abs(x) * 4096.0 + 0.5)).astype(np.int32))

    def run(build, keep=False):
        t0 = time.perf_counter()
        g = DeviceGraph(ctx)
        y = g.add(build(g), g.broadcast_to(g.constant(4096), (n,)))
        g.output(y)
        tables, _, bufs = g.gen_trace()
        ctx.download(y.buf.view(0, 4))                 # the wait: the context's stream has finished the rows
        dt = (time.perf_counter() - t0) * 1e3
        words = [ctx.download(b) for _, b, _ in tables] if keep else None
        for b in bufs:
            b.free()
        return dt, words

    paths = {"device": build_device, "host": build_host}
    same = all(np.array_equal(a, b) for a, b in zip(run(build_device, True)[1], run(build_host, True)[1]))
    for _ in range(args.warmup):
        for build in paths.values():
            run(build)
    ms = {k: [] for k in paths}
    for _ in range(args.reps):
        for k, build in paths.items():
            ms[k].append(run(build)[0])
    stat = {k: {"p50": round(sorted(v)[len(v) // 2], 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in ms.items()}
    doc = {"what": "gen_trace of one 2^%d-element float32 weight tensor (resident in HBM as a torch tensor) + one Add, ms per call "
                   "from the torch tensor to finished rows (host clock around build + gen_trace + one download that waits for "
                   "the context's stream); device = input_float on the tensor, host = .cpu() + numpy rounding + input(int32); "
                   "%d warm-up calls per path, then %d timed calls per path in turn, one process, one MI355X" %
                   (args.log_n, args.warmup, args.reps),
           "elements": n, "rows_identical": bool(same), "ms": stat,
           "device_path_faster": stat["device"]["p50"] < stat["host"]["p50"],
           "host_over_device_p50": round(stat["host"]["p50"] / stat["device"]["p50"], 2)}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc), flush=True)
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
