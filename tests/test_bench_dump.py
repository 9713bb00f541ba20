"""bench.py --dump-outputs: what the timed path computed in its last step (the proof bytes a caller receives, one per
context), written as float32 .npy files that repeat from run to run.  On CPU with the test-only emulation build."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libluminair_emu.so")


def _bench(out_dir, steps):
    if not os.path.exists(EMU):
        subprocess.run([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], check=True, capture_output=True)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--emu-library", EMU, "--log-rows", "5",
                        "--steps", str(steps), "--warmup", "1", "--no-extras", "--no-anchor", "--no-cpu-baseline",
                        "--dump-outputs", str(out_dir)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_dump_outputs_are_the_last_steps_proofs_and_repeat(tmp_path):
    line = _bench(tmp_path / "a", steps=3)
    assert line["steps"] == 3 and line["errors"] == []
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["proof_%02d.npy" % i for i in range(line["config"]["proofs_in_flight_per_gpu"])]
    got = np.load(tmp_path / "a" / files[0])
    assert got.dtype == np.float32
    # the bytes lmn_prove returns for the bench's trace (config 2a, rank 0's seed)
    import luminair_amd
    from luminair_amd import backend, synthetic as syn
    p = luminair_amd.Prover(0, library=backend.Library(EMU))
    want = p.ctx.prove_tables([(k, r, len(r)) for k, r in syn.config2_add_only(1 << 5, 42)])
    p.ctx.close()
    assert np.array_equal(got, np.frombuffer(want, np.uint8).astype(np.float32))
    _bench(tmp_path / "b", steps=2)
    assert sorted(os.listdir(tmp_path / "b")) == files
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_dump_outputs_keeps_to_the_size_limit_with_a_seeded_sample(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 16)
    big = (np.arange(1 << 16) % 251).astype(np.uint8)
    small = np.arange(10, dtype=np.uint8)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 1 << 16
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small.astype(np.float32))
    assert not os.path.exists(tmp_path / "a" / "small.index.npy")
    vals, idx = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "a" / "big.index.npy")
    assert vals.dtype == np.float32 and idx.dtype == np.float64 and 0 < len(vals) == len(idx) < len(big)
    assert np.array_equal(vals, big[idx.astype(np.int64)].astype(np.float32))
    assert np.array_equal(idx, np.load(tmp_path / "b" / "big.index.npy"))     # the same sample every time
