"""LASR CTC timings on synthetic weights at the published shape (hidden 512, 8 heads of 64, FFN 2048, 17 layers, conv kernel 32, 128
mels, vocabulary 512), 10 s rows at batch 1 / 8 / 32.  Per batch: wall-clock ms per generate (upload, front end, encoder, CTC tail,
download; the call returns after its one synchronisation), the device-side split from the handle's event timers - front end, encoder,
tail - the launches of the call and audio seconds per second.  Median of `--runs` timed calls after `--warmup` warm-ups.  Appends one
JSON line per step to profiles/lasr/bench.jsonl.

Every batch is a child process of its own under `timeout -k 10`; the first step that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SECONDS = 10


def one(batch, runs, warmup, out):
    import numpy as np
    import mlx_audio_swift_amd as mas
    cfg = mas.LasrCTCConfig(max_batch=batch, max_seconds=SECONDS)
    dev = mas.LasrCTCModel.synthetic(cfg, seed=777)
    dev.enable_timing()
    g = np.random.default_rng(batch)
    rows = [(0.1 * g.standard_normal(SECONDS * 16000)).astype(np.float32) for _ in range(batch)]
    wall, parts = [], []
    for i in range(warmup + runs):
        t0 = time.perf_counter()
        dev.generate_tokens(rows)
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            wall.append(dt)
            parts.append(dev.timing())
    med = statistics.median
    row = dict(shape="512/8x64/2048/17/k32/128/512", seconds=SECONDS, batch=batch, runs=runs, warmup=warmup, generate_ms=med(wall),
               generate_ms_min=min(wall), generate_ms_max=max(wall), front_end_ms=med([p[0] for p in parts]),
               encoder_ms=med([p[1] for p in parts]), tail_ms=med([p[2] for p in parts]), launches=dev.launches,
               audio_s_per_s=batch * SECONDS / (med(wall) / 1e3))
    dev.close()
    print(json.dumps(row))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write(json.dumps(row) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds a single batch step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lasr", "bench.jsonl"))
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        one(a.one, a.runs, a.warmup, a.out)
        return 0
    for B in a.batches:
        r = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", str(B), "--runs",
                            str(a.runs), "--warmup", str(a.warmup), "--out", a.out])
        if r.returncode != 0:
            print(f"step batch={B} ended with status {r.returncode}: nothing further is started", file=sys.stderr)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
