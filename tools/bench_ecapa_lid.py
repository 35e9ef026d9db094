"""Language-identification timings on synthetic weights at the published shape (60 mels / 1024 channels / 128 attention / 128 SE /
256 embedding / 512 hidden / 107 classes), 10 s rows at batch 1 / 8 / 32 / 64.  Per batch: wall-clock ms per predict (upload, front
end, model, download; the call returns after its stream has drained), the device-side split from the handle's event timers - front
end, model - the launches of the call and rows per second.  Median of `--runs` timed calls after `--warmup` warm-ups.  Appends one
JSON line per step to profiles/ecapa_lid/bench.jsonl.

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
    cfg = mas.EcapaTdnnConfig(max_batch=batch, max_samples=SECONDS * 16000)
    dev = mas.EcapaTdnnLID.synthetic(cfg, seed=777)
    g = np.random.default_rng(batch)
    rows = [(0.1 * g.standard_normal(SECONDS * 16000)).astype(np.float32) for _ in range(batch)]
    wall, parts = [], []
    for i in range(warmup + runs):
        t0 = time.perf_counter()
        dev.predict_raw(rows)
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            wall.append(dt)
            parts.append(dev.timing())
    med = statistics.median
    row = dict(shape="60/1024/128/128/256/512/107", seconds=SECONDS, batch=batch, runs=runs, warmup=warmup, predict_ms=med(wall),
               predict_ms_min=min(wall), predict_ms_max=max(wall), front_end_ms=med([p[0] for p in parts]),
               model_ms=med([p[1] for p in parts]), launches=dev.launches, rows_per_s=batch / (med(wall) / 1e3))
    dev.close()
    print(json.dumps(row))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write(json.dumps(row) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32, 64])
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds a single batch step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ecapa_lid", "bench.jsonl"))
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
