"""Smart Turn timings on synthetic weights at the published shape (8 s window, 400 positions, 384 / 6 heads / 4 layers / 1536), full
8 s rows at batch 1 / 8 / 32 / 64, with the replayed graph and with MIS_NO_GRAPH=1 (plain launches).  Per (batch, mode): wall-clock ms
per predict (upload, prepare, mel, encoder, head, download; the call returns after its stream has drained), the device-side split from
the handle's event timers - prepare + mel, encoder, head; inside a graph replay encoder and head are one interval and the head is
reported as null - launches of the chain and rows per second.  Median of `--runs` timed calls after `--warmup` warm-ups.  Appends one
JSON line per step to profiles/smartturn/bench.jsonl.

Every (batch, mode) step is a child process of its own under `timeout -k 10`; the first step that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one(batch, runs, warmup, out):
    import numpy as np
    import mlx_audio_swift_amd as mas
    cfg = mas.SmartTurnConfig()
    dev = mas.SmartTurnModel.synthetic(cfg, seed=777)
    g = np.random.default_rng(batch)
    rows = [(0.1 * g.standard_normal(cfg.window_samples)).astype(np.float32) for _ in range(batch)]
    wall, parts = [], []
    for i in range(warmup + runs):
        t0 = time.perf_counter()
        dev.predict_raw(rows)
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            wall.append(dt)
            parts.append(dev.timing())
    med = lambda xs: statistics.median(xs)
    graph = os.environ.get("MIS_NO_GRAPH") is None
    head = med([p[2] for p in parts])
    row = dict(shape="8s/400/384/6/4/1536", batch=batch, graph=graph, runs=runs, warmup=warmup, predict_ms=med(wall), predict_ms_min=min(wall),
               predict_ms_max=max(wall), prepare_mel_ms=med([p[0] for p in parts]),
               encoder_ms=med([p[1] for p in parts]) if not graph else None, encoder_plus_head_ms=med([p[1] for p in parts]) if graph else None,
               head_ms=head if head >= 0 else None, launches=dev.launches, rows_per_s=batch / (med(wall) / 1e3))
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
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds a single (batch, mode) step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smartturn", "bench.jsonl"))
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        one(a.one, a.runs, a.warmup, a.out)
        return 0
    for B in a.batches:
        for no_graph in (False, True):
            env = dict(os.environ)
            env.pop("MIS_NO_GRAPH", None)
            if no_graph:
                env["MIS_NO_GRAPH"] = "1"
            r = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", str(B), "--runs",
                                str(a.runs), "--warmup", str(a.warmup), "--out", a.out], env=env)
            if r.returncode != 0:
                print(f"step batch={B} no_graph={no_graph} ended with status {r.returncode}: nothing further is started", file=sys.stderr)
                return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
