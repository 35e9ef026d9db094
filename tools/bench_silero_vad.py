"""Wall-clock of SileroVAD at the published 16 kHz branch with synthetic weights -> profiles/silero_vad/bench.jsonl.

    python tools/bench_silero_vad.py [--out profiles/silero_vad/bench.jsonl]

Cases: 10 s rows at batch 1, 8, 32 and 64 (predict_proba_batch: copy in, device, copy out), one 10-minute row (18 750 chunks, walked in
passes of max_chunks 1024), and feed per chunk at batch 1 and 64.  Median of 5 runs after 2 warm-ups.  Each line also carries the split
of the last run - device milliseconds of the front end (copy in + six contractions) and of the recurrence, from events around each
pass - the microseconds of recurrence per LSTM step, and the launch count."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mlx_audio_swift_amd as mas  # noqa: E402


def row(seconds, seed):
    rng = np.random.default_rng(seed)
    x = (1e-3 * rng.standard_normal(int(seconds * 16000))).astype(np.float32)
    for start in np.arange(0.5, seconds, 4.0):
        a, b = int(start * 16000), min(int((start + 2.5) * 16000), len(x))
        x[a:b] += 0.1 * rng.standard_normal(b - a).astype(np.float32)
    return x


def timed(fn):
    wall = []
    for i in range(7):
        t0 = time.perf_counter()
        fn()
        if i >= 2:
            wall.append((time.perf_counter() - t0) * 1e3)
    return wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "silero_vad", "bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    cfg = mas.SileroVADConfig(max_batch=64, max_chunks=1024)
    model = mas.SileroVAD.synthetic(cfg)
    lines = []
    for name, seconds, batch in (("10s_b1", 10, 1), ("10s_b8", 10, 8), ("10s_b32", 10, 32), ("10s_b64", 10, 64), ("600s_b1", 600, 1)):
        rows = [row(seconds, 100 + i) for i in range(batch)]
        wall = timed(lambda: model.predict_proba_batch(rows))
        front_ms, rec_ms = model.timing()
        steps = -(-len(rows[0]) // 512)                               # LSTM steps of a row: one a chunk at the published branch
        lines.append(dict(case=name, seconds=seconds, batch=batch, weights="synthetic", predict_ms_median=statistics.median(wall),
                          predict_ms_min=min(wall), predict_ms_max=max(wall), device_front_ms=front_ms, device_recurrence_ms=rec_ms,
                          steps_per_row=steps, recurrence_us_per_step=rec_ms * 1e3 / steps, launches=model.launches, max_chunks=cfg.max_chunks,
                          audio_s_per_wall_s=seconds * batch / (statistics.median(wall) * 1e-3)))
        print(json.dumps(lines[-1]))
    for batch in (1, 64):
        chunks = np.stack([row(1.0, 200 + i)[:512] for i in range(batch)])
        state = [model.initial_state(batch)]

        def step():
            _, state[0] = model.feed(chunks, state[0])

        wall = timed(step)
        front_ms, rec_ms = model.timing()
        lines.append(dict(case=f"feed_b{batch}", batch=batch, weights="synthetic", feed_ms_median=statistics.median(wall), feed_ms_min=min(wall),
                          feed_ms_max=max(wall), device_front_ms=front_ms, device_recurrence_ms=rec_ms, recurrence_us_per_step=rec_ms * 1e3,
                          launches=model.launches))
        print(json.dumps(lines[-1]))
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
