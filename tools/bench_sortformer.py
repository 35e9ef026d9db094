"""Sortformer diarization timings at the published shape with synthetic weights -> profiles/sortformer/bench.jsonl.
10 s rows at batch 1 / 8 / 32 and one 90 s row through generate_batch, one 90 s row through generate_stream at 5 s chunks with both
compression modes; median of 5 runs after 2 warm-ups; wall-clock, the device intervals of the forward call (front end / stem /
Conformer / BART + head) and launches per call.

    python tools/bench_sortformer.py [--out profiles/sortformer/bench.jsonl]"""
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


def wave(seed, seconds):
    rng = np.random.default_rng(seed)
    n = int(16000 * seconds)
    t = np.arange(n) / 16000.0
    return (0.05 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * 220 * t) * (0.5 + 0.5 * np.sin(2 * np.pi * 1.5 * t))).astype(np.float32)


def median_of(fn, runs=5, warm=2):
    for _ in range(warm):
        fn()
    wall, extra = [], None
    for _ in range(runs):
        t0 = time.perf_counter()
        extra = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(wall), extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sortformer", "bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    rows = []
    for batch, seconds in ((1, 10), (8, 10), (32, 10), (1, 90)):
        m = mas.SortformerModel.synthetic(mas.SortformerConfig(max_batch=batch, max_seconds=seconds + 1))
        m.enable_timing()
        audio = [wave(b, seconds) for b in range(batch)]

        def call():
            m.generate_batch(audio)
            return m.timing(), m.launches

        ms, (dev, launches) = median_of(call)
        rows.append(dict(case="generate", batch=batch, seconds=seconds, wall_ms=ms, front_ms=dev[0], stem_ms=dev[1], conformer_ms=dev[2],
                         bart_head_ms=dev[3], launches=launches, audio_seconds_per_second=batch * seconds / (ms / 1e3)))
        m.close()
    for aosc in (False, True):
        cfg = mas.SortformerConfig(max_batch=1, max_seconds=91, modules_config=mas.ModulesConfig(use_aosc=aosc))
        m = mas.SortformerModel.synthetic(cfg)
        audio = wave(3, 90)

        def stream():
            n, launches = 0, 0
            for _ in m.generate_stream(audio, chunk_duration=5.0):
                n += 1
                launches += m.launches
            return n, launches

        ms, (chunks, launches) = median_of(stream)
        rows.append(dict(case="generate_stream", use_aosc=aosc, seconds=90, chunk_seconds=5.0, chunks=chunks, wall_ms=ms,
                         encode_launches_per_chunk=launches / chunks, audio_seconds_per_second=90 / (ms / 1e3)))
        m.close()
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
