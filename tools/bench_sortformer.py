"""Sortformer diarization timings at the published shape with synthetic weights -> profiles/sortformer/bench.jsonl.
10 s rows at batch 1 / 8 / 32 and one 90 s row through generate_batch, one 90 s row through generate_stream at 5 s chunks with both
compression modes; median of 5 runs after 2 warm-ups; wall-clock, the device intervals of the forward call (front end / stem /
Conformer / BART + head) and launches per call.

    python tools/bench_sortformer.py [--out profiles/sortformer/bench.jsonl]

--encoder-dtype bfloat16 (or both) -> profiles/sortformer_bf16/bench.jsonl: f32 mode and bf16 mode of the same build in ONE process, the two
models alive side by side and their runs alternating (median of 7 after 3 warm-ups each).  Offline: generate_batch of 10 s x 1 / 8 / 32 and of
one 119 s row (the longest max_source_positions 1500 admits).  Streaming: encode_embeddings alone at the frame counts generate_stream's steps
reach with the default cache 188, FIFO 188 and 5 s chunks: 63 (the first chunk), 251, 439 (cache and FIFO full)."""
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


def alternating(fns, runs=7, warm=3):
    """{name: (median wall ms, the last run's return)} of callables run in turn, so that drift of the machine meets all of them alike"""
    wall, extra = {k: [] for k in fns}, {}
    for i in range(warm + runs):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            extra[k] = fn()
            if i >= warm:
                wall[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (statistics.median(wall[k]), extra[k]) for k in fns}


def compare_dtypes(dtypes):
    rows = []

    def pair(case, make, fields, **tags):
        res = alternating(make)
        for dt, (ms, extra) in res.items():
            rows.append(dict(case=case, encoder_dtype=dt, wall_ms=ms, **tags, **fields(extra)))
        if len(res) == 2:
            rows.append(dict(case=case + "_ratio", f32_over_bf16_wall=res["float32"][0] / res["bfloat16"][0], **tags))

    for batch, seconds in ((1, 10), (8, 10), (32, 10), (1, 119)):
        models = {dt: mas.SortformerModel.synthetic(mas.SortformerConfig(max_batch=batch, max_seconds=seconds + 1), encoder_dtype=dt) for dt in dtypes}
        audio = [wave(b, seconds) for b in range(batch)]
        for m in models.values():
            m.enable_timing()

        def call(m):
            m.generate_batch(audio)
            return m.timing(), m.launches

        pair("generate", {dt: (lambda m=m: call(m)) for dt, m in models.items()},
             lambda e: dict(front_ms=e[0][0], stem_ms=e[0][1], conformer_ms=e[0][2], bart_head_ms=e[0][3], launches=e[1]), batch=batch, seconds=seconds)
        for m in models.values():
            m.close()
    models = {dt: mas.SortformerModel.synthetic(mas.SortformerConfig(max_batch=1, max_seconds=60), encoder_dtype=dt) for dt in dtypes}
    rng = np.random.default_rng(5)
    for T in (63, 251, 439):
        emb = rng.standard_normal((1, T, 512)).astype(np.float32)

        def step(m):
            m.encode_embeddings(emb)
            return m.launches

        pair("encode_embeddings", {dt: (lambda m=m: step(m)) for dt, m in models.items()}, lambda e: dict(launches=e), frames=T)
    for m in models.values():
        m.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--encoder-dtype", choices=("float32", "bfloat16", "both"), default="float32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    bf16 = args.encoder_dtype != "float32"
    args.out = args.out or os.path.join(ROOT, "profiles", "sortformer_bf16" if bf16 else "sortformer", "bench.jsonl")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    rows = compare_dtypes(("float32", "bfloat16") if args.encoder_dtype == "both" else ("bfloat16",)) if bf16 else []
    for batch, seconds in () if bf16 else ((1, 10), (8, 10), (32, 10), (1, 90)):
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
    for aosc in () if bf16 else (False, True):
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
