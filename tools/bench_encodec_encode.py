"""Wall-clock of Encodec.encode at the published 24 kHz shape (32 filters, ratios 8 5 4 2, LSTM width 512, 128-dim codebooks of 1024
entries) with synthetic weights -> profiles/encodec_encode/bench.jsonl.

    python tools/bench_encodec_encode.py [--out profiles/encodec_encode/bench.jsonl]

Cases: 10 s rows at batch 1 / 8 / 32 for 6 kbps and 24 kbps (8 / 32 quantizers), and one 60 s row at both.  Median of 5 runs after 2
warm-ups of encode (host chunk walk, copy in, device, copy out).  Wall-clock only: the engine has no per-phase timers, so the split
into normalise / encoder convs / LSTM / RVQ and the launch count are NOT reported."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encodec_encode", "bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    cfg = mas.EncodecConfig()                                               # the encodec_24khz defaults
    model = mas.Encodec.synthetic(cfg)
    lines = []
    for seconds, batch in ((10, 1), (10, 8), (10, 32), (60, 1)):
        L = seconds * cfg.sampling_rate
        x = (0.1 * np.random.default_rng(seconds + batch).standard_normal((batch, L, 1))).astype(np.float32)
        for bw in (6.0, 24.0):
            wall = []
            for i in range(7):
                t0 = time.perf_counter()
                codes, _ = model.encode(x, bandwidth=bw)
                if i >= 2:
                    wall.append((time.perf_counter() - t0) * 1e3)
            med = statistics.median(wall)
            line = dict(case=f"{seconds}s_b{batch}_{bw:g}kbps", seconds=seconds, batch=batch, bandwidth=bw, n_q=int(codes.shape[2]),
                        frames=int(codes.shape[3]), weights="synthetic", encode_ms_median=med, encode_ms_min=min(wall), encode_ms_max=max(wall),
                        audio_s_per_s=batch * seconds / (med / 1e3), codes_in_range=bool(codes.min() >= 0 and codes.max() < cfg.codebook_size))
            print(json.dumps(line), flush=True)
            lines.append(line)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
