"""Wall-clock of MossFormer2SE.enhance at the published shape (24 blocks) with synthetic weights -> profiles/mossformer2/bench.jsonl.

    python tools/bench_mossformer2.py [--out profiles/mossformer2/bench.jsonl]

Cases: 10 s rows at batch 1 and 8, and one 60 s row.  Median of 5 runs after 2 warm-ups of enhance_batch (copy in, device, copy out).
Each line also carries the split of the last run - device milliseconds of the front end, the mask network and the synthesis - the
launch count, and the network interval's achieved f32 TFLOP/s against the arithmetic of the layer widths (multiply-adds a frame x 2)."""
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


def macs_per_frame(cfg, frames):
    """Multiply-adds of the mask network for one frame of a row of `frames` frames: the contractions only."""
    D, I, Q, G = cfg.out_channels, 256, 128, 256
    keys = min(frames, G)
    flash = D * (4 * D + Q) + keys * Q + keys * 4 * D + 2 * Q * 4 * D + 2 * D * D
    fsmn = D * I + I * 2 * I + 2 * I * I + I * D
    head = cfg.in_channels * D + D * D + D * 2 * D + D * cfg.out_channels_final
    return cfg.num_blocks * (flash + fsmn) + head


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mossformer2", "bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    lines = []
    for name, seconds, batch in (("10s_b1", 10, 1), ("10s_b8", 10, 8), ("60s_b1", 60, 1)):
        cfg = mas.MossFormer2SEConfig(max_batch=batch, max_seconds=float(seconds))
        model = mas.MossFormer2SE.synthetic(cfg)
        rng = np.random.default_rng(100)
        rows = [(0.05 * rng.standard_normal(seconds * cfg.sample_rate)).astype(np.float32) for _ in range(batch)]
        wall = []
        for i in range(7):
            t0 = time.perf_counter()
            out = model.enhance_batch(rows)
            if i >= 2:
                wall.append((time.perf_counter() - t0) * 1e3)
        front_ms, net_ms, synth_ms = model.timing()
        T = int(model.frames([len(rows[0])])[0][0])
        flop = 2.0 * macs_per_frame(cfg, T) * T * batch
        line = dict(case=name, seconds=seconds, batch=batch, weights="synthetic", frames=T, enhance_ms_median=statistics.median(wall),
                    enhance_ms_min=min(wall), enhance_ms_max=max(wall), device_front_ms=front_ms, device_network_ms=net_ms,
                    device_synthesis_ms=synth_ms, launches=model.launches, network_gflop=flop / 1e9,
                    network_tflops=flop / (net_ms * 1e-3) / 1e12, finite=bool(np.isfinite(out[0]).all()))
        print(json.dumps(line), flush=True)
        lines.append(line)
        model.close()
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
