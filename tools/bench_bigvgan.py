"""Wall-clock of BigVGAN.decode at the published 24 kHz / 100-band depth with synthetic weights -> profiles/bigvgan/bench.jsonl.

    python tools/bench_bigvgan.py [--out profiles/bigvgan/bench.jsonl]

Cases: 10 s rows (938 mel frames) at batch 1 and 8, and one 60 s row (5625 frames).  Median of 5 runs after 2 warm-ups of decode (copy
in, device, copy out).  Each line also carries the device interval of the last run (events behind the copy in and before the copy out),
the launch count, audio seconds per second of wall-clock, and the achieved TFLOP/s of the device interval from the FLOP count DERIVED
from the layer widths (2 x multiply-adds of conv_pre, the transposed convs, the AMP-block convs and conv_post; the activations are not
counted)."""
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

SAMPLE_RATE = 24000


def published(**workspace):
    return mas.BigVGANConfig(num_mels=100, upsample_rates=[4, 4, 2, 2, 2, 2], upsample_kernel_sizes=[8, 8, 4, 4, 4, 4],
                             upsample_initial_channel=1536, resblock="1", resblock_kernel_sizes=[3, 7, 11],
                             resblock_dilation_sizes=[[1, 3, 5]] * 3, activation="snakebeta", snake_logscale=True, **workspace)


def macs_per_frame(cfg) -> int:
    """Multiply-adds of the convolutions for one mel frame, from the layer widths."""
    per_conv = 2 if cfg.resblock == "1" else 1
    total, cum = 7 * cfg.num_mels * cfg.upsample_initial_channel, 1
    for i, rate in enumerate(cfg.upsample_rates):
        ch = cfg.upsample_initial_channel >> (i + 1)
        cum *= rate
        total += cum * 2 * (2 * ch) * ch                                  # two taps reach every output sample of the transposed conv
        total += cum * ch * ch * sum(per_conv * len(d) * k for k, d in zip(cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes))
    return total + cum * 7 * ch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bigvgan", "bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    lines = []
    model, key = None, None
    for name, seconds, batch in (("10s_b1", 10, 1), ("10s_b8", 10, 8), ("60s_b1", 60, 1)):
        frames = -(-seconds * SAMPLE_RATE // 256)
        if key != frames:
            if model is not None:
                model.close()
            cfg = published(max_batch=8 if seconds == 10 else 1, max_frames=frames)
            model, key = mas.BigVGAN.synthetic(cfg), frames
        mel = np.random.default_rng(seconds + batch).standard_normal((batch, cfg.num_mels, frames), dtype=np.float32)
        wall = []
        for i in range(7):
            t0 = time.perf_counter()
            wav = model.decode(mel)
            if i >= 2:
                wall.append((time.perf_counter() - t0) * 1e3)
        device_ms, med = model.timing(), statistics.median(wall)
        flops = 2.0 * macs_per_frame(cfg) * frames * batch
        line = dict(case=name, seconds=seconds, batch=batch, frames=frames, weights="synthetic", decode_ms_median=med, decode_ms_min=min(wall),
                    decode_ms_max=max(wall), device_ms=device_ms, launches=model.launches,
                    audio_s_per_s=batch * frames * cfg.hop_length / SAMPLE_RATE / (med / 1e3), gmacs_per_frame_derived=macs_per_frame(cfg) / 1e9,
                    tflops_device_derived=flops / (device_ms / 1e3) / 1e12, finite=bool(np.isfinite(wav).all()), peak=float(np.abs(wav).max()))
        print(json.dumps(line))
        lines.append(line)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
