"""Parakeet TDT at the published shape with synthetic weights: 10 s rows at batch 1 / 8 / 32 and one 60 s row.  Median of 5 after 2 warm-ups of
the wall clock of generate_batch's device call (it ends in the call's one synchronisation) and of the device intervals front end / encoder
(+ joint.enc) / decode, appended to profiles/parakeet/bench.jsonl.  Synthetic weights emit arbitrarily, so emissions and steps per row are
recorded beside the decode time: microseconds per step and per emission can be read off.  Nothing is gated: the parent has nothing to
compare with.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mlx_audio_swift_amd as mas  # noqa: E402
from sortformer_ref import test_wave  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--encoder-dtype", default="float32", choices=["float32", "bfloat16", "both"],
                    help="both: every case in f32 mode and in bf16 mode in the same run (profiles/parakeet_bf16/bench.jsonl)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parakeet", "bench.jsonl"))
    a = ap.parse_args()
    if mas._lib.lib().mis_device_count() < 1:
        raise SystemExit("bench_parakeet needs a GPU")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    dtypes = ("float32", "bfloat16") if a.encoder_dtype == "both" else (a.encoder_dtype,)
    for seconds, batch, dtype in ((s, b, d) for s, b in ((10, 1), (10, 8), (10, 32), (60, 1)) for d in dtypes):
        cfg = mas.ParakeetConfig(num_hidden_layers=a.layers, max_batch=batch, max_seconds=seconds, max_tokens=2048, encoder_dtype=dtype)
        m = mas.ParakeetModel.synthetic(cfg, seed=7)
        m.enable_timing()
        rows = [test_wave(100 + b, 16000 * seconds - 53 * b) for b in range(batch)]
        wall, dev, raws = [], [], None
        for i in range(a.warmup + a.runs):
            t0 = time.perf_counter()
            raws = m.decode_raw(rows)
            dt = (time.perf_counter() - t0) * 1e3
            if i >= a.warmup:
                wall.append(dt)
                dev.append(m.timing())
        med = lambda xs: float(statistics.median(xs))
        steps, emis = [r["steps"] for r in raws], [len(r["tokens"]) for r in raws]
        decode = med([d[2] for d in dev])
        frames = int(m.frames([len(r) for r in rows])[1].sum())             # 46 d^2 multiply-adds a frame and block, from the layer widths
        row = dict(bench="parakeet_tdt", encoder_dtype=dtype, encoder_tflops=2 * 46 * cfg.hidden_size ** 2 * frames * a.layers / med([d[1] for d in dev]) / 1e9,
                   layers=a.layers, seconds=seconds, batch=batch, launches=m.launches, wall_ms=med(wall), wall_min_ms=min(wall),
                   wall_max_ms=max(wall), front_ms=med([d[0] for d in dev]), encoder_ms=med([d[1] for d in dev]), decode_ms=decode, steps=steps,
                   emissions=emis, truncated=[r["truncated"] for r in raws], decode_us_per_step_longest_row=1e3 * decode / max(max(steps), 1),
                   decode_us_per_emission_longest_row=1e3 * decode / max(max(emis), 1), audio_seconds_per_second=batch * seconds / (med(wall) / 1e3))
        print(json.dumps(row))
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")
        m.close()


if __name__ == "__main__":
    main()
