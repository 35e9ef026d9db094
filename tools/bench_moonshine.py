"""Moonshine timings on synthetic weights at the published tiny (288 / 1152 / 6+6 / 8 heads / V 32768) and base (416 / 1664 / 8+8)
depths, 10 s rows at batch 1 and 32: encode ms, ms per decoder step, launches per step, audio-s/s of generate with a forced token
count (an unreachable EOS id, so every row runs max_tokens steps).  Appends one JSON line per (model, batch) to
profiles/moonshine/bench.jsonl.  Wall-clock around synchronous ABI calls (each returns after its stream has drained); warm-up runs
first, then `--runs` timed repetitions, median and min..max reported."""
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

MODELS = {"tiny": dict(hidden_size=288, intermediate_size=1152, encoder_num_hidden_layers=6, decoder_num_hidden_layers=6),
          "base": dict(hidden_size=416, intermediate_size=1664, encoder_num_hidden_layers=8, decoder_num_hidden_layers=8)}


def timed(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), runs=runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moonshine", "bench.jsonl"))
    a = ap.parse_args()
    n = int(a.seconds * 16000)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for name, shape in MODELS.items():
        cfg = mas.MoonshineConfig(vocab_size=32768, eos_token_id=32767, **shape)
        dev = mas.MoonshineModel.synthetic(cfg, seed=777)
        for B in (1, 32):
            g = np.random.default_rng(B)
            rows = [(0.1 * g.standard_normal(n)).astype(np.float32) for _ in range(B)]
            gp = mas.STTGenerateParameters(max_tokens=a.tokens, temperature=0.0)
            enc = timed(lambda: dev.encode(rows, want_output=False), a.warmup, a.runs)
            ids = dev.generate_ids(rows, gp)
            forced = all(len(t) == a.tokens for t in ids)
            gen = timed(lambda: dev.generate_ids(rows, gp), a.warmup, a.runs)
            tok = np.zeros(B, np.int32)

            def steps():
                dev.decoder_reset(a.tokens)
                for _ in range(a.tokens):
                    dev.decoder_forward(tok, want_logits=False)
            dev.encode(rows, want_output=False)
            st = timed(steps, 1, a.runs)
            row = dict(model=name, batch=B, seconds_per_row=a.seconds, tokens=a.tokens, forced_token_count=forced, encode=enc, generate=gen,
                       step_ms_in_generate=(gen["median_ms"] - enc["median_ms"]) / a.tokens,
                       step_ms_teacher_forced_with_sync=st["median_ms"] / a.tokens, launches_per_step=dev.launches_per_step,
                       audio_s_per_s=B * a.seconds / (gen["median_ms"] / 1e3), frames_per_row=int(mas.moonshine_frames(n)))
            print(json.dumps(row))
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")
        dev.close()


if __name__ == "__main__":
    main()
