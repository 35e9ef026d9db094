"""Canary at the published shape with synthetic weights: 10 s rows at batch 1 / 8 / 32, the median of 5 generates after 2 warm-ups.
Per batch one JSON line in profiles/canary/bench.jsonl: encoder ms, cross-K/V ms, ms per decode step and launches per step (with the
captured graph, or with plain launches when MIS_NO_GRAPH=1 is set: run the tool twice), the derived weight bytes of a step and a
device-to-device copy of the f32 step's size timed in the same run as the bandwidth yardstick.  --decoder-dtype both runs every batch with
the f32 decoder and with the bf16 decoder in the same run and adds step_ms_f32_over_bf16 to the bf16 line (profiles/canary_bf16/bench.jsonl).

    python tools/bench_canary.py [--batches 1,8,32] [--seconds 10] [--tokens 64] [--decoder-dtype both] [--out profiles/canary/bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import mlx_audio_swift_amd as mas
    import sortformer_ref as R
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--enc-layers", type=int, default=32)
    ap.add_argument("--encoder-dtype", default="float32", choices=["float32", "bfloat16"])
    ap.add_argument("--decoder-dtype", default="float32", choices=["float32", "bfloat16", "both"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "canary", "bench.jsonl"))
    a = ap.parse_args()
    batches = [int(b) for b in a.batches.split(",")]
    cfg = mas.CanaryConfig(encoder=mas.CanaryEncoderConfig(n_layers=a.enc_layers), max_batch=max(batches), max_seconds=int(np.ceil(a.seconds)),
                           max_tokens=a.tokens, max_prompt=16, encoder_dtype=a.encoder_dtype)
    dtypes = ("float32", "bfloat16") if a.decoder_dtype == "both" else (a.decoder_dtype,)
    models = {dt: mas.CanaryModel.synthetic(cfg, seed=11, decoder_dtype=dt) for dt in dtypes}
    for m in models.values():
        m.enable_timing()
    d, h = cfg.decoder, cfg.enc_output_dim
    step_floats = d.num_layers * (6 * h * h + 2 * h * d.inner_size) + h * cfg.vocab_size
    src = torch.empty(step_floats, dtype=torch.float32, device="cuda")
    dst = torch.empty_like(src)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    wave = R.test_wave(5, int(16000 * a.seconds))
    for B, dt in ((B, dt) for B in batches for dt in dtypes):
        m, wbytes = models[dt], 4 if dt == "float32" else 2
        prompts = [[0, 1, 2, 4 + b % 5, 9] for b in range(B)]
        rows = []
        for it in range(7):
            m.decode_raw([wave] * B, prompts, eos=-1, max_tokens=a.tokens)      # no eos: every row runs to max_tokens
            if it >= 2:
                rows.append(m.timing() + (m.last_steps, m.launches))
        copies = []
        for it in range(7):
            ev[0].record(); dst.copy_(src); ev[1].record(); torch.cuda.synchronize()
            if it >= 2:
                copies.append(ev[0].elapsed_time(ev[1]))
        med = lambda i: statistics.median(r[i] for r in rows)
        steps = rows[0][4]
        rec = dict(batch=B, encoder_dtype=a.encoder_dtype, decoder_dtype=dt, seconds=a.seconds, enc_layers=a.enc_layers, graph=os.environ.get("MIS_NO_GRAPH") is None, front_ms=med(0), encoder_ms=med(1),
                   cross_kv_ms=med(2), steps=steps, step_ms=med(3) / steps, launches_per_step=11 * d.num_layers + 2, launches=rows[0][5],
                   step_weight_bytes=wbytes * step_floats, d2d_copy_bytes=4 * step_floats, d2d_copy_ms=statistics.median(copies), S_out_proj=8 if h <= 1024 else 4 if h <= 2048 else 2)
        rec["step_over_copy"] = rec["step_ms"] / rec["d2d_copy_ms"]
        if dt == "float32":
            f32_step = rec["step_ms"]
        elif len(dtypes) == 2:
            rec["step_ms_f32_over_bf16"] = f32_step / rec["step_ms"]
        print(json.dumps(rec))
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
