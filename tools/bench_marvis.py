"""Marvis / CSM on synthetic weights at the published depth (llama-1B backbone, llama-100M depth decoder, K = 32, audio vocabulary 2051):
ms per frame of the code loop alone, launches per frame, streamed weight bytes per frame and the bandwidth they imply, audio-seconds
per second of generate / generate_stream with Mimi and the time to first audio.  Warm-up run, then `--runs` timed runs: median and
spread (min / max) are reported.  One JSON line per case; --out appends them to a file (profiles/marvis/).

    python tools/bench_marvis.py --batches 1,32 --bits 0,8 --cbs 32,8 --frames 48 --runs 5 --out profiles/marvis/bench.jsonl"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mlx_audio_swift_amd as mas  # noqa: E402
from mlx_audio_swift_amd import marvis as mv  # noqa: E402


def weight_bytes_per_frame(args, Cb, bits):
    """Bytes of LM / head / projection weights streamed for one frame (every decoder position re-streams the decoder's layers)."""
    def lm(c):
        D = c.resolved_head_dim
        per = (c.num_attention_heads + 2 * c.num_key_value_heads) * D * c.hidden_size + c.hidden_size * c.num_attention_heads * D \
            + 3 * c.intermediate_size * c.hidden_size
        return per * c.num_hidden_layers
    wb = (bits / 8.0 + 4.0 / 64.0) if bits else 2.0                      # codes + a bf16 scale / bias pair per group of 64
    b, d = args.backbone, args.decoder
    total = lm(b) * wb + args.audio_vocab_size * b.hidden_size * wb                       # backbone position + codebook0_head
    if Cb > 1:
        total += d.hidden_size * b.hidden_size * 2.0 + Cb * lm(d) * wb + (Cb - 1) * args.audio_vocab_size * d.hidden_size * 2.0
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--bits", default="0,8")
    ap.add_argument("--cbs", default="32,8")
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--prompt", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    args = mv.CSMModelArgs.from_json(dict(backbone_flavor="llama-1B", decoder_flavor="llama-100M", text_vocab_size=128256,
                                          audio_vocab_size=2051, audio_num_codebooks=32))
    mimi = mas.Mimi.synthetic(mas.MimiConfig())
    rows = []
    for bits in [int(x) for x in a.bits.split(",")]:
        model = mas.MarvisTTSModel.synthetic(args, quant_bits=bits or None)
        for B in [int(x) for x in a.batches.split(",")]:
            rng = np.random.default_rng(1)
            prompts = [mv.tokenize_segment(rng.integers(0, 128256, a.prompt // 2), rng.integers(1, 2048, (32, a.prompt - a.prompt // 2)), 32,
                                           add_eos=False) for _ in range(B)]
            for Cb in [int(x) for x in a.cbs.split(",")]:
                gp = mas.MarvisGenerateParameters(max_frames=a.frames, quality_level=Cb, temperature=0.9, top_p=0.8, seed=1)
                gp1 = mas.MarvisGenerateParameters(max_frames=1, quality_level=Cb, temperature=0.9, top_p=0.8, seed=1)

                def timed(fn):
                    t0 = time.perf_counter(); r = fn(); return time.perf_counter() - t0, r
                model.generate_codes(prompts, gp)                                            # warm-up
                loop = []
                for _ in range(a.runs):                                                      # frames alone: (F frames) - (1 frame) removes reset + prefill
                    tF, codes = timed(lambda: model.generate_codes(prompts, gp))
                    t1, _ = timed(lambda: model.generate_codes(prompts, gp1))
                    n = min(len(c) for c in codes)
                    loop.append((tF - t1) / max(n - 1, 1) * 1e3)
                n_frames = sum(len(c) for c in codes)
                model.generate_batch(prompts, mimi, gp)                                      # warm-up
                gen, stream, first = [], [], []
                for _ in range(a.runs):
                    t, pcm = timed(lambda: model.generate_batch(prompts, mimi, gp))
                    gen.append(sum(len(p) for p in pcm) / 24000.0 / t)
                    t0 = time.perf_counter(); tf = None; secs = 0.0
                    for ev in model.generate_stream_batch(prompts, mimi, gp, streaming_interval=0.5):
                        if isinstance(ev, mas.AudioEvent):
                            tf = tf if tf is not None else time.perf_counter() - t0
                            secs += len(ev.audio) / 24000.0
                    stream.append(secs / (time.perf_counter() - t0)); first.append(tf * 1e3)
                med = statistics.median
                ms = med(loop)
                wb = weight_bytes_per_frame(args, Cb, bits)
                row = dict(bench="marvis", bits=bits, batch=B, Cb=Cb, frames=a.frames, runs=a.runs, frames_generated=n_frames,
                           ms_per_frame=round(ms, 4), ms_per_frame_min=round(min(loop), 4), ms_per_frame_max=round(max(loop), 4),
                           launches_per_frame=model.launches_per_frame, weight_mb_per_frame=round(wb / 1e6, 1),
                           implied_tb_per_s=round(wb / (ms * 1e-3) / 1e12, 3),
                           generate_audio_s_per_s=round(med(gen), 2), generate_min=round(min(gen), 2), generate_max=round(max(gen), 2),
                           stream_audio_s_per_s=round(med(stream), 2), stream_min=round(min(stream), 2), stream_max=round(max(stream), 2),
                           first_audio_ms=round(med(first), 2), first_audio_ms_min=round(min(first), 2), first_audio_ms_max=round(max(first), 2))
                assert row["implied_tb_per_s"] < 8.0, row                                   # sanity: nothing streams faster than HBM
                print(json.dumps(row), flush=True)
                rows.append(row)
        model.close()
    mimi.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
