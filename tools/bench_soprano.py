"""Secondary bench (BASELINE configs[1] / SURVEY §8d C2): Soprano-80M-shaped synthetic model, fixed 24-token prompt,
64 forced decode steps ([STOP] out of range) -> 129 024 samples (4.03 s @ 32 kHz) per row.  Positional argument = batch (default 1);
--bits 8 / 4: every Linear of the LM as a synthetic MLX-quantised matrix (group 64, bf16 scales), streamed as codes.  lm_path: the
program that ran the LM loop (1 = batch-1 token engine, 0 = launch chain; MIS_TOKEN_ENGINE=0 forces the chain)."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mlx_audio_swift_amd as mas

ap = argparse.ArgumentParser()
ap.add_argument("batch", type=int, nargs="?", default=1)
ap.add_argument("--bits", type=int, choices=(0, 8, 4), default=0)
args = ap.parse_args()
B = args.batch
cfg = mas.SopranoConfiguration(stop_token_id=-1)
m = mas.SopranoModel.synthetic(cfg, seed=4321, quant_bits=args.bits or None)
rng = np.random.default_rng(1235)
rows = [rng.integers(4, 8000, 24).astype(np.int32) for _ in range(B)]
gp = mas.GenerateParameters(max_tokens=64, temperature=0.7, top_p=0.95, repetition_penalty=1.5, repetition_context_size=30,
                            seed=7, sampler_flavor=1)
best = 1e9
for rep in range(4):
    t0 = time.perf_counter(); pcm = m.generate_batch(rows, gp); dt = time.perf_counter() - t0
    best = min(best, dt)
audio_s = sum(len(p) for p in pcm) / cfg.sample_rate
lm = f"{args.bits}-bit" if args.bits else "bf16"
print(json.dumps({"workload": f"Soprano-80M {lm} LM + f32 Vocos/ISTFT decoder, batch {B}, 24-token prompt, 64 new tokens",
                  "samples_per_row": int(len(pcm[0])), "generate_ms": best * 1e3, "audio_s_per_s": audio_s / best,
                  "ms_per_token": best * 1e3 / 64, "bits": args.bits, "lm_path": m.lm_path,
                  "token_engine_env": os.environ.get("MIS_TOKEN_ENGINE")}))
