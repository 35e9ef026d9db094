"""Nemotron ASR at the published shape with synthetic weights: 10 s rows at batch 1 / 8 / 32, one 60 s and one 400 s row.  Median of 5 after 2
warm-ups of the wall clock of generate_batch's device call (it ends in the call's one synchronisation) and of the device intervals front end /
encoder (+ prompt + joint.enc) / decode, and the attention launch alone on a 60 s and a 400 s row at context (56, 13) against the same launch
with left = -1 (the full walk: the baseline the tile skip is measured against), appended to profiles/nemotron/bench.jsonl.  --encoder-dtype
both runs every case in f32 mode and in bf16 mode in one process on the same rows, and both attention kernels alone on the same tensors
(profiles/nemotron_bf16/bench.jsonl).  Nothing is gated.  Needs a GPU; there is no fallback."""
import argparse
import ctypes as C
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
from mlx_audio_swift_amd.generation import check  # noqa: E402
from sortformer_ref import test_wave  # noqa: E402


def attention_alone(T, left, right, repeat, dtype="float32"):
    H, hd = 8, 128
    w, rng = H * hd, np.random.default_rng(1)
    qkv, table = rng.standard_normal((1, T, 3 * w)).astype(np.float32), rng.standard_normal((2 * T - 1, w)).astype(np.float32)
    u, v = (rng.uniform(-0.5, 0.5, (H, hd)).astype(np.float32) for _ in range(2))
    cnt, ms = np.asarray([T], np.int32), C.c_float(0)
    fn = mas._lib.lib().mis_debug_nemotron_attn
    if dtype == "bfloat16":                                               # the same tensors, truncated to bf16 bit patterns: the time does not depend on the values
        qkv, table = ((x.view(np.uint32) >> 16).astype(np.uint16) for x in (qkv, table))
        fn = mas._lib.lib().mis_debug_nemotron_attn_bf16
    out = np.zeros((1, T, w), qkv.dtype)
    check(fn(0, qkv.ctypes.data, 3 * w, w, 2 * w, cnt.ctypes.data, 1, T, H, hd, 1.0, float(np.sqrt(hd)), u.ctypes.data, v.ctypes.data, table.ctypes.data, w,
             2 * T - 1, T - 1, left, right, T, w, out.ctypes.data, repeat, C.byref(ms)))
    return float(ms.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--encoder-dtype", default="float32", choices=["float32", "bfloat16", "both"],
                    help="both: every case in f32 mode and in bf16 mode in the same run (profiles/nemotron_bf16/bench.jsonl)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nemotron", "bench.jsonl"))
    a = ap.parse_args()
    if mas._lib.lib().mis_device_count() < 1:
        raise SystemExit("bench_nemotron needs a GPU")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)

    def emit(row):
        print(json.dumps(row), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")

    med = lambda xs: float(statistics.median(xs))
    dtypes = ("float32", "bfloat16") if a.encoder_dtype == "both" else (a.encoder_dtype,)
    for max_seconds, max_batch, cases, dtype in ((s, b, c, d) for s, b, c in ((10, 32, ((10, 1), (10, 8), (10, 32))), (400, 1, ((60, 1), (400, 1)))) for d in dtypes):
        cfg = mas.NemotronConfig(num_hidden_layers=a.layers, max_batch=max_batch, max_seconds=max_seconds, max_tokens=8192, max_symbols=10, encoder_dtype=dtype)
        m = mas.NemotronASR.synthetic(cfg, seed=7)
        m.enable_timing()
        for seconds, batch in cases:
            rows = [test_wave(100 + b, 16000 * seconds - 53 * b) for b in range(batch)]
            wall, dev, raws = [], [], None
            for i in range(a.warmup + a.runs):
                t0 = time.perf_counter()
                raws = m.decode_raw(rows)
                dt = (time.perf_counter() - t0) * 1e3
                if i >= a.warmup:
                    wall.append(dt)
                    dev.append(m.timing())
            steps, emis = [r["steps"] for r in raws], [len(r["tokens"]) for r in raws]
            emit(dict(bench="nemotron_rnnt", encoder_dtype=dtype, layers=a.layers, seconds=seconds, batch=batch, context=list(cfg.default_context), launches=m.launches,
                      wall_ms=med(wall), wall_min_ms=min(wall), wall_max_ms=max(wall), front_ms=med([d[0] for d in dev]),
                      encoder_ms=med([d[1] for d in dev]), decode_ms=med([d[2] for d in dev]), steps_max=max(steps), emissions_max=max(emis),
                      truncated=any(r["truncated"] for r in raws), audio_seconds_per_second=batch * seconds / (med(wall) / 1e3)))
        m.close()
    for seconds in (60, 400):
        T = 1 + 16000 * seconds // 160
        for _ in range(3):
            T = T // 2 + 1
        for dtype in dtypes:
            emit(dict(bench="nemotron_attn_alone", encoder_dtype=dtype, seconds=seconds, frames=T, heads=8, head_size=128,
                      chunked_56_13_ms=attention_alone(T, 56, 13, 5, dtype), full_walk_left_unlimited_ms=attention_alone(T, -1, 13, 5, dtype)))


if __name__ == "__main__":
    main()
