"""The Nemotron stream session at the published shape with synthetic weights.  Median of 5 after 2 warm-ups (a warm-up and a run are each one
feed of one native chunk, 80 (right + 1) ms of audio a stream, on streams that already hold a full left context): wall clock of the feed (it
ends in the feed's one synchronisation) and its device time, at 1 / 8 / 32 / 64 streams for the right contexts 0, 1, 3, 6, 13, beside the
budget - the chunk's own duration; k_nm_attn_stream alone on the last chunk of a 70-frame row against k_nm_attn on the whole row; and the
same 10 s row through transcribe_streaming and through offline generate.  Synthetic weights emit max_symbols tokens on every frame: the
decode share is that worst case, as in tools/bench_nemotron.py.  Appended to profiles/nemotron_stream/bench.jsonl.  Nothing is gated.  Needs a
GPU; there is no fallback."""
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


def attention_alone(repeat):
    H, hd, T, left, right = 8, 128, 70, 56, 13
    w, rng, Cs = H * hd, np.random.default_rng(1), right + 1
    qkv, table = rng.standard_normal((1, T, 3 * w)).astype(np.float32), rng.standard_normal((2 * T - 1, w)).astype(np.float32)
    u, v = (rng.uniform(-0.5, 0.5, (H, hd)).astype(np.float32) for _ in range(2))
    p = lambda a: a.ctypes.data
    cnt, out, ms = np.asarray([T], np.int32), np.zeros((1, T, w), np.float32), C.c_float(0)
    check(mas._lib.lib().mis_debug_nemotron_attn(0, p(qkv), 3 * w, w, 2 * w, p(cnt), 1, T, H, hd, 1.0, float(np.sqrt(hd)), p(u), p(v), p(table), w, 2 * T - 1,
                                                 T - 1, left, right, T, w, p(out), repeat, C.byref(ms)))
    Rr, pos, n = 128, np.asarray([T - Cs], np.int32), np.asarray([Cs], np.int32)
    q, ring, so, ms2 = np.ascontiguousarray(qkv[:, T - Cs:, :w]), np.zeros((1, Rr, 2 * w), np.float32), np.zeros((1, Cs, w), np.float32), C.c_float(0)
    ring[0, :T] = qkv[0, :, w:]
    check(mas._lib.lib().mis_debug_nemotron_attn_stream(0, p(q), p(ring), Rr, p(n), p(pos), 1, Cs, H, hd, 1.0, float(np.sqrt(hd)), p(u), p(v), p(table), w,
                                                        2 * T - 1, T - 1, left, right, p(so), repeat, C.byref(ms2)))
    same = bool(np.array_equal(so[0].view(np.uint32), out[0, T - Cs:].view(np.uint32)))
    return dict(bench="nemotron_attn_stream_alone", frames=T, heads=H, head_size=hd, offline_whole_row_ms=float(ms.value), stream_last_chunk_ms=float(ms2.value),
                same_bits=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8, 32, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nemotron_stream", "bench.jsonl"))
    a = ap.parse_args()
    if mas._lib.lib().mis_device_count() < 1:
        raise SystemExit("bench_nemotron_stream needs a GPU")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)

    def emit(row):
        print(json.dumps(row), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")

    med = lambda xs: float(statistics.median(xs))
    rights = (0, 1, 3, 6, 13)
    cfg = mas.NemotronConfig(num_hidden_layers=a.layers, max_batch=1, max_seconds=10, max_tokens=8192, max_symbols=10,
                             att_context_size=[[56, r] for r in rights[::-1]])
    m = mas.NemotronASR.synthetic(cfg, seed=7)
    for right in rights:
        chunk = 1280 * (right + 1)
        for S in a.streams:
            s = mas.NemotronStreamSession(m, S, att_context_size=(56, right), max_pass_frames=right + 1)
            waves = [test_wave(100 + b, chunk * (a.warmup + a.runs + 1) + 1280 * 57) for b in range(S)]
            at = 1280 * 57 + 256                                           # the left context is full before anything is timed
            for lo in range(0, at, 1280 * 14):
                s.feed_raw([w[lo:min(lo + 1280 * 14, at)] for w in waves])
            wall, dev, toks = [], [], 0
            for i in range(a.warmup + a.runs):
                t0 = time.perf_counter()
                out = s.feed_raw([w[at:at + chunk] for w in waves])
                dt = (time.perf_counter() - t0) * 1e3
                at += chunk
                if i >= a.warmup:
                    wall.append(dt); dev.append(s.timing()); toks = max(len(o[0]) for o in out)
            emit(dict(bench="nemotron_stream_feed", layers=a.layers, streams=S, context=[56, right], budget_ms=80 * (right + 1), launches=s.launches,
                      wall_ms=med(wall), wall_min_ms=min(wall), wall_max_ms=max(wall), device_ms=med(dev), tokens_a_feed_max=toks,
                      decode="synthetic weights: max_symbols emissions on every frame"))
            s.close()
    emit(attention_alone(20))
    wave = test_wave(7, 160000)
    runs = dict(stream=[], offline=[])
    for i in range(a.warmup + a.runs):
        t0 = time.perf_counter(); r1 = m.transcribe_streaming(wave, chunk_ms=480); t1 = time.perf_counter()
        r2 = m.generate(wave); t2 = time.perf_counter()
        if i >= a.warmup:
            runs["stream"].append((t1 - t0) * 1e3); runs["offline"].append((t2 - t1) * 1e3)
    emit(dict(bench="nemotron_stream_vs_offline_10s", layers=a.layers, context=list(cfg.default_context), transcribe_streaming_ms=med(runs["stream"]),
              offline_generate_ms=med(runs["offline"]), same_tokens=[t.id for t in r1.tokens] == [t.id for t in r2.tokens],
              decode="synthetic weights: max_symbols emissions on every frame"))
    m.close()


if __name__ == "__main__":
    main()
