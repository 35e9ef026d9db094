"""The Nemotron stream session at the published shape with synthetic weights.  Median of 5 after 2 warm-ups (a warm-up and a run are each one
feed of one native chunk, 80 (right + 1) ms of audio a stream, on streams that already hold a full left context): wall clock of the feed (it
ends in the feed's one synchronisation) and its device time, at 1 / 8 / 32 / 64 streams for the right contexts 0, 1, 3, 6, 13, beside the
budget - the chunk's own duration; k_nm_attn_stream alone on the last chunk of a 70-frame row against k_nm_attn on the whole row; and the
same 10 s row through transcribe_streaming and through offline generate.  Synthetic weights emit max_symbols tokens on every frame: the
decode share is that worst case, as in tools/bench_nemotron.py.  Appended to profiles/nemotron_stream/bench.jsonl.  Nothing is gated.  Needs a
GPU; there is no fallback.

--encoder-dtype bfloat16 / both: the bf16 session (csrc/nemotron_stream_bf16.h) on a model finalized in bf16 mode; `both` runs the f32 and
the bf16 session in one process on the same feeds, with each feed's device time split into the decode launch and the rest, then the
short-pass contraction alone per role, live-row count and rule against the 64 x 64 rule, and the attention launch alone against
k_nm_attn_stream.  These rows go to profiles/nemotron_stream_bf16/bench.jsonl."""
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


def _bf16(a):
    """float32 array -> bf16 bits, round to nearest even"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def attention_alone_bf16(repeat):
    """one chunk of 14 queries behind a full left context, 1 and 64 streams: k_nm_attn_stream (f32) and k_nm_attn_stream_bf16"""
    H, hd, left, right, Rr, Tp = 8, 128, 56, 13, 128, 16
    w, rng, Cs, lib, p = H * hd, np.random.default_rng(1), right + 1, mas._lib.lib(), lambda a: a.ctypes.data
    table = rng.standard_normal((2 * 70 - 1, w)).astype(np.float32)
    u, v = (rng.uniform(-0.5, 0.5, (H, hd)).astype(np.float32) for _ in range(2))
    for S in (1, 64):
        q, ring = rng.standard_normal((S, Tp, w)).astype(np.float32), rng.standard_normal((S, Rr, 2 * w)).astype(np.float32)
        n, pos, ms, ms16 = np.full(S, Cs, np.int32), np.full(S, 56, np.int32), C.c_float(0), C.c_float(0)
        o, o16 = np.zeros((S, Tp, w), np.float32), np.zeros((S, Tp, w), np.uint16)
        check(lib.mis_debug_nemotron_attn_stream(0, p(q), p(ring), Rr, p(n), p(pos), S, Tp, H, hd, 1.0, float(np.sqrt(hd)), p(u), p(v), p(table), w, 139, 69, left,
                                                 right, p(o), repeat, C.byref(ms)))
        q16, r16, t16 = _bf16(q), _bf16(ring), _bf16(table)
        check(lib.mis_debug_nemotron_attn_stream_bf16(0, p(q16), p(r16), Rr, p(n), p(pos), S, Tp, H, hd, 1.0, float(np.sqrt(hd)), p(u), p(v), p(t16), w, 139, 69,
                                                      left, right, p(o16), repeat, C.byref(ms16)))
        yield dict(bench="nemotron_attn_stream_alone_bf16", streams=S, queries=Cs, heads=H, head_size=hd, f32_ms=float(ms.value), bf16_ms=float(ms16.value))


def contraction_alone(repeat):
    """the block's K = d and K = 4 d roles at d = 1024, per live-row count: rule 0 (k_pk_gemm_bf16, 64 x 64) and the short-pass rules 2 / 3 / 4"""
    d, rng, lib, p = 1024, np.random.default_rng(2), mas._lib.lib(), lambda a: a.ctypes.data
    roles = dict(qkv=(1, 0, 3 * d, d), ff1a=(1, 1, 4 * d, d), o=(0, 2, d, d), ff1b=(0, 2, d, 4 * d))     # load, epilogue, N, K
    for name, (load, epi, N, K) in roles.items():
        wb, bias, lnw, lnb = _bf16(rng.standard_normal((N, K)) / K ** 0.5), np.zeros(N, np.float32), np.ones(K, np.float32), np.zeros(K, np.float32)
        for B, n, Tp in ((1, 1, 16), (1, 14, 16), (64, 1, 16), (16, 14, 16), (64, 14, 16), (1, 44, 44), (4, 44, 44), (8, 44, 44), (16, 44, 44), (32, 44, 44),
                          (64, 44, 44)):
            x = rng.standard_normal((B, Tp, K)).astype(np.float32)
            xa, st, res = x if load == 1 else _bf16(x), np.tile(np.asarray([0.0, 1.0], np.float32), (B, Tp, 1)), np.zeros((B, Tp, N), np.float32)
            cnt, out, row = np.full(B, n, np.int32), np.zeros((B, Tp, N), np.float32 if epi == 2 else np.uint16), {}
            for rule in (0, 2, 3, 4):
                ms = C.c_float(0)
                check(lib.mis_debug_nemotron_gemm_bf16(0, load, epi, rule, p(xa), p(st), p(lnw), p(lnb), p(wb), p(bias), p(res), 0.5, p(cnt), B, Tp, K, N, p(out),
                                                       repeat, C.byref(ms)))
                row[f"rule{rule}_us"] = 1e3 * float(ms.value)
            yield dict(bench="nemotron_gemm_rows_alone", role=name, N=N, K=K, entries=B, live_rows=B * n, Tp=Tp, **row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8, 32, 64])
    ap.add_argument("--rights", type=int, nargs="*", default=[0, 1, 3, 6, 13], help="the right contexts of the feed table (none: the kernels alone)")
    ap.add_argument("--encoder-dtype", choices=["float32", "bfloat16", "both"], default="float32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dtypes = ["float32", "bfloat16"] if a.encoder_dtype == "both" else [a.encoder_dtype]
    a.out = a.out or os.path.join(ROOT, "profiles", "nemotron_stream" if dtypes == ["float32"] else "nemotron_stream_bf16", "bench.jsonl")
    if mas._lib.lib().mis_device_count() < 1:
        raise SystemExit("bench_nemotron_stream needs a GPU")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)

    def emit(row):
        print(json.dumps(row), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")

    med = lambda xs: float(statistics.median(xs))
    rights = tuple(a.rights)
    cfg = mas.NemotronConfig(num_hidden_layers=a.layers, max_batch=1, max_seconds=10, max_tokens=8192, max_symbols=10,
                             att_context_size=[[56, r] for r in (rights or (13,))[::-1]])
    models = {dt: mas.NemotronASR.synthetic(cfg, seed=7, encoder_dtype=dt) for dt in dtypes}
    m = models[dtypes[0]]
    for right in rights:
        chunk = 1280 * (right + 1)
        for S in a.streams:
            waves = [test_wave(100 + b, chunk * (a.warmup + a.runs + 1) + 1280 * 57) for b in range(S)]
            for dt in dtypes:                                              # the same feeds through each kind of session
                s = mas.NemotronStreamSession(models[dt], S, att_context_size=(56, right), max_pass_frames=right + 1, encoder_dtype=dt)
                s.decode_timing()
                at = 1280 * 57 + 256                                       # the left context is full before anything is timed
                for lo in range(0, at, 1280 * 14):
                    s.feed_raw([w[lo:min(lo + 1280 * 14, at)] for w in waves])
                wall, dev, dec, toks = [], [], [], 0
                for i in range(a.warmup + a.runs):
                    t0 = time.perf_counter()
                    out = s.feed_raw([w[at:at + chunk] for w in waves])
                    dt_ms = (time.perf_counter() - t0) * 1e3
                    at += chunk
                    if i >= a.warmup:
                        wall.append(dt_ms); dev.append(s.timing()); dec.append(s.decode_timing()); toks = max(len(o[0]) for o in out)
                emit(dict(bench="nemotron_stream_feed", encoder_dtype=dt, layers=a.layers, streams=S, context=[56, right], budget_ms=80 * (right + 1),
                          launches=s.launches, wall_ms=med(wall), wall_min_ms=min(wall), wall_max_ms=max(wall), device_ms=med(dev), decode_ms=med(dec),
                          encoder_and_rest_ms=med(dev) - med(dec), tokens_a_feed_max=toks, decode="synthetic weights: max_symbols emissions on every frame"))
                s.close()
    if "bfloat16" in dtypes:
        for row in list(contraction_alone(20)) + list(attention_alone_bf16(20)):
            emit(row)
    if dtypes[0] != "float32":
        for mm in models.values():
            mm.close()
        return
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
