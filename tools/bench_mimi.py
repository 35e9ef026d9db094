"""Mimi codec bench (mimi_202407 widths, synthetic weights): whole decode of B x 10 s (125 frames, 32 codebooks) in audio-s/s, the
stream at batch 1 in ms per 80 ms frame (single-frame steps, as MimiStreamingDecoder.decodeFrames runs them), and encode of 10 s rows
in audio-s/s.  Codes and pcm stay on the device (the entry points take device pointers), so the figures are the codec's own time plus
the per-call host synchronisation.  One JSON line."""
import argparse, json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mlx_audio_swift_amd as mas
from mlx_audio_swift_amd.generation import check

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--frames", type=int, default=125)
ap.add_argument("--nq", type=int, default=32)
ap.add_argument("--stream-frames", type=int, default=100)
ap.add_argument("--encode-rows", type=int, default=4)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
lib = mas._lib.lib()
cfg = mas.MimiConfig(num_codebooks=32)
m = mas.Mimi.synthetic(cfg, seed=77)
spf = m.num_samples(1)
dev = torch.device("cuda:0")
rng = np.random.default_rng(3)
B, T, nq = args.batch, args.frames, args.nq


def best_of(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return min(ts), float(np.median(ts))


codes = torch.from_numpy(rng.integers(0, cfg.bins, (B, nq, T)).astype(np.int32)).to(dev)
pcm = torch.empty(B, T * spf, dtype=torch.float32, device=dev)
torch.cuda.synchronize()
dec_best, dec_med = best_of(lambda: check(lib.mis_mimi_decode(m._h, codes.data_ptr(), B, nq, T, pcm.data_ptr())), args.reps)
audio_s = B * T * spf / cfg.sample_rate

sc = torch.from_numpy(rng.integers(0, cfg.bins, (1, nq, args.stream_frames)).astype(np.int32)).to(dev)
frames = [sc[:, :, f:f + 1].contiguous() for f in range(args.stream_frames)]
out = torch.empty(spf, dtype=torch.float32, device=dev)
check(lib.mis_mimi_decode_stream_begin(m._h, 1))
for f in frames[:10]:
    check(lib.mis_mimi_decode_stream_step(m._h, f.data_ptr(), nq, 1, out.data_ptr()))
check(lib.mis_mimi_decode_stream_begin(m._h, 1))
t0 = time.perf_counter()
for f in frames:
    check(lib.mis_mimi_decode_stream_step(m._h, f.data_ptr(), nq, 1, out.data_ptr()))
stream_ms = (time.perf_counter() - t0) * 1e3 / len(frames)
check(lib.mis_mimi_decode_stream_end(m._h))

n = 10 * cfg.sample_rate
audio = torch.from_numpy((0.3 * rng.standard_normal((args.encode_rows, n))).astype(np.float32)).to(dev)
nf = m.encode_num_frames(n)
ecodes = torch.empty(args.encode_rows, nq, nf, dtype=torch.int32, device=dev)
enc_best, _ = best_of(lambda: check(lib.mis_mimi_encode(m._h, audio.data_ptr(), args.encode_rows, n, nq, ecodes.data_ptr())), 3)

print(json.dumps({"workload": f"Mimi mimi_202407 synthetic, decode {B} x {T} frames x {nq} codebooks, stream batch 1, encode "
                              f"{args.encode_rows} x 10 s",
                  "decode_ms": dec_best * 1e3, "decode_ms_median": dec_med * 1e3, "decode_audio_s_per_s": audio_s / dec_best,
                  "stream_ms_per_frame": stream_ms, "stream_frames": len(frames),
                  "encode_ms": enc_best * 1e3, "encode_audio_s_per_s": args.encode_rows * 10.0 / enc_best,
                  "pcm_checksum": float(pcm.double().abs().sum().item())}))
