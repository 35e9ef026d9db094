"""Wall-clock of FSMNVAD.detect at the published shape with synthetic weights -> profiles/fsmn_vad/bench.jsonl.

    python tools/bench_fsmn_vad.py [--out profiles/fsmn_vad/bench.jsonl]

Cases: 10 s rows at batch 1, 8 and 32, and one 10-minute row at batch 1 (the chunked path, chunk_frames 3000).  Median of 5 runs after
2 warm-ups of detect_batch (copy in, device, copy out, host state machine).  Each line also carries the split of the last run: device
milliseconds of the front end and of the encoder (events around each chunk's copy in + fbank and encoder + copy out), wall-clock of
the host state machine, and the launch count.  Noise bursts in silence, so the state machine opens and closes segments."""
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


def row(seconds, seed):
    rng = np.random.default_rng(seed)
    x = np.zeros(int(seconds * 16000), np.float32)
    for start in np.arange(0.5, seconds, 4.0):
        a, b = int(start * 16000), min(int((start + 2.5) * 16000), len(x))
        x[a:b] = 0.1 * rng.standard_normal(b - a).astype(np.float32)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fsmn_vad", "bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    cfg = mas.FSMNVADConfig(max_batch=32)
    model = mas.FSMNVAD.synthetic(cfg)
    lines = []
    for name, seconds, batch in (("10s_b1", 10, 1), ("10s_b8", 10, 8), ("10s_b32", 10, 32), ("600s_b1", 600, 1)):
        rows = [row(seconds, 100 + i) for i in range(batch)]
        wall = []
        for i in range(7):
            t0 = time.perf_counter()
            segs = model.detect_batch(rows)
            if i >= 2:
                wall.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        sil, dec, R, T = model.detect_raw(rows)
        raw_ms = (time.perf_counter() - t0) * 1e3
        front_ms, enc_ms = model.timing()
        launches = model.launches
        t0 = time.perf_counter()
        for b in range(batch):
            mas.fsmn_vad_postprocess(sil[b, : R[b]], dec[b, : T[b]], len(rows[b]), cfg)
        host_ms = (time.perf_counter() - t0) * 1e3
        line = dict(case=name, seconds=seconds, batch=batch, weights="synthetic", detect_ms_median=statistics.median(wall), detect_ms_min=min(wall),
                    detect_ms_max=max(wall), detect_raw_ms=raw_ms, device_front_ms=front_ms, device_encoder_ms=enc_ms,
                    host_state_machine_ms=host_ms, launches=launches, chunk_frames=cfg.chunk_frames, segments_row0=len(segs[0]))
        print(json.dumps(line))
        lines.append(line)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
