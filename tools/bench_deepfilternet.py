"""Wall-clock of DeepFilterNet.enhance_batch at the published DeepFilterNet3 shape with synthetic weights -> profiles/deepfilternet/bench.jsonl.

    python tools/bench_deepfilternet.py [--out profiles/deepfilternet/bench.jsonl]

Cases: 10 s rows at batch 1 / 8 / 32, and one 60 s row; noise bursts on a noise floor.  Median of 5 runs after 2 warm-ups of
enhance_batch (copy in, device, copy out).  Each line carries the four device intervals of the last run (front end, network without
the recurrences, recurrences, synthesis), the launch count and the microseconds per GRU step (recurrence interval / (recurrence
launches x frames of the longest row)).  Then one 10 s row for every candidate KR of the recurrence kernel (the columns of Wh a thread
keeps in registers): microseconds per step, median of 5.  Context, not gates: Silero's LSTM step takes 1.4 us, MossFormer2-SE 23.4 ms
for one 10 s row (README.md)."""
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

CONTEXT = dict(silero_lstm_step_us=1.4, mossformer2_10s_b1_ms=23.4)


def noise_bursts(n, hop, rng):
    x = 0.01 * rng.standard_normal(n)
    for s in range(0, n, 50 * hop):
        m = min(20 * hop, n - s)
        x[s: s + m] += 0.3 * rng.standard_normal(m) * np.hanning(m)
    return x.astype(np.float32)


def rec_launches(model):
    _, lr, ld = model.layers
    return model.layers[0] + (max(lr, ld) if model.config.emb_hidden_dim == model.config.df_hidden_dim else lr + ld)


def run(model, rows):
    wall, rec = [], []
    for i in range(7):
        t0 = time.perf_counter()
        out = model.enhance_batch(rows)
        if i >= 2:
            wall.append((time.perf_counter() - t0) * 1e3)
            rec.append(model.timing()[2])
    return out, wall, rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deepfilternet", "bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    lines = []
    for name, seconds, batch in (("10s_b1", 10, 1), ("10s_b8", 10, 8), ("10s_b32", 10, 32), ("60s_b1", 60, 1)):
        cfg = mas.DeepFilterNetConfig(max_batch=batch, max_seconds=float(seconds))
        model = mas.DeepFilterNet.synthetic(cfg)
        rng = np.random.default_rng(100)
        rows = [noise_bursts(seconds * cfg.sample_rate, cfg.hop_size, rng) for _ in range(batch)]
        out, wall, rec = run(model, rows)
        front, net, rec_ms, synth = model.timing()
        T = int(model.frames([len(rows[0])])[0][0])
        line = dict(case=name, seconds=seconds, batch=batch, weights="synthetic", frames=T, enhance_ms_median=statistics.median(wall),
                    enhance_ms_min=min(wall), enhance_ms_max=max(wall), device_front_ms=front, device_network_ms=net,
                    device_recurrence_ms=rec_ms, device_synthesis_ms=synth, launches=model.launches, recurrence_launches=rec_launches(model),
                    gru_step_us=statistics.median(rec) * 1e3 / (rec_launches(model) * T), finite=bool(np.isfinite(out[0]).all()), context=CONTEXT)
        print(json.dumps(line), flush=True)
        lines.append(line)
        model.close()
    for kr in (64, 96, 128):
        for batch in (1, 32):
            cfg = mas.DeepFilterNetConfig(max_batch=batch, max_seconds=10.0, gru_kr=kr)
            model = mas.DeepFilterNet.synthetic(cfg)
            rng = np.random.default_rng(100)
            rows = [noise_bursts(10 * cfg.sample_rate, cfg.hop_size, rng) for _ in range(batch)]
            _, wall, rec = run(model, rows)
            T = int(model.frames([len(rows[0])])[0][0])
            line = dict(case=f"kr{kr}_10s_b{batch}", gru_kr=kr, hidden=cfg.emb_hidden_dim, batch=batch, frames=T, recurrence_launches=rec_launches(model),
                        device_recurrence_ms_median=statistics.median(rec), gru_step_us=statistics.median(rec) * 1e3 / (rec_launches(model) * T),
                        enhance_ms_median=statistics.median(wall))
            print(json.dumps(line), flush=True)
            lines.append(line)
            model.close()
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
