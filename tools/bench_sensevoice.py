"""SenseVoice timings on synthetic weights at the published shape (50 + 20 SAN-M layers, output 512, 4 heads of 128, FFN 2048, FSMN
kernel 11, vocabulary 25055, 80 mels, LFR 7/6): 10 s rows at batch 1 / 8 / 32 / 64 and one 30 s row.  Per step: wall-clock ms per
generate_batch (upload, front end, encoder, fused head + arg-max, decode, download; the call returns after its one synchronisation), the
device-side split from the handle's event timers - front end, encoder, head - the launches of the call, audio seconds per second and
the achieved TFLOP/s against the DERIVED count (2 x (560 x 1536 + 69 x 512 x 1536 + 70 x (512 x 512 + 2 x 512 x 2048) + 512 x 25055)
= about 0.47 GFLOP a sequence row from the layer widths, the attention products not counted).  At batch 32 the same run also calls
forward on the same rows and records its head interval (the unfused head: logits to memory, log-softmax, in chunks of head_rows) next
to generate's fused one.  Median of `--runs` timed calls after `--warmup` warm-ups.  Appends one JSON line per step to
profiles/sensevoice/bench.jsonl.

Every step is a child process of its own under `timeout -k 10`; the first step that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"b1": (1, 10), "b8": (8, 10), "b32": (32, 10), "b64": (64, 10), "long": (1, 30)}


def one(step, runs, warmup, out):
    import numpy as np
    import mlx_audio_swift_amd as mas
    batch, seconds = STEPS[step]
    cfg = mas.SenseVoiceConfig(max_batch=batch, max_seconds=seconds, head_rows=1024)
    dev = mas.SenseVoiceModel.synthetic(cfg, seed=777)
    g = np.random.default_rng(batch)
    rows = [(0.1 * g.standard_normal(seconds * 16000)).astype(np.float32) for _ in range(batch)]
    wall, parts = [], []
    for i in range(warmup + runs):
        t0 = time.perf_counter()
        dev.generate_batch(rows)
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            wall.append(dt)
            parts.append(dev.timing())
    med = statistics.median
    launches = dev.launches
    e = cfg.encoder_conf
    D, Fd, L = e.output_size, e.linear_units, cfg.num_layers
    flop_row = 2.0 * (cfg.input_size * 3 * D + (L - 1) * D * 3 * D + L * (D * D + 2 * D * Fd) + D * cfg.vocab_size)
    T = int(dev.frames([seconds * 16000])[1][0])
    device_ms = med([sum(p) for p in parts])
    row = dict(shape="512/4x128/2048/50+20/k11/25055", step=step, seconds=seconds, batch=batch, runs=runs, warmup=warmup, generate_ms=med(wall),
               generate_ms_min=min(wall), generate_ms_max=max(wall), front_end_ms=med([p[0] for p in parts]),
               encoder_ms=med([p[1] for p in parts]), head_fused_ms=med([p[2] for p in parts]), launches=launches,
               audio_s_per_s=batch * seconds / (med(wall) / 1e3), derived_gflop_per_row=flop_row / 1e9,
               derived_tflops_on_device_time=batch * T * flop_row / (device_ms * 1e-3) / 1e12)
    if step == "b32":                                                 # the unfused head on the same rows, in the same run
        heads = []
        for i in range(1 + runs):
            dev.forward(rows)
            if i >= 1:
                heads.append(dev.timing()[2])
        row["head_unfused_ms"] = med(heads)
        row["forward_launches"] = dev.launches
    dev.close()
    print(json.dumps(row))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write(json.dumps(row) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", nargs="+", default=list(STEPS), choices=list(STEPS))
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a single step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensevoice", "bench.jsonl"))
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        one(a.one, a.runs, a.warmup, a.out)
        return 0
    for step in a.steps:
        r = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", step, "--runs",
                            str(a.runs), "--warmup", str(a.warmup), "--out", a.out])
        if r.returncode != 0:
            print(f"step {step} ended with status {r.returncode}: nothing further is started", file=sys.stderr)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
