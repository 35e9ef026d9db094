"""DeepFilterNet hop by hop at the published DeepFilterNet3 shape with synthetic weights -> profiles/deepfilternet_stream/bench.jsonl.

    python tools/bench_deepfilternet_stream.py [--out profiles/deepfilternet_stream/bench.jsonl]

1. Feeds: 1 / 8 / 32 / 64 streams x 1 / 4 / 16 hops a stream and feed, every stream past its look-ahead.  Median of 5 feeds after 2
   warm-ups: wall-clock of DeepFilterNetStreamer.feed_hops (packing, copy in, device, copy out), device milliseconds of the feed and of
   its recurrence launches, launches a feed.  The real-time budget is one hop, hop_size / sample_rate = 10 ms: `realtime_streams` is the
   largest measured stream count whose 1-hop feed stays under it (no target fixed in advance).
2. The two forms of the recurrence, hidden size 256: microseconds a launch (recurrence interval of a feed / its recurrence launches) at
   1, 2, 4, 8, 16, 32 frames a feed on 1 stream and on 64, the short-chunk form (every column of Wh streamed) against the offline form
   (a register slice of KR columns filled first).  The threshold in csrc/deepfilternet_stream.hip is read from this table.
Context: the offline engine takes 17.4 ms for one 10 s row (profiles/deepfilternet/bench.jsonl), 17.4 us a frame."""
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

CONTEXT = dict(offline_10s_b1_ms=17.4, offline_frame_us=17.4)


def rec_launches(model):
    _, lr, ld = model.layers
    return model.layers[0] + (max(lr, ld) if model.config.emb_hidden_dim == model.config.df_hidden_dim else lr + ld)


def feeds(st, streams, hops, rng):
    """2 warm-ups + 5 measured feeds of `hops` hops a stream -> (wall ms, device ms, recurrence ms), a list each."""
    hop = st.hop
    wall, dev, rec = [], [], []
    for i in range(7):
        rows = [(0.05 * rng.standard_normal(hops * hop)).astype(np.float32) for _ in range(streams)]
        t0 = time.perf_counter()
        out, _ = st.feed_hops(rows)
        if i >= 2:
            wall.append((time.perf_counter() - t0) * 1e3)
            d, r = st.timing()
            dev.append(d), rec.append(r)
    assert all(len(o) == hops * hop and np.isfinite(o).all() for o in out)
    return wall, dev, rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deepfilternet_stream", "bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    cfg = mas.DeepFilterNetConfig(max_batch=64, max_seconds=1.0)
    model = mas.DeepFilterNet.synthetic(cfg)
    budget_ms = 1e3 * cfg.hop_size / cfg.sample_rate
    rng = np.random.default_rng(100)
    lines, realtime = [], 0
    for streams in (1, 8, 32, 64):
        st = mas.DeepFilterNetStreamer(model, None, streams, 16)
        st.feed_hops([np.zeros(4 * st.hop, np.float32)] * streams)          # past the look-ahead: every feed below has targets
        for hops in (1, 4, 16):
            wall, dev, rec = feeds(st, streams, hops, rng)
            line = dict(case=f"feed_s{streams}_h{hops}", streams=streams, hops_per_feed=hops, weights="synthetic", feed_ms_median=statistics.median(wall),
                        feed_ms_min=min(wall), feed_ms_max=max(wall), device_ms_median=statistics.median(dev),
                        device_recurrence_ms_median=statistics.median(rec), launches=st.launches, budget_ms=budget_ms * hops,
                        within_budget=statistics.median(wall) < budget_ms * hops, context=CONTEXT)
            if hops == 1 and line["within_budget"]:
                realtime = max(realtime, streams)
            print(json.dumps(line), flush=True)
            lines.append(line)
        st.close()
    line = dict(case="realtime_streams", hops_per_feed=1, budget_ms=budget_ms, realtime_streams=realtime, measured_stream_counts=[1, 8, 32, 64])
    print(json.dumps(line), flush=True)
    lines.append(line)
    for streams in (1, 64):
        st = mas.DeepFilterNetStreamer(model, None, streams, 32)
        st.feed_hops([np.zeros(4 * st.hop, np.float32)] * streams)
        for frames in (1, 2, 4, 8, 16, 32):
            us = {}
            for form, thr in (("step", 64), ("offline", 0)):
                st.set_gru_step_frames(thr)
                _, _, rec = feeds(st, streams, frames, rng)
                us[form] = statistics.median(rec) * 1e3 / rec_launches(model)
            line = dict(case=f"gru_s{streams}_t{frames}", hidden=cfg.emb_hidden_dim, gru_kr=96, streams=streams, frames=frames,
                        recurrence_launches=rec_launches(model), step_form_us_per_launch=us["step"], offline_form_us_per_launch=us["offline"])
            print(json.dumps(line), flush=True)
            lines.append(line)
        st.close()
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
