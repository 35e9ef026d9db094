"""DeepFilterNet hop by hop without a GPU: the float64 stream reference against the offline reference (the boundary of the yardstick
included), the host logic of DeepFilterNetStreamer on a fake feed, the refusals and defaults, and the resource bounds of the kernels
csrc/deepfilternet_stream.hip instantiates."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlx_audio_swift_amd as mas  # noqa: E402
import deepfilternet_ref as R  # noqa: E402
import deepfilternet_stream_ref as SR  # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"


# ---------------------------------------------------------------------------------------------- the float64 reference
@pytest.mark.parametrize("name", ["S", "W"])
def test_stream_reference_agrees_with_offline_up_to_count(name):
    """x = 14 hops + 3 samples of bursts, pad_end_frames p = 3, H = 17, L = 2: count = (H - L) hop - (fft - hop) = 14 hop.

    Over [:count] the hop-by-hop reference and DeepFilterNetRef.forward(concat(x, zeros(p hop))) compute the same float64 sums in two
    orders, and differ in one more thing: the offline reference divides by sum w^2 of the engine's float32 window table, the streamer
    (as processChunk) does not.  The gate is therefore derived, not read off: max |1 / sum w^2 - 1| over the table (2.9e-7 for fft 192:
    the table's float32 rounding) relative to the peak, + 1e-12 for the float64 orders of summation.  Measured max |difference| / peak:
    S 1.6e-7, W 1.3e-7; with the division applied to the stream's output as well: S 3.5e-16, W 1.4e-16, gated at 1e-12 (float64
    rounding through ~30 layers with room to spare, six orders below the float32 unit; nothing else separates the two).

    Beyond count the two must differ: offline forward(x) zero-fills the look-ahead of its last frames, the streamer is fed zero audio,
    whose features are not zero (measured: 1.9e-4 of the peak on S, against a rounding gate of 2.9e-7; asserted above 100 gates, which
    rounding cannot explain).  That is the boundary in the yardstick, tested here rather than assumed."""
    cfg, W = R.case(name)
    hop, L, delay = cfg.hop_size, cfg.conv_lookahead, cfg.fft_size - cfg.hop_size
    x = R.rows(cfg)[7][: 14 * hop + 3]
    p = 3
    xe = np.concatenate([x, np.zeros(p * hop, np.float32)])
    H = len(xe) // hop
    count = (H - L) * hop - delay
    ref = R.DeepFilterNetRef(cfg, W)
    off = ref.forward(xe)
    st = SR.DeepFilterNetStreamRef(cfg, W)
    raw = SR.stream_all(st, x, p)
    assert len(raw) == (H - L) * hop and st.hops == H
    y = raw[delay:]
    peak = np.abs(off[25]).max()
    assert peak > 1e-3
    w2 = ref.win[:hop] ** 2 + ref.win[hop:] ** 2
    gate = np.abs(1.0 / w2 - 1.0).max() + 1e-12
    dist = np.abs(y[:count] - off[25][:count]).max() / peak
    exact = np.abs(y[:count] / np.tile(w2, count // hop) - off[25][:count]).max() / peak
    print(f"deepfilternet stream reference {name}: distance {dist:.3e} gate {gate:.3e}; with the division {exact:.3e}")
    assert dist <= gate and exact <= 1e-12, (dist, gate, exact)
    assert np.abs(np.stack(st.lsnr)[:, 0] - off[11][: H - L, 0]).max() <= 1e-9
    # the boundary: against the un-extended row, equal up to its own count, different behind it
    short = ref.forward(x)[25]
    cx = (len(x) // hop - L) * hop - delay
    assert np.abs(y[:cx] / np.tile(w2, cx // hop) - short[:cx]).max() / peak <= 1e-12
    n2 = min(len(short), len(y))
    assert n2 - cx >= hop and np.abs(y[cx: n2] - short[cx: n2]).max() / peak > 100 * gate


# ---------------------------------------------------------------------------------------------- host logic on a fake feed
class Model:
    def __init__(self, **kw):
        self.config = mas.DeepFilterNetConfig(fft_size=16, hop_size=8, nb_erb=4, nb_df=2, **kw)


class DelayFeed:
    """What the device does to the sample count: a stream's input, delayed by conv_lookahead hops; records every feed."""

    def __init__(self, streams, hop, L):
        self.hop, self.L, self.seen, self.buf, self.feeds = hop, L, [0] * streams, [np.zeros(0, np.float32) for _ in range(streams)], []

    def __call__(self, rows):
        outs, ls = [], []
        self.feeds.append([len(r) // self.hop for r in rows])
        for b, r in enumerate(rows):
            before = max(0, self.seen[b] - self.L)
            self.seen[b] += len(r) // self.hop
            self.buf[b] = np.concatenate([self.buf[b], r])
            after = max(0, self.seen[b] - self.L)
            outs.append(self.buf[b][before * self.hop: after * self.hop].copy())
            ls.append(np.arange(before, after, dtype=np.float32))
        return outs, ls


def streamer(streams=1, max_hops=4, **cfg):
    m = Model()
    feed = DelayFeed(streams, m.config.hop_size, m.config.conv_lookahead)
    return mas.DeepFilterNetStreamer(m, mas.DeepFilterNetStreamingConfig(**cfg), streams, max_hops, _feed=feed), feed


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("chunk", [1, 7, 8, 9, 7 * 8 + 5])
def test_pending_remainder_delay_and_count(chunk, pad):
    hop, L, delay = 8, 2, 8
    x = np.arange(1, 1 + 11 * hop + 5, dtype=np.float32)
    st, feed = streamer(pad_end_frames=pad)
    outs = [st.process_chunk(x[at: at + chunk]) for at in range(0, len(x), chunk)]
    assert all(max(f) <= 4 for f in feed.feeds)                           # a long chunk is walked in feeds of at most max_hops hops
    assert len(st._pending[0]) == len(x) % hop                            # the remainder below one hop waits
    outs.append(st.flush())
    y = np.concatenate(outs)
    H = (len(x) + pad * hop) // hop
    count = max(0, (H - L) * hop - delay)
    assert st.hops_seen == H and len(y) == count
    assert np.array_equal(y, np.concatenate([x, np.zeros(pad * hop, np.float32)])[delay: delay + count])
    assert len(st.last_lsnr[0]) <= pad + 1


def test_delay_drop_spans_small_chunks_and_can_be_switched_off():
    x = np.arange(1, 81, dtype=np.float32)
    st, _ = streamer()
    lens = [len(st.process_chunk(x[at: at + 4])) for at in range(0, 80, 4)]
    assert lens[:6] == [0, 0, 0, 0, 0, 0] and lens[6:9] == [0, 8, 0] and sum(lens) == (10 - 2) * 8 - 8
    st, _ = streamer(compensate_delay=False, pad_end_frames=0)
    y = np.concatenate([st.process_chunk(x), st.flush()])
    assert np.array_equal(y, x[: (10 - 2) * 8])


def test_flush_twice_reset_and_empty_chunk():
    x = np.arange(1, 8 * 5 + 4, dtype=np.float32)
    st, feed = streamer(pad_end_frames=3)
    assert st.process_chunk(np.zeros(0, np.float32)).size == 0 and feed.feeds == []       # an empty chunk feeds nothing
    a = st.process_chunk(x)
    b = st.flush()
    assert st.hops_seen == 5 + 3 and len(a) + len(b) == (8 - 2) * 8 - 8 and len(st._pending[0]) == 3
    c = st.flush()                                                        # as the reference: the remainder + another padding
    assert st.hops_seen == 11 and len(c) == 3 * 8 and len(st._pending[0]) == 3
    st.reset()
    feed.seen, feed.buf = [0], [np.zeros(0, np.float32)]
    assert st.hops_seen == 0 and len(st._pending[0]) == 0 and st._dropped == [0]
    y = np.concatenate([st.process_chunk(x), st.flush()])
    assert np.array_equal(y, np.concatenate([a, b]))


def test_process_chunks_serves_every_slot():
    st, feed = streamer(streams=3, pad_end_frames=0)
    x = np.arange(1, 65, dtype=np.float32)
    out = st.process_chunks([x[:24], None, x[:40]])
    assert out[1] is None and len(out[0]) == 0 and len(out[2]) == 16 and st.hops_seen == [3, 0, 5]
    assert feed.feeds == [[3, 0, 4], [0, 0, 1]]
    out = st.process_chunks([x[24:], x, None], is_last=[True, False, False])
    assert np.array_equal(out[0], x[8:48]) and np.array_equal(out[1], x[8:48]) and out[2] is None
    with pytest.raises(mas.AudioGenerationError):
        st.process_chunks([x])


def test_refusals_and_defaults():
    d = mas.DeepFilterNetStreamingConfig()
    assert (d.pad_end_frames, d.compensate_delay, d.enable_stage_skipping, d.min_db_thresh, d.max_db_erb_thresh, d.max_db_df_thresh,
            d.enable_profiling, d.profiling_force_eval_per_stage, d.materialize_every_hops) == (3, True, False, -10.0, 30.0, 20.0, False, False, 512)
    st, _ = streamer(enable_profiling=True, materialize_every_hops=7)                     # accepted and ignored
    with pytest.raises(mas.DeepFilterNetError) as e:
        st.process_chunk(np.zeros((2, 8), np.float32))
    assert e.value.sts_case == "invalidAudioShape"
    with pytest.raises(mas.AudioGenerationError) as e:
        streamer(enable_stage_skipping=True)
    assert "stage_skipping" in str(e.value) and "host decision" in str(e.value)
    for kw, word in ((dict(fft_size=16, hop_size=4), "fft_size"), (dict(df_lookahead=3, conv_lookahead=2), "df_lookahead")):
        m = Model()
        for k, v in kw.items():
            setattr(m.config, k, v)
        with pytest.raises(mas.AudioGenerationError) as e:
            mas.DeepFilterNetStreamer(m, None, 1, 4, _feed=lambda rows: None)
        assert word in str(e.value)
    with pytest.raises(mas.DeepFilterNetError) as e:
        mas.deepfilternet_enhance_streaming(Model(), np.zeros((2, 8), np.float32))
    assert e.value.sts_case == "invalidAudioShape"
    assert not hasattr(mas.DeepFilterNet, "create_streamer")              # the class keeps its surface; the streamer is its own class


# ---------------------------------------------------------------------------------------------- resources
@pytest.fixture(scope="module")
def usage():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S",
                            os.path.join(ROOT, "mlx-audio-swift_amd", "csrc", "deepfilternet_stream.hip"), "-o", os.path.join(td, "k.s"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    use, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = use.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for key, pat in (("vgprs", r"remark:\s+VGPRs: (\d+)"), ("agprs", r"remark:\s+AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m:
                cur[key] = int(m.group(1))
    return use


def test_stream_kernels_do_not_spill(usage):
    """Every kernel of deepfilternet_stream.hip: scratch 0, LDS within 64 KiB, and the recurrence within the register budget of its block
    (3 H threads: at H = 256 three waves a SIMD, 168 registers).  The short-chunk form (KR = 0) keeps no slice of Wh: its registers are
    the 32 loads in flight, so it stays under 128 (four waves a SIMD) at every hidden size."""
    mine = {k: v for k, v in usage.items() if "k_dfn_" in k}
    gru = {tuple(int(g) for g in re.search(r"k_dfn_gruILi(\d+)ELi(\d+)ELb1E", k).groups()): v for k, v in mine.items() if "k_dfn_gru" in k}
    assert sorted(gru) == [(32, 0), (32, 32), (64, 0), (64, 64), (128, 0), (128, 128), (256, 0), (256, 64), (256, 96), (256, 128)]
    assert len(mine) == len(gru) + 5                                      # gemm, norm, enh in their stream form, ola_stream, roll
    for k, v in mine.items():
        assert v["scratch"] == 0 and v["lds"] <= 65536 and v["vgprs"] + v["agprs"] <= 512, (k, v)
    for (H, KR), v in gru.items():
        waves_per_simd = -(-(3 * H // 64) // 4) if 3 * H >= 64 else 1
        budget = min(512, (512 // waves_per_simd) // 8 * 8)
        assert KR < v["vgprs"] + v["agprs"] <= (128 if KR == 0 else budget), (H, KR, v, budget)
        assert v["lds"] == 16 * H
