"""DeepFilterNet hop by hop on the GPU.  The yardstick is the offline engine itself: a stream fed any chunking and flushed returns the
first count = (H - L) hop - (fft - hop) samples of DeepFilterNet.enhance on the zero-extended samples and the lsnr of frames 0..H-1-L,
bit for bit (np.array_equal on the uint32 views).  Independence across slots, ragged feeds, reset and interleaved enhance calls are
held to the same equality; the float64 stream reference (tests/deepfilternet_stream_ref.py) is held to the gate the offline chained test
uses, 4 x the float32 reference's own distance to float64 + 2^-23.  With MIS_DEEPFILTERNET_STREAM_PARITY_LOG=<file> the observed
distances are appended as JSON lines."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlx_audio_swift_amd as mas  # noqa: E402
import deepfilternet_ref as R  # noqa: E402
import deepfilternet_stream_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -23
MAX_HOPS = 16


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Bundle:
    def __init__(self, name, **kw):
        self.name = name
        self.cfg, self.W = R.case(name, **kw)
        self.model = mas.DeepFilterNet.from_weights(self.cfg, self.W)
        self.hop, self.L, self.delay = self.cfg.hop_size, self.cfg.conv_lookahead, self.cfg.fft_size - self.cfg.hop_size
        rows = R.rows(self.cfg)
        self.row, self.zero = rows[7], rows[6]                            # 40 hops + 3 samples of bursts; the all-zero row
        self._off = {}

    def offline(self, x, pad):
        """enhance(concat(x, zeros(pad hop))), its lsnr, H and count; computed once a (row, pad)."""
        key = (x.tobytes(), pad)
        if key not in self._off:
            xe = np.concatenate([x, np.zeros(pad * self.hop, np.float32)])
            wav, lsnr = self.model.enhance_raw([xe])
            H = len(xe) // self.hop
            self._off[key] = (wav[0], lsnr[0], H, max(0, (H - self.L) * self.hop - self.delay))
        return self._off[key]

    def stream(self, x, chunk, pad=3, compensate=True, streams=1, slot=0, thr=None, max_hops=MAX_HOPS):
        """One stream in `slot`, fed in chunks of `chunk` samples and flushed -> (samples, lsnr, the streamer's hop count)."""
        st = mas.DeepFilterNetStreamer(self.model, mas.DeepFilterNetStreamingConfig(pad_end_frames=pad, compensate_delay=compensate), streams, max_hops)
        if thr is not None:
            st.set_gru_step_frames(thr)
        outs, ls = [], []

        def one(c, last):
            chunks = [None] * streams
            chunks[slot] = c
            outs.append(st.process_chunks(chunks, last)[slot]), ls.append(st.last_lsnr[slot])

        for at in range(0, len(x), chunk):
            one(x[at: at + chunk], False)
        one(np.zeros(0, np.float32), True)
        seen = st.hops_seen if streams == 1 else st.hops_seen[slot]
        st.close()
        return np.concatenate(outs), np.concatenate(ls), seen


@pytest.fixture(scope="module")
def bundles():
    return {"S": Bundle("S"), "W": Bundle("W")}


# ---------------------------------------------------------------------------------------------- 1. bit identity with enhance
@pytest.mark.parametrize("name", ["S", "W"])
def test_stream_equals_offline_bit_for_bit(bundles, name):
    bd = bundles[name]
    hop = bd.hop
    for x in (bd.row, bd.zero):
        for pad in (0, 3):
            wav, lsnr, H, count = bd.offline(x, pad)
            for chunk in (hop, 3 * hop, MAX_HOPS * hop, 1, hop - 1, hop + 1, 7 * hop + 5):
                if x is bd.zero and chunk not in (hop, 7 * hop + 5):
                    continue
                y, l, seen = bd.stream(x, chunk, pad)
                assert seen == H and len(y) == count and len(l) == H - bd.L, (name, pad, chunk, seen, H, len(y), count)
                assert same(y, wav[:count]) and same(l, lsnr[: H - bd.L]), (name, pad, chunk)
            y, l, _ = bd.stream(x, 3 * hop, pad, compensate=False)       # the first fft - hop raw samples in front
            assert len(y) == count + bd.delay and same(y[bd.delay:], wav[:count]) and np.isfinite(y).all() and np.abs(y).max() <= 1.0
    assert np.abs(bd.offline(bd.row, 3)[0]).max() > 1e-3


# ---------------------------------------------------------------------------------------------- 2. independence
@pytest.mark.parametrize("name", ["S", "W"])
def test_streams_do_not_depend_on_their_neighbours(bundles, name):
    bd = bundles[name]
    hop, B = bd.hop, 8
    rng = np.random.default_rng(11)
    rows = [R.rows(bd.cfg, seed=20 + b)[7][: (18 + b) * hop] for b in range(B)]
    single = [bd.stream(r, 2 * hop, pad=0) for r in rows]                 # every stream alone, in slot 0
    st = mas.DeepFilterNetStreamer(bd.model, mas.DeepFilterNetStreamingConfig(pad_end_frames=0), B, MAX_HOPS)
    at, outs, ls, feed = [0] * B, [[] for _ in range(B)], [[] for _ in range(B)], 0
    while any(at[b] < len(rows[b]) for b in range(B)):
        take = [int(rng.integers(0, 5)) * hop for _ in range(B)]          # 0..4 hops a stream and feed, some of them 0
        if feed == 3:
            assert same(bd.model.enhance(bd.row), bd.offline(bd.row, 0)[0])                  # enhance between two feeds
        if feed == 5:                                                     # stream 2 starts over while the others continue
            st.reset(2)
            at[2], outs[2], ls[2] = 0, [], []
        feed += 1
        part = [rows[b][at[b]: at[b] + take[b]] for b in range(B)]
        o, l = st.feed_hops(part, junk=np.nan)                            # junk behind a stream's hops in pcm
        for b in range(B):
            if len(part[b]) == 0:
                assert len(o[b]) == 0 and len(l[b]) == 0, b               # a stream that brings nothing returns nothing
            at[b] += len(part[b]); outs[b].append(o[b]); ls[b].append(l[b])
    for b in range(B):
        y, l = np.concatenate(outs[b])[bd.delay:], np.concatenate(ls[b])
        assert same(y, single[b][0]) and same(l, single[b][1]), (name, b)
        assert st.hops_seen[b] == len(rows[b]) // hop
    st.close()
    y, l, _ = bd.stream(rows[3], 2 * hop, pad=0, streams=5, slot=4)       # the same stream in another slot
    assert same(y, single[3][0]) and same(l, single[3][1])


# ---------------------------------------------------------------------------------------------- 3. both recurrence forms
@pytest.mark.parametrize("name", ["S", "W"])
def test_both_recurrence_forms_give_the_same_bits(bundles, name):
    """The threshold is 4 targets a feed: feeds of 4 and 5 hops lie on either side of it, and a ragged feed of (1, 6) hops runs the
    offline form for a stream that alone would run the short-chunk form; W has two-layer chains.  Forcing either form changes nothing."""
    bd = bundles[name]
    hop = bd.hop
    wav, lsnr, H, count = bd.offline(bd.row, 3)
    for chunk in (4 * hop, 5 * hop):
        for thr in (None, 0, 64):
            y, l, _ = bd.stream(bd.row, chunk, 3, thr=thr)
            assert same(y, wav[:count]) and same(l, lsnr[: H - bd.L]), (name, chunk, thr)
    st = mas.DeepFilterNetStreamer(bd.model, mas.DeepFilterNetStreamingConfig(pad_end_frames=0), 2, MAX_HOPS)
    a, b = bd.row[: 36 * hop], R.rows(bd.cfg, seed=9)[7][: 36 * hop]
    oa, ob, pa, pb = [], [], 0, 0
    for i in range(12):                                                   # stream 0 brings 1 or 6 hops, stream 1 the other
        na, nb = (1, 6) if i % 2 == 0 else (6, 1)
        na, nb = min(na, 36 - pa), min(nb, 36 - pb)
        o, _ = st.feed_hops([a[pa * hop: (pa + na) * hop], b[pb * hop: (pb + nb) * hop]])
        oa.append(o[0]); ob.append(o[1]); pa += na; pb += nb
    st.close()
    for x, o in ((a, oa), (b, ob)):
        got = np.concatenate(o)[bd.delay:]
        assert len(got) > 20 * hop and same(got, bd.offline(x, 0)[0][: len(got)]), name


# ---------------------------------------------------------------------------------------------- 4. a long stream
def test_long_stream_of_single_hops():
    bd = Bundle("S", max_batch=1, max_seconds=6.1)
    x = R.rows(bd.cfg, long_frames=3000)[5][: 3000 * bd.hop]
    wav, lsnr, H, count = bd.offline(x, 0)
    st = mas.DeepFilterNetStreamer(bd.model, mas.DeepFilterNetStreamingConfig(pad_end_frames=0), 1, 1)
    outs = [st.feed_hops([x[h * bd.hop: (h + 1) * bd.hop]])[0][0] for h in range(3000)]
    y = np.concatenate(outs)[bd.delay:]
    assert H == 3000 and st.hops_seen == 3000 and len(y) == count and same(y, wav[:count])
    st.close()


# ---------------------------------------------------------------------------------------------- 5. the published shape
def test_published_shape_hop_by_hop():
    bd = Bundle("P", max_seconds=12.5 * 480 / 48000)
    x = R.rows(bd.cfg, long_frames=12)[5][: 12 * bd.hop]
    wav, lsnr, H, count = bd.offline(x, 0)
    y, l, seen = bd.stream(x, bd.hop, pad=0, max_hops=1)
    assert seen == H == 12 and len(y) == count == 9 * bd.hop and same(y, wav[:count]) and same(l, lsnr[: H - bd.L])
    assert np.abs(y).max() > 1e-4


# ---------------------------------------------------------------------------------------------- 6. launches
def test_launch_count(bundles):
    """A feed with targets: the offline chain + the roll.  Before the look-ahead has filled: analysis [+ erb_fb] + features + the roll.
    A feed without a hop: nothing."""
    for name, fb, skip in (("S", False, False), ("W", True, True)):
        bd = bundles[name]
        st = mas.DeepFilterNetStreamer(bd.model, None, 2, MAX_HOPS)
        z = np.zeros(0, np.float32)
        st.feed_hops([bd.row[: bd.hop], z])
        assert st.launches == st.expected_launches(False, fb, skip) == 3 + int(fb)
        st.feed_hops([bd.row[bd.hop: 4 * bd.hop], bd.row[: bd.hop]])
        assert st.launches == st.expected_launches(True, fb, skip) == bd.model.expected_launches(fb, skip) + 1
        st.feed_hops([z, z])
        assert st.launches == 0 and st.hops_seen == [4, 1]
        st.close()


# ---------------------------------------------------------------------------------------------- 7. errors
def test_create_and_feed_errors(bundles):
    import ctypes as C
    from mlx_audio_swift_amd import _lib
    bd = bundles["S"]
    m, lib = bd.model, _lib.lib()

    def create(model, streams, max_hops):
        h = C.c_void_p()
        rc = lib.mis_deepfilternet_stream_create(model._h, streams, max_hops, C.byref(h))
        return rc, _lib.last_error(), h

    for args, word in (((m, 0, 4), "streams"), ((m, 9, 4), "streams"), ((m, 1, 0), "max_hops"), ((m, 1, 257), "max_hops"),
                       ((mas.DeepFilterNet(bd.cfg), 1, 4), "not finalized")):
        rc, msg, _ = create(*args)
        assert rc != 0 and word in msg, (args[1:], msg)
    assert lib.mis_deepfilternet_stream_create(m._h, 1, 4, None) != 0 and "null" in _lib.last_error()
    for kw, word in ((dict(fft_size=192, hop_size=48), "fft_size"), (dict(df_lookahead=3, conv_lookahead=2), "df_lookahead")):
        cfg, W = R.case("S", **kw)
        rc, msg, _ = create(mas.DeepFilterNet.from_weights(cfg, W), 1, 4)
        assert rc != 0 and word in msg, msg
    rc, _, h = create(m, 2, 4)
    assert rc == 0
    hop = bd.hop
    pcm, out = np.zeros((2, 4 * hop), np.float32), np.zeros((2, 4 * hop), np.float32)
    lens, ls, lc = np.zeros(2, np.int64), np.zeros((2, 4), np.float32), np.zeros(2, np.int32)

    def feed(hops, pcm_p=pcm.ctypes.data, stride=4 * hop, out_p=out.ctypes.data, room=4 * hop, rows=4):
        hp = np.asarray(hops, np.int32)
        rc = lib.mis_deepfilternet_stream_feed(h, pcm_p, hp.ctypes.data, stride, out_p, room, lens.ctypes.data, ls.ctypes.data, rows, lc.ctypes.data)
        return rc, _lib.last_error()

    for kw, word in ((dict(hops=[5, 0]), "max_hops"), (dict(hops=[-1, 0]), "max_hops"), (dict(hops=[1, 1], pcm_p=None), "null"),
                     (dict(hops=[1, 1], out_p=None), "null"), (dict(hops=[4, 0], stride=3 * hop), "pcm"), (dict(hops=[4, 4]), None),
                     (dict(hops=[4, 4], room=3 * hop), "out"), (dict(hops=[4, 4], rows=3), "lsnr")):
        rc, msg = feed(**kw)
        assert (rc == 0) == (word is None) and (word is None or word in msg), (kw, msg)
    assert int(lib.mis_deepfilternet_stream_hops_seen(h, 0)) == 4 and int(lib.mis_deepfilternet_stream_hops_seen(h, 2)) == -1
    assert lib.mis_deepfilternet_stream_reset(h, 2) != 0 and "stream" in _lib.last_error()
    lib.mis_deepfilternet_stream_destroy(h)
    assert same(bd.stream(bd.row, 3 * hop, 0)[0], bd.offline(bd.row, 0)[0][: bd.offline(bd.row, 0)[3]])   # the model is still usable


# ---------------------------------------------------------------------------------------------- 8. the module functions
def test_enhance_streaming_and_chunks(bundles):
    bd = bundles["S"]
    wav, _, H, count = bd.offline(bd.row, 3)
    y = mas.deepfilternet_enhance_streaming(bd.model, bd.row, chunk_samples=5)          # floored at one hop
    assert same(y, wav[:count])
    parts = list(mas.deepfilternet_stream_chunks(bd.model, bd.row, 4 * bd.hop))
    assert [p[1] for p in parts] == list(range(len(parts))) and [p[2] for p in parts] == [False] * (len(parts) - 1) + [True]
    assert same(np.concatenate([p[0] for p in parts]), wav[:count])
    assert mas.deepfilternet_enhance_streaming(bd.model, np.zeros(0, np.float32)).size == 0


# ---------------------------------------------------------------------------------------------- 9. float64 parity
def relrms(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30))


@pytest.mark.parametrize("name", ["S", "W"])
def test_float64_stream_reference(bundles, name):
    """The device's stream over [:count] against the float64 hop-by-hop reference, inside the offline chained test's gate."""
    bd = bundles[name]
    wav, _, H, count = bd.offline(bd.row, 3)
    y, _, _ = bd.stream(bd.row, bd.hop, 3)
    xe = np.concatenate([bd.row, np.zeros(3 * bd.hop, np.float32)])
    w64 = SR.stream_all(SR.DeepFilterNetStreamRef(bd.cfg, bd.W), xe)[bd.delay:][:count]
    w32 = R.DeepFilterNetRef(bd.cfg, bd.W, np.float32).forward(xe)[25][:count]
    d_ref, d_dev = relrms(w32, w64), relrms(y, w64)
    gate = 4.0 * d_ref + FLOOR
    print(f"deepfilternet stream {name}: device {d_dev:.3e} f32-reference {d_ref:.3e} gate {gate:.3e}")
    path = os.environ.get("MIS_DEEPFILTERNET_STREAM_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(config=name, kind="stream", stage=25, device=d_dev, f32_reference=d_ref, gate=gate)) + "\n")
    assert d_dev <= gate, (d_dev, gate)
