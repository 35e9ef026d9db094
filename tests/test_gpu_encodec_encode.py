"""-m gpu: EnCodec encode (csrc/encodec.hip: loudness normalisation, SEANet encoder, one-launch residual-VQ search) against the
float64 specification tests/encodec_encode_ref.py.

Gates are derived, never read from the device.  Stage taps: each stage of the specification runs on the DEVICE's previous stage;
d_ref is the relative rms between the specification's float32 twin and its float64 mode on that input, the gate 4 d_ref + 2^-23 (the
rule of tests/test_gpu_deepfilternet.py).  RVQ: exact on a dyadic grid; on Gaussian data the chosen entry's float64 distance is within
rvq_bound (derived in the specification file) of the minimum, and every residual update is bit for bit.  End to end: codes equal the
specification's up to the first near-tie of a frame (top-2 gap under rvq_bound), at most 10 % of the entries exempt.
With MIS_ENCODEC_ENCODE_PARITY_LOG=<file> the observed fractions are appended as JSON lines."""
import json
import os
from dataclasses import replace

import numpy as np
import pytest

import encodec_encode_ref as er
import mlx_audio_swift_amd as mas
from oracle import encodec as oe
from test_encodec_encode_cpu import exact_grid_case

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -23


def relrms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30)) if a.size else 0.0


def log_parity(**line):
    path = os.environ.get("MIS_ENCODEC_ENCODE_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")


def host_cfg(cfg, name, **extra):
    fields = {k: getattr(cfg, k) for k in mas.EncodecConfig.__dataclass_fields__ if hasattr(cfg, k)}
    fields["normalize"] = er.is_normalize(name)
    fields.update(extra)
    return mas.EncodecConfig(**fields)


class Bundle:
    def __init__(self, name):
        self.name, self.cfg = name, er.CONFIGS[name]
        self.W = er.make_synthetic_weights(self.cfg)
        self.dev = mas.Encodec.from_weights(host_cfg(self.cfg, name), self.W)
        self.r64 = er.EncodeRef(self.cfg, self.W, normalize=er.is_normalize(name))
        self.r32 = er.EncodeRef(self.cfg, self.W, dtype=np.float32, normalize=er.is_normalize(name))
        self.cases = [er.audio_rows(self.cfg, L, 1 + i % 3, seed=100 + i) for i, L in enumerate(er.row_lengths(self.cfg))]


@pytest.fixture(scope="module")
def bundles():
    return {n: Bundle(n) for n in er.CONFIGS}


NAMES = list(er.CONFIGS)


@pytest.mark.parametrize("name", NAMES)
def test_stage_taps_and_scales(bundles, name):
    b = bundles[name]
    stages = b.r64.stage_names()
    for x in b.cases:                                                       # [R, L, C]
        prev = np.swapaxes(x, 1, 2)
        for sid, st in enumerate(stages):
            got = b.dev.encode_tap(x, sid)
            w64, w32 = b.r64.stage(st, prev), b.r32.stage(st, prev)
            assert got.shape == w64.shape and np.isfinite(got).all(), (name, st, got.shape, w64.shape)
            d_ref, d_dev = relrms(w32, w64), relrms(got, w64)
            gate = 4.0 * d_ref + FLOOR
            log_parity(test="stage", config=name, rows=x.shape[0], L=x.shape[1], stage=st, d_ref=d_ref, d_dev=d_dev, gate=gate, frac=d_dev / gate)
            assert d_dev <= gate, (name, st, x.shape, d_dev, gate)
            prev = got
        if er.is_normalize(name):
            _, scales = b.dev.encode_rows(x)
            s64, s32 = b.r64.normalise(np.swapaxes(x, 1, 2))[1], b.r32.normalise(np.swapaxes(x, 1, 2))[1]
            d_ref, d_dev = relrms(s32, s64), relrms(scales, s64)
            log_parity(test="scale", config=name, rows=x.shape[0], L=x.shape[1], d_ref=d_ref, d_dev=d_dev, gate=4.0 * d_ref + FLOOR)
            assert scales.dtype == np.float32 and d_dev <= 4.0 * d_ref + FLOOR, (name, d_dev, d_ref)


@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_rvq_exact_tier(name):
    cfg = er.CONFIGS[name]
    nq = cfg.num_quantizers
    for frames, rows in ((1, 1), (31, 2), (32, 1), (33, 3), (65, 2)):
        Wg, emb = exact_grid_case(cfg, frames, rows, seed=frames)
        W = dict(er.make_synthetic_weights(cfg))
        W.update(Wg)
        dev = mas.Encodec.from_weights(host_cfg(cfg, name), W)
        ref = er.EncodeRef(cfg, W)
        for n in (1, nq):
            codes, res = dev.rvq_tap(emb, n)
            wc, wr, gaps, _ = ref.rvq(emb, n)
            assert np.array_equal(codes, wc), (name, frames, n, np.argwhere(codes != wc)[:4])
            assert res.shape == wr.shape == (n + 1, rows, cfg.codebook_dim, frames)
            assert np.array_equal(res.view(np.uint32), wr.astype(np.float32).view(np.uint32)), (name, frames, n)
        assert (gaps == 0).any()                                           # the planted ties were reached


@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_rvq_gaussian_tier(bundles, name):
    b = bundles[name]
    cfg, nq, D = b.cfg, b.cfg.num_quantizers, b.cfg.codebook_dim
    rng = np.random.default_rng(17)
    for frames, rows in ((33, 2), (65, 1), (7, 3)):
        emb = rng.standard_normal((rows, D, frames)).astype(np.float32)
        codes, res = b.dev.rvq_tap(emb, nq)
        assert codes.min() >= 0 and codes.max() < cfg.codebook_size
        assert np.array_equal(res[0].view(np.uint32), emb.view(np.uint32))
        worst = 0.0
        for q in range(nq):
            E32 = np.asarray(b.W[f"quantizer.layers.{q}.codebook.embed"], np.float32)
            E = E32.astype(np.float64)
            r = np.swapaxes(res[q], 1, 2).astype(np.float64)                 # the device's own residual [R, F, D]
            dist = ((r[:, :, None, :] - E[None, None]) ** 2).sum(-1)           # [R, F, CB]
            chosen = np.take_along_axis(dist, codes[:, q, :, None].astype(np.int64), -1)[..., 0]
            bound = er.rvq_bound(np.sqrt((r ** 2).sum(-1)), np.sqrt((E ** 2).sum(-1)).max(), D)
            excess = chosen - dist.min(-1)
            worst = max(worst, float((excess / bound).max()))
            assert (excess <= bound).all(), (name, q, float(excess.max()), float(bound.min()))
            nxt = (np.swapaxes(res[q], 1, 2) - E32[codes[:, q]]).astype(np.float32)
            assert np.array_equal(np.swapaxes(res[q + 1], 1, 2).view(np.uint32), nxt.view(np.uint32)), (name, q)
        log_parity(test="rvq_gaussian", config=name, rows=rows, frames=frames, worst_excess_over_bound=worst)


@pytest.mark.parametrize("name", NAMES)
def test_end_to_end_codes(bundles, name):
    b = bundles[name]
    nq = b.cfg.num_quantizers
    for x in b.cases:
        codes, _ = b.dev.encode_rows(x)
        emb = b.r64.encoder(np.swapaxes(x, 1, 2))
        want, _, gaps, bounds = b.r64.rvq(emb, nq)
        exempt = er.exempt_mask(gaps, bounds)
        assert codes.shape == want.shape == (x.shape[0], nq, er.num_frames(b.cfg, x.shape[1]))
        share = float(exempt.mean())
        differ = int(((codes != want) & ~exempt).sum())
        log_parity(test="end_to_end", config=name, rows=x.shape[0], L=x.shape[1], exempt_share=share, differing_non_exempt=differ,
                   differing_total=int((codes != want).sum()))
        assert share <= er.EXEMPT_CAP and differ == 0, (name, x.shape, share, differ)


def test_chunked_normalised_encode_and_round_trip():
    name = "tiny_48k"
    cfg = er.CONFIGS[name]
    W = er.make_synthetic_weights(cfg)
    dev = mas.Encodec.from_weights(host_cfg(cfg, name, chunk_length_s=0.1, overlap=0.25), W)      # 120-sample chunks, stride 90
    ref = er.EncodeRef(cfg, W, normalize=True, chunk_length=120, chunk_stride=90)
    raw = [er.audio_rows(cfg, n, 1, seed=n)[0] for n in (250, 140)]
    x, mask = mas.preprocess_encodec_audio(raw, cfg.sampling_rate, 120, 90)
    assert x.shape == (2, 300, 2)
    codes, scales = dev.encode(x, mask, bandwidth=1.5)
    wc, ws = ref.encode(x, mask, bandwidth=1.5)
    assert codes.shape == wc.shape == (3, 2, 3, er.num_frames(cfg, 120)) and len(scales) == 3
    for s, w in zip(scales, ws):
        assert s.shape == (2,) and np.allclose(s, w, rtol=2.0 ** -22, atol=0)
    orc = oe.EncodecOracle(cfg, W)
    frames = [orc.decode_frame(codes[i], scale=scales[i]) for i in range(3)]
    want = np.stack([oe.linear_overlap_add([f[:, ch] for f in frames], 90) for ch in range(2)], axis=1)
    got = dev.decode(codes, scales)
    assert got.shape == want.shape and np.abs(got - want).max() <= 3e-4 * np.abs(want).max()
    # a frame longer than the chunk is refused (Encodec.swift:220-222)
    with pytest.raises(mas.AudioGenerationError) as e:
        dev.encode_rows(x[:, :150])
    assert "longer than chunk" in str(e.value)


@pytest.mark.parametrize("name", ["tiny", "tiny_48k"])
def test_reconstruct_returns_the_input_length(bundles, name):
    b = bundles[name]
    x = er.audio_rows(b.cfg, 7 * b.cfg.hop_length - 3, 2, seed=9)
    y = b.dev.reconstruct(x)
    assert y.shape[0] == 2 and y.shape[-1] == x.shape[1] and np.isfinite(y).all()
    enc = b.dev.encode_audio(x)
    assert isinstance(enc, mas.EncodecEncodedAudio) and enc.codes.shape[:2] == (1, 2)
    assert np.array_equal(b.dev.decode_audio(enc)[..., : x.shape[1]], y)


@pytest.mark.parametrize("name", NAMES)
def test_row_independence_and_bandwidth_prefix(bundles, name):
    b = bundles[name]
    L = 7 * b.cfg.hop_length - 3
    x = er.audio_rows(b.cfg, L, 1, seed=21)
    alone_c, alone_s = b.dev.encode_rows(x)
    junk = (50.0 * np.random.default_rng(4).standard_normal((2, L, b.cfg.audio_channels))).astype(np.float32)
    for pos in range(3):
        batch = np.insert(junk, pos, x[0], axis=0)
        c, s = b.dev.encode_rows(batch)
        assert np.array_equal(c[pos], alone_c[0]), (name, pos)
        if er.is_normalize(name):
            assert s[pos].tobytes() == alone_s[0].tobytes()
    small, _ = b.dev.encode(x, bandwidth=b.cfg.target_bandwidths[0])
    large, _ = b.dev.encode(x, bandwidth=b.cfg.target_bandwidths[1])
    assert small.shape[2] == 1 and large.shape[2] == 3 and np.array_equal(small[0, :, 0], large[0, :, 0])
    assert np.array_equal(large[0], alone_c)


def test_loader_and_errors(tmp_path):
    from safetensors.numpy import save_file
    name = "tiny"
    cfg = er.CONFIGS[name]
    W = er.make_synthetic_weights(cfg)
    hc = host_cfg(cfg, name)
    x = er.audio_rows(cfg, 5 * cfg.hop_length, 1, seed=2)
    decoder_only = mas.Encodec.from_weights(hc, oe.make_synthetic_weights(cfg))
    assert not decoder_only.has_encoder
    with pytest.raises(mas.AudioGenerationError) as e:
        decoder_only.encode(x)
    assert "without encoder weights" in str(e.value)
    assert decoder_only.decode_frame(np.zeros((1, 3, 4), np.int32)).shape == (1, 4 * cfg.hop_length)
    dev = mas.Encodec.from_weights(hc, W)
    assert dev.has_encoder
    with pytest.raises(mas.AudioGenerationError):
        dev.encode(x, bandwidth=2.0)                                        # not in target_bandwidths
    with pytest.raises(mas.AudioGenerationError):
        dev.encode(x, bandwidth=3.0)                                        # listed, but asks for 6 of the 3 quantizers
    with pytest.raises(mas.AudioGenerationError):
        dev.encode(np.zeros((1, 40, 3), np.float32))                        # 3 channels
    d = tmp_path / "model"
    d.mkdir()
    meta = {k: (list(v) if isinstance(v, tuple) else v) for k, v in vars(hc).items()}
    (d / "config.json").write_text(json.dumps(dict(meta, model_type="encodec")))
    save_file({k: np.ascontiguousarray(v) for k, v in W.items()}, str(d / "model.safetensors"))
    loaded = mas.Encodec.from_pretrained(str(d))
    assert loaded.config == hc and np.array_equal(loaded.encode(x)[0], dev.encode(x)[0])
    save_file(dict({k: np.ascontiguousarray(v) for k, v in W.items()}, **{"encoder.layers.99.conv.bias": np.zeros(3, np.float32)}),
              str(d / "model.safetensors"))
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.Encodec.from_model_directory(str(d))
    assert "unused keys" in str(e.value)
    with pytest.raises(mas.AudioGenerationError):
        mas.Encodec.from_pretrained(str(tmp_path / "nowhere"))
    syn = mas.Encodec.synthetic(hc, seed=3)
    assert syn.has_encoder and syn.encode(x)[0].shape == (1, 1, 1, 5)
