"""Sortformer without a GPU: the reference of tests/sortformer_ref.py against independent implementations (transformers'
ParakeetEncoder, torch's TransformerEncoderLayer, a scipy STFT path), its distance-indexed band form against the literal rel-shift, the host side of
mlx-audio-swift_amd/sortformer.py (configs, sanitize, segments, RTTM, silence trimming, the compression port against a line-by-line
transliteration), the decision seeds of tests/test_gpu_sortformer.py, and the kernels' resource use from the compile remarks."""
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
import sortformer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.parametrize("T", [1, 2, 31, 33, 65])
def test_band_form_equals_the_literal_rel_shift(T):
    cfg = R.case_config("A")
    ref = R.Ref(cfg, R.synthetic_weights(cfg, 3), torch.float64)
    g = torch.Generator().manual_seed(T)
    x = torch.randn(T, 128, generator=g, dtype=torch.float64)
    a = ref.fc_attn("fc_encoder.layers.0.self_attn.", x, band=False)
    b = ref.fc_attn("fc_encoder.layers.0.self_attn.", x, band=True)
    assert torch.equal(a, b)
    # the table the device builds by distance: row d + Tcap - 1 holds the angle d x div_term, whatever Tcap is
    pe = ref.pos_emb(T)
    for d in (-(T - 1), 0, T - 1):
        ang = d * torch.exp(torch.arange(0, 128, 2, dtype=torch.float64) * (-math.log(10000.0) / 128))
        assert torch.allclose(pe[(T - 1) - d, 0::2], torch.sin(ang)) and torch.allclose(pe[(T - 1) - d, 1::2], torch.cos(ang))


def test_bart_layer_equals_torch_transformer_encoder_layer():
    cfg = R.case_config("B")
    t = cfg.tf_encoder_config
    W = R.synthetic_weights(cfg, 4)
    ref = R.Ref(cfg, W, torch.float64)
    layer = torch.nn.TransformerEncoderLayer(t.d_model, t.encoder_attention_heads, t.encoder_ffn_dim, dropout=0.0, activation="relu",
                                             layer_norm_eps=t.layer_norm_eps, batch_first=True, norm_first=False).double().eval()
    q = "tf_encoder.layers.1."
    g = lambda n: ref.W[q + n]
    with torch.no_grad():
        layer.self_attn.in_proj_weight.copy_(torch.cat([g("self_attn.q_proj.weight"), g("self_attn.k_proj.weight"), g("self_attn.v_proj.weight")]))
        layer.self_attn.in_proj_bias.copy_(torch.cat([g("self_attn.q_proj.bias"), g("self_attn.k_proj.bias"), g("self_attn.v_proj.bias")]))
        layer.self_attn.out_proj.weight.copy_(g("self_attn.out_proj.weight")); layer.self_attn.out_proj.bias.copy_(g("self_attn.out_proj.bias"))
        layer.linear1.weight.copy_(g("fc1.weight")); layer.linear1.bias.copy_(g("fc1.bias"))
        layer.linear2.weight.copy_(g("fc2.weight")); layer.linear2.bias.copy_(g("fc2.bias"))
        layer.norm1.weight.copy_(g("self_attn_layer_norm.weight")); layer.norm1.bias.copy_(g("self_attn_layer_norm.bias"))
        layer.norm2.weight.copy_(g("final_layer_norm.weight")); layer.norm2.bias.copy_(g("final_layer_norm.bias"))
        x = torch.randn(37, t.d_model, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
        want = layer(x[None])[0]
    assert torch.allclose(ref.tf_layer(1, x), want, rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("peak,norm,pad", [(True, True, 16), (False, False, 0), (True, True, 0)])
def test_front_end_equals_a_scipy_stft_path(peak, norm, pad):
    from scipy.signal import stft
    from scipy.signal.windows import hann
    wave = R.test_wave(1, 16000 + 77)
    got = R.features(wave, 80, torch.float64, peak, norm, pad).numpy()
    x = wave.astype(np.float64)
    if peak:
        x = x / (np.abs(x).max() + 1e-3)
    x = np.concatenate([x[:1], x[1:] - 0.97 * x[:-1]])
    win = np.zeros(512)
    win[56:456] = hann(400, sym=True)
    _, _, Z = stft(x, window=win, nperseg=512, noverlap=512 - 160, nfft=512, boundary="zeros", padded=False, return_onesided=True)
    F = 1 + len(x) // 160
    power = np.abs(Z.T[:F] * win.sum()) ** 2
    mel = np.log(power @ R.mel_filters(80) + 2.0 ** -24)
    if norm:
        mel = (mel - mel.mean(0)) / (mel.std(0, ddof=1) + 1e-5)
    if pad:
        mel = np.concatenate([mel, np.zeros((-F % pad, 80))])
    assert got.shape == mel.shape and np.abs(got - mel).max() < 1e-7 * max(1.0, np.abs(mel).max())


def test_config_defaults_and_decoding():
    c = mas.SortformerConfig.from_dict({})
    e, t, m, p = c.fc_encoder_config, c.tf_encoder_config, c.modules_config, c.processor_config
    assert (e.hidden_size, e.num_hidden_layers, e.num_attention_heads, e.intermediate_size, e.num_mel_bins, e.conv_kernel_size,
            e.subsampling_conv_channels, e.attention_bias, e.scale_input) == (512, 18, 8, 2048, 80, 9, 256, True, True)
    assert (t.d_model, t.encoder_layers, t.encoder_attention_heads, t.encoder_ffn_dim, t.max_source_positions, t.k_proj_bias) == (192, 18, 8, 768, 1500, False)
    assert (m.num_speakers, m.chunk_len, m.fifo_len, m.spkcache_len, m.spkcache_sil_frames_per_spk, m.max_index, m.use_aosc) == (4, 188, 0, 188, 5, 10000, False)
    assert (p.feature_size, p.sampling_rate, p.hop_length, p.n_fft, p.win_length, p.preemphasis) == (80, 16000, 160, 512, 400, 0.97)
    c = mas.SortformerConfig.from_dict({"model_type": "sortformer", "num_speakers": 4, "fc_encoder_config": {"hidden_size": 256, "num_hidden_layers": 4},
                                        "tf_encoder_config": {"d_model": 96}, "modules_config": {"use_aosc": True, "fifo_len": 188},
                                        "processor_config": {"hop_length": 160}})
    assert (c.fc_encoder_config.hidden_size, c.fc_encoder_config.num_hidden_layers, c.tf_encoder_config.d_model) == (256, 4, 96)
    assert c.modules_config.use_aosc and c.modules_config.fifo_len == 188 and c.fc_encoder_config.intermediate_size == 2048
    flat = mas.SortformerConfig.from_dict({"hidden_size": 128, "d_model": 48, "spkcache_len": 94})        # the flat-config fallback
    assert (flat.fc_encoder_config.hidden_size, flat.tf_encoder_config.d_model, flat.modules_config.spkcache_len) == (128, 48, 94)
    assert len(mas.sortformer_expected_keys(mas.SortformerConfig())) == 993


def test_sanitize():
    w = {"fc_encoder.subsampling.layers.0.weight": np.zeros((256, 1, 3, 3), np.float32),
         "fc_encoder.subsampling.layers.0.bias": np.zeros(256, np.float32),
         "fc_encoder.subsampling.linear.weight": np.zeros((512, 2560), np.float32),
         "fc_encoder.layers.0.conv.pointwise_conv1.weight": np.zeros((1024, 512, 1), np.float32),
         "fc_encoder.layers.0.conv.depthwise_conv.weight": np.zeros((512, 1, 9), np.float32),
         "fc_encoder.layers.0.conv.norm.num_batches_tracked": np.zeros(1, np.float32)}
    s = mas.sortformer_sanitize(w)
    assert s["fc_encoder.subsampling.layers_0.weight"].shape == (256, 3, 3, 1) and "fc_encoder.subsampling.layers_0.bias" in s
    assert s["fc_encoder.subsampling.linear.weight"].shape == (512, 2560)
    assert s["fc_encoder.layers.0.conv.pointwise_conv1.weight"].shape == (1024, 1, 512)
    assert s["fc_encoder.layers.0.conv.depthwise_conv.weight"].shape == (512, 9, 1)
    assert not any("num_batches_tracked" in k for k in s)
    done = {"fc_encoder.subsampling.layers_0.weight": np.zeros((256, 3, 3, 1), np.float32),
            "fc_encoder.layers.0.conv.depthwise_conv.weight": np.zeros((512, 9, 1), np.float32)}
    again = mas.sortformer_sanitize(done)
    assert {k: v.shape for k, v in again.items()} == {k: v.shape for k, v in done.items()}


def _preds(n, spk, spans):
    p = np.zeros((n, spk), np.float32)
    for s, a, b, v in spans:
        p[a:b, s] = v
    return p


def test_preds_to_segments_cases():
    f = mas.preds_to_segments
    segs = f(_preds(20, 2, [(0, 0, 10, 0.8), (1, 5, 15, 0.9)]), 0.08)
    assert len(segs) >= 2 and {s.speaker for s in segs} == {0, 1} and all(s.end > s.start for s in segs)
    assert f(np.zeros((20, 4), np.float32), 0.08) == []
    short = _preds(20, 2, [(0, 5, 7, 0.9)])
    assert f(short, 0.08, min_duration=0.5) == [] and len(f(short, 0.08, min_duration=0.0)) == 1
    gap = _preds(30, 1, [(0, 0, 5, 0.9), (0, 7, 15, 0.9)])
    assert len(f(gap, 0.08, merge_gap=0.0)) == 2 and len(f(gap, 0.08, merge_gap=0.5)) == 1
    order = f(_preds(20, 3, [(2, 0, 5, 0.9), (0, 8, 13, 0.9), (1, 15, 20, 0.9)]), 0.08)
    assert [s.speaker for s in order] == [2, 0, 1]
    ex = f(_preds(12, 1, [(0, 3, 8, 0.9), (0, 10, 12, 0.9)]), 0.08)
    assert len(ex) == 2 and abs(ex[0].start - 0.24) < 1e-5 and abs(ex[0].end - 0.64) < 1e-5 and abs(ex[1].start - 0.80) < 1e-5 and abs(ex[1].end - 0.96) < 1e-5


def test_rttm_text_and_state():
    out = mas.DiarizationOutput([mas.DiarizationSegment(0.0, 1.0, 0), mas.DiarizationSegment(1.5, 2.5, 1)], num_speakers=2)
    assert out.text.split("\n") == ["SPEAKER audio 1 0.000 1.000 <NA> <NA> speaker_0 <NA> <NA>", "SPEAKER audio 1 1.500 1.000 <NA> <NA> speaker_1 <NA> <NA>"]
    empty = mas.DiarizationOutput([])
    assert empty.text == "" and empty.num_speakers == 0
    z = lambda *s: np.zeros(s, np.float32)
    st = mas.StreamingState(z(1, 0, 512), z(1, 0, 4), z(1, 0, 512), z(1, 0, 4), 0, z(1, 512), z(1))
    assert (st.spkcache_len, st.fifo_len, st.frames_processed) == (0, 0, 0)


def test_trim_silence_hand_cases():
    sr, fl = 16000, 480
    loud = np.ones(40 * fl, np.float32)
    w, off = mas.trim_silence(loud, sr)
    assert off == 0 and len(w) == len(loud)                                  # nothing to trim
    w, off = mas.trim_silence(np.ones(10 * fl, np.float32), sr)              # shorter than 2 x 16 frames: untouched
    assert off == 0 and len(w) == 10 * fl
    x = np.concatenate([np.zeros(20 * fl), np.ones(30 * fl), np.zeros(10 * fl + 100)]).astype(np.float32)
    w, off = mas.trim_silence(x, sr)
    assert off == 20 * fl and len(w) == 30 * fl
    x[25 * fl: 26 * fl] = 0.0                                                # a hole: the first run of 16 speech frames starts behind it
    w, off = mas.trim_silence(x, sr)
    assert off == 26 * fl and len(w) == 24 * fl


@pytest.mark.parametrize("seed", range(6))
def test_compression_port_equals_the_transliteration(seed):
    from mlx_audio_swift_amd import sortformer as S
    rng = np.random.default_rng(seed)
    m = mas.ModulesConfig(spkcache_len=16, spkcache_sil_frames_per_spk=1, use_aosc=True)
    n = 16 + int(rng.integers(1, 9))
    preds = rng.uniform(0, 1, (1, n, 4)).astype(np.float32)
    preds[0, :, 3] = rng.uniform(0, 0.4, n)                                 # a speaker that never speaks: all of its scores disabled
    if seed % 2:
        preds[0, ::3] = preds[0, 1]                                         # ties: equal rows
        preds[0, :, 2] = 0.9
    embs = rng.standard_normal((1, n, 8)).astype(np.float32)
    mean_sil = rng.standard_normal((1, 8)).astype(np.float32)
    e1, p1 = S.compress_spkcache_aosc(embs, preds, mean_sil, m)
    e2, p2 = R.literal_compress_aosc(embs, preds, mean_sil, m)
    assert e1.shape == (1, 16, 8) and np.array_equal(e1, e2) and np.array_equal(p1, p2)
    # the state update around it
    st = mas.StreamingState(embs[:, :16], preds[:, :16], np.concatenate([embs, embs], 1)[:, :20], np.concatenate([preds, preds], 1)[:, :20], 7, mean_sil,
                            np.ones(1, np.float32))
    out = mas.maybe_compress_state(st, 16, 16, m)
    assert (out.spkcache_len, out.fifo_len, out.frames_processed) == (16, 16, 7)
    simple = mas.maybe_compress_state(st, 16, 16, mas.ModulesConfig(use_aosc=False))
    assert (simple.spkcache_len, simple.fifo_len) == (16, 16)
    assert mas.maybe_compress_state(simple, 16, 16, m) is simple


def test_decision_seeds_satisfy_the_cap():
    """On the references alone: at most 2 % of the entries of every row are exempt at every threshold, and in every row at least two
    speakers are active on some frames and inactive on others (the synthetic head's gain R.HEAD_GAIN was raised until this held)."""
    cfg = R.case_config("A")
    W = R.synthetic_weights(cfg, 5, R.HEAD_GAIN)
    r32, r64 = R.Ref(cfg, W, torch.float32), R.Ref(cfg, W, torch.float64)
    for seed in R.DECISION_SEEDS:
        row = R.decision_row(seed)
        p64, p32 = (r.forward_features(R.features(row, 32, r.dtype)).numpy() for r in (r64, r32))
        for thr in R.DECISION_THRESHOLDS:
            assert R.exempt_mask(p64, p32, thr).mean() <= 0.02, (seed, thr)
        on = p64 > 0.5
        assert sum(bool(on[:, s].any() and not on[:, s].all()) for s in range(4)) >= 2, seed


# ---------------------------------------------------------------------------------------------- transformers' ParakeetEncoder
def _parakeet(cfg, W):
    """transformers' ParakeetEncoder (an implementation of the same FastConformer that is neither this project's nor the reference's)
    in float64 with the weights of W: torch layouts, i.e. the inverse of the sanitize transposes."""
    from transformers.models.parakeet.configuration_parakeet import ParakeetEncoderConfig
    from transformers.models.parakeet.modeling_parakeet import ParakeetEncoder
    e = cfg.fc_encoder_config
    pc = ParakeetEncoderConfig(hidden_size=e.hidden_size, num_hidden_layers=e.num_hidden_layers, num_attention_heads=e.num_attention_heads,
                               num_key_value_heads=e.num_key_value_heads, intermediate_size=e.intermediate_size, hidden_act="silu",
                               attention_bias=e.attention_bias, convolution_bias=True, conv_kernel_size=e.conv_kernel_size,
                               subsampling_factor=8, subsampling_conv_channels=e.subsampling_conv_channels, num_mel_bins=e.num_mel_bins,
                               subsampling_conv_kernel_size=3, subsampling_conv_stride=2, dropout=0.0, dropout_positions=0.0, layerdrop=0.0,
                               activation_dropout=0.0, attention_dropout=0.0, scale_input=e.scale_input)
    pc._attn_implementation = "eager"
    enc = ParakeetEncoder(pc).double().eval()
    sd = {}
    for k, v in W.items():
        if not k.startswith("fc_encoder."):
            continue
        k, t = k[len("fc_encoder."):], torch.as_tensor(np.asarray(v, np.float32)).double()
        if k.startswith("subsampling.layers_"):
            k = k.replace("layers_", "layers.")
            t = t.permute(0, 3, 1, 2) if t.ndim == 4 else t
        elif t.ndim == 3:
            t = t.permute(0, 2, 1)
        sd[k] = t.contiguous()
    missing, unexpected = enc.load_state_dict(sd, strict=False)
    assert not unexpected and all("num_batches_tracked" in k or "inv_freq" in k for k in missing), (missing, unexpected)
    return enc


@pytest.mark.parametrize("name", ["A", "P2"])
def test_conformer_stack_equals_transformers_parakeet_encoder(name):
    """The subsampling alone, one block alone, and one full-length row through the whole stack, float64.  The subsampling must agree to
    float64 rounding.  ParakeetEncoder's attention takes its softmax in float32 whatever the model's dtype, and the encoder forms its
    position table in float32 (relative error 2^-24 in every weight, sine and cosine), so a block and the full row are held to 1e-5 of
    the output's largest value: two orders above what those roundings can reach through a block's O(1) gains, four below what a wrong
    ordering, sign, scale or shift gives (the bound is set from the formats, not from what the comparison shows)."""
    if name == "A":
        cfg = R.case_config("A")
    else:                                                                 # head size 64, more heads, no input scale, 5 taps.  (attention_bias
        cfg = R.case_config("A")                                          # stays on: without it ParakeetEncoder also drops the feed-forward
        e = cfg.fc_encoder_config                                         # biases, which the reference's ConformerFeedForward always has.)
        e.hidden_size, e.num_attention_heads, e.num_key_value_heads, e.scale_input, e.conv_kernel_size = 256, 4, 4, False, 5
        cfg.modules_config.fc_d_model = 256
    W = R.synthetic_weights(cfg, 9)
    ref, enc = R.Ref(cfg, W, torch.float64), _parakeet(cfg, W)
    mels, d = cfg.fc_encoder_config.num_mel_bins, cfg.fc_encoder_config.hidden_size
    feats = R.features(R.test_wave(2, 16000 * 3 + 211), mels, torch.float64, pad_to=0)          # 301 frames: odd lengths at every stage
    with torch.no_grad():
        sub = enc.subsampling(feats[None])[0]
        mine = ref.pre_encode(feats)
        assert mine.shape == sub.shape == (R.diar_frames(feats.shape[0]), d)
        assert torch.allclose(mine, sub, rtol=1e-11, atol=1e-11 * float(sub.abs().max()))
        x = torch.randn(41, d, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
        blk = enc.layers[1](x[None], attention_mask=None, position_embeddings=ref.pos_emb(41)[None])[0]
        assert float((ref.fc_layer(1, x) - blk).abs().max()) <= 1e-5 * float(blk.abs().max())
        full = enc(feats[None]).last_hidden_state[0]
        got = ref.stages_from_embeddings(mine)[cfg.fc_encoder_config.num_hidden_layers - 1]
        assert got.shape == full.shape and float((got - full).abs().max()) <= 1e-5 * float(full.abs().max())


@pytest.mark.parametrize("aosc", [False, True])
def test_streaming_chain_of_the_reference_and_the_host_port(aosc):
    """The reference's own generateStream chain (float64 model, transliterated state code): at every step the lengths are the ones
    maybeCompressState's definition gives, frames_processed counts every diarization frame once, and the host's numpy
    maybe_compress_state returns the transliteration's VALUES from the same state, in both compression modes."""
    mod = dict(spkcache_len=16, spkcache_sil_frames_per_spk=1, use_aosc=aosc, chunk_left_context=1, chunk_right_context=1, spkcache_update_period=16)
    cfg = R.case_config("A", **mod)
    m = cfg.modules_config
    ref = R.Ref(cfg, R.synthetic_weights(cfg, 5, R.HEAD_GAIN), torch.float64)
    wave = R.test_wave(70, 96000)
    feats, _ = R.stream_features(ref, wave)
    steps = list(R.generate_stream(ref, wave, 0.64, 16, 16))
    assert len(steps) >= 9 and steps[-1][6].frames_processed == sum(R.diar_frames(b - a) for _, (a, b), *_ in steps) == R.diar_frames(feats.shape[0])
    fired = 0
    for idx, (a, b), right, before, preds, new, after in steps:
        n = R.diar_frames(b - a)
        assert preds.shape == (n, 4) and new.fifo.shape[1] == before.fifo.shape[1] + n and new.fifo_preds.shape[1] == new.fifo.shape[1]
        assert new.spkcache_preds.shape[1] == new.spkcache.shape[1] == before.spkcache.shape[1]
        assert (right is not None) == (aosc and idx + 1 < len(steps))
        assert (after.spkcache.shape[1], after.fifo.shape[1]) == R.expected_lengths(new.spkcache.shape[1], new.fifo.shape[1], 16, 16, m)
        host = mas.maybe_compress_state(mas.StreamingState(new.spkcache, new.spkcache_preds, new.fifo, new.fifo_preds, new.frames_processed,
                                                           new.mean_sil_emb, new.n_sil_frames), 16, 16, m)
        for x, y in ((host.spkcache, after.spkcache), (host.spkcache_preds, after.spkcache_preds), (host.fifo, after.fifo),
                     (host.fifo_preds, after.fifo_preds), (host.mean_sil_emb, after.mean_sil_emb), (host.n_sil_frames, after.n_sil_frames)):
            assert np.array_equal(np.asarray(x, np.float32), np.asarray(y, np.float32)), idx
        fired += after.spkcache.shape[1] < new.spkcache.shape[1] + (new.fifo.shape[1] - after.fifo.shape[1])
    assert fired >= 3                                                    # the cache was compressed several times


@pytest.mark.parametrize("seed", range(4))
def test_simple_compression_equals_the_transliteration(seed):
    from mlx_audio_swift_amd import sortformer as S
    rng = np.random.default_rng(100 + seed)
    n = 20 + seed
    preds = rng.uniform(0, 1, (1, n, 4)).astype(np.float32)
    if seed % 2:
        preds[0, 5:9] = preds[0, 2]                                       # ties
        preds[0, 11] = 0.0                                                # below the clip
    embs = rng.standard_normal((1, n, 8)).astype(np.float32)
    e1, p1 = S.compress_spkcache_simple(embs, preds, 16)
    e2, p2 = R.literal_compress_simple(embs, preds, 16)
    assert e1.shape == (1, 16, 8) and np.array_equal(e1, e2) and np.array_equal(p1, p2)


# ---------------------------------------------------------------------------------------------- ISA
@pytest.fixture(scope="module")
def usage():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S",
                            os.path.join(ROOT, "mlx-audio-swift_amd", "csrc", "sortformer.hip"), "-o", os.path.join(td, "k.s"),
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
        for key, pat in (("vgprs", r"remark:\s+VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m:
                cur[key] = int(m.group(1))
    return use


def test_kernel_resources(usage):
    """No kernel of sortformer.hip uses scratch, the log-mel front end it shares with lasr.hip (k_nemo_*, csrc/audio_front.h) included.  Every instance of the attention kernel stays within 128 VGPRs, and its LDS within the
    figure the file's header derives for head size 64 with the band: (64 x 65 + 2 x 32 x 65 + 2 x 64 + 96 x 65) floats = 58752 bytes."""
    mine = {k: v for k, v in usage.items() if "k_sf_" in k or "k_nemo_" in k}
    assert sum("k_nemo_" in k for k in mine) == 2, mine
    assert len(mine) >= 15 and all(v["scratch"] == 0 for v in mine.values()), mine
    attn = {k: v for k, v in mine.items() if "k_sf_attn" in k}
    assert len(attn) == 4 and all(v["vgprs"] <= 128 for v in attn.values()), attn
    assert max(v["lds"] for v in attn.values()) == 4 * (64 * 65 + 2 * 32 * 65 + 2 * 64 + 96 * 65) == 58752
