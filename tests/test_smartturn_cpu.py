"""CPU tier of the Smart Turn family: the reference of the GPU tests (tests/smartturn_ref.py) is held to independent implementations
(transformers' WhisperEncoder with the same weights, WhisperFeatureExtractor on the same samples), and the host-side pieces of
mlx_audio_swift_amd.smartturn (config, sanitize, directory parsing) are checked without a GPU."""
import json
import os

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
import smartturn_ref as sr

FLOOR_FACTOR, SLACK = 2.0, 2e-3                      # the gate constants of test_gpu_smartturn.py


def _small_config(**enc):
    base = dict(max_source_positions=100, d_model=128, encoder_attention_heads=2, encoder_layers=2, encoder_ffn_dim=256)
    return mas.SmartTurnConfig(encoder_config=mas.SmartTurnEncoderConfig(**{**base, **enc}), max_audio_seconds=2)


@pytest.mark.parametrize("k_bias", [False, True], ids=["no_k_bias", "k_bias"])
def test_reference_encoder_matches_transformers(k_bias):
    """The f32 reference encoder against transformers' WhisperEncoder with identical weights: max_source_positions 100, 200 frames,
    d 128 / 2 heads / 2 layers.  Gate 1e-5 of the largest value, the one test_moonshine_cpu.py applies to its transformers comparison
    (float32 round-off of two summation orders sits near 1e-6; a modelling difference gives > 1e-1).  transformers' k_proj never has a
    bias; with k_proj_bias the reference's bias is loaded by hand."""
    transformers = pytest.importorskip("transformers")
    from transformers.models.whisper.modeling_whisper import WhisperEncoder
    cfg = _small_config(k_proj_bias=k_bias)
    e = cfg.encoder_config
    hc = transformers.WhisperConfig(num_mel_bins=80, d_model=e.d_model, encoder_layers=e.encoder_layers, encoder_attention_heads=e.encoder_attention_heads,
                                    encoder_ffn_dim=e.encoder_ffn_dim, max_source_positions=e.max_source_positions, activation_function="gelu")
    hf = WhisperEncoder(hc).eval()
    W = sr.make_weights(cfg, seed=3)
    load = {}
    for k, v in W.items():
        if not k.startswith("encoder.") or k.endswith("k_proj.bias"):
            continue
        load[k[len("encoder."):]] = v.permute(0, 2, 1).contiguous() if k in ("encoder.conv1.weight", "encoder.conv2.weight") else v
    res = hf.load_state_dict(load, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    if k_bias:
        for i, layer in enumerate(hf.layers):
            layer.self_attn.k_proj.bias = torch.nn.Parameter(W[f"encoder.layers.{i}.self_attn.k_proj.bias"].clone())
    feats = sr.input_features(sr.wave(30000, 1), cfg)                                        # [200, 80]
    with torch.no_grad():
        want = hf(torch.from_numpy(feats.T.copy())[None]).last_hidden_state[0]
    got = sr.SmartTurnRef(cfg, W, round=None).encode(feats)
    assert got.shape == (100, 128) == tuple(want.shape)
    err = float((got - want).abs().max() / want.abs().max())
    print("smartturn ref encoder vs transformers", err)
    assert err < 1e-5


def test_reference_features_match_the_whisper_feature_extractor():
    """An un-normalised row of exactly W samples against WhisperFeatureExtractor(feature_size=80, chunk_length=2), tolerance 6e-5 (what
    test_gpu_mel.py allows against HF features).  Differences found: (1) the window - Smart Turn's front end takes DSP.hanningWindow, the
    SYMMETRIC Hann (N - 1 in the denominator), OpenAI's front end the periodic one; with the reference's own window the two differ by up
    to ~1e-2 in the normalised log domain, so the comparison runs the reference chain with window="periodic" and the symmetric window is
    pinned separately below; (2) none in the frame count: both make 1 + W / hop frames and drop the last (200 at 2 s)."""
    transformers = pytest.importorskip("transformers")
    cfg = _small_config()
    pc = mas.SmartTurnProcessorConfig(max_audio_seconds=2, normalize_audio=False)
    a = sr.wave(cfg.window_samples, 5)
    fe = transformers.WhisperFeatureExtractor(feature_size=80, chunk_length=2)
    hf = fe(a, sampling_rate=16000, return_tensors="np")["input_features"][0].T              # [200, 80]
    ours = sr.features(sr.prepare(a, pc), pc, window="periodic")
    assert ours.shape == hf.shape == (200, 80)
    d = float(np.abs(ours - hf).max())
    sym = sr.features(sr.prepare(a, pc), pc)
    print("smartturn features vs HF", d, "symmetric-vs-periodic", float(np.abs(sym - ours).max()))
    assert d < 6e-5
    # the symmetric window itself: DSP.swift:15-22
    n = np.arange(400, dtype=np.float64)
    from oracle import mel as omel
    assert np.abs(omel.hanning_window(400) - 0.5 * (1 - np.cos(2 * np.pi * n / 399))).max() < 1e-6
    assert 1e-4 < float(np.abs(sym - ours).max())                                            # and it is a different front end


def test_prepare_keeps_the_tail_pads_in_front_and_normalises_the_whole_window():
    pc = mas.SmartTurnProcessorConfig(max_audio_seconds=2)
    Wn = 32000
    long = sr.wave(Wn + 12345, 1)
    raw = mas.SmartTurnProcessorConfig(max_audio_seconds=2, normalize_audio=False)
    assert np.array_equal(sr.prepare(long, raw), long[-Wn:])                                 # a long row keeps its tail
    short = sr.wave(1600, 3) + 0.25
    p = sr.prepare(short, raw)
    assert np.array_equal(p[-1600:], short) and not p[:-1600].any()                          # zeros in FRONT
    q = sr.prepare(short, pc)                                                                # statistics over all W samples, padding included
    x = np.concatenate([np.zeros(Wn - 1600), short.astype(np.float64)])
    want = (x - x.mean()) / x.std()
    assert np.abs(q - want).max() < 1e-4 and abs(float(q.mean())) < 1e-4 and abs(float(q.std()) - 1) < 1e-4
    assert np.all(q[:-1600] == q[0]) and q[0] != 0                                           # the padding moved with the mean
    assert np.abs(sr.prepare(short, pc, "f64") - want).max() < 1e-6
    z = sr.prepare(np.zeros(Wn // 2, np.float32), pc)
    assert not z.any()                                                                       # an all-zero row stays all zeros
    f = sr.input_features(np.zeros(Wn // 2, np.float32), _small_config())
    assert f.shape == (200, 80) and np.abs(f + 1.5).max() < 1e-6                             # (log10(1e-10) + 4) / 4


def test_config_defaults_compatibility_keys_and_missing_processor():
    c = mas.SmartTurnConfig()
    e, p = c.encoder_config, c.processor_config
    assert (c.model_type, c.architecture, c.dtype, c.sample_rate, c.max_audio_seconds, c.threshold) == ("smart_turn", "smart_turn", "float32", 16000, 8, 0.5)
    assert (e.model_type, e.num_mel_bins, e.max_source_positions, e.d_model, e.encoder_attention_heads, e.encoder_layers, e.encoder_ffn_dim,
            e.k_proj_bias) == ("smart_turn_encoder", 80, 400, 384, 6, 4, 1536, False)
    assert (p.sampling_rate, p.max_audio_seconds, p.n_fft, p.hop_length, p.n_mels, p.normalize_audio, p.threshold) == (16000, 8, 400, 160, 80, True, 0.5)
    assert (c.window_samples, c.frames, c.positions) == (128000, 800, 400)
    # the compatibility keys fill a missing processor_config, together with the encoder's mel bins
    d = mas.SmartTurnConfig.from_dict({"sample_rate": 8000, "max_audio_seconds": 4, "threshold": 0.7, "encoder_config": {"num_mel_bins": 64, "d_model": 256},
                                       "unknown": 1, "dtype": None})
    q = d.processor_config
    assert (q.sampling_rate, q.max_audio_seconds, q.n_mels, q.threshold, q.n_fft, q.hop_length, q.normalize_audio) == (8000, 4, 64, 0.7, 400, 160, True)
    assert (d.encoder_config.d_model, d.encoder_config.encoder_layers, d.dtype) == (256, 4, "float32")
    # a processor_config that is present wins over them
    g = mas.SmartTurnConfig.from_dict({"max_audio_seconds": 4, "threshold": 0.7, "processor_config": {"max_audio_seconds": 6, "normalize_audio": False}})
    assert (g.processor_config.max_audio_seconds, g.processor_config.threshold, g.processor_config.normalize_audio, g.max_audio_seconds) == (6, 0.5, False, 4)
    cc = mas.SmartTurnConfig.from_dict({"encoder_config": {"k_proj_bias": True}}).to_c()
    assert (cc.num_mel_bins, cc.max_source_positions, cc.d_model, cc.encoder_attention_heads, cc.encoder_layers, cc.encoder_ffn_dim, cc.k_proj_bias,
            cc.sampling_rate, cc.max_audio_seconds, cc.n_fft, cc.hop_length, cc.normalize_audio, cc.threshold) == (80, 400, 384, 6, 4, 1536, 1, 16000, 8, 400,
                                                                                                                    160, 1, 0.5)
    with pytest.raises(mas.AudioGenerationError):
        mas.SmartTurnConfig.from_dict({"processor_config": {"n_mels": 64}}).to_c()           # 64 mel bins into an 80-bin encoder


def test_engine_rejects_configurations_before_it_needs_a_device():
    """mis_smartturn_create judges the configuration first: the rejections hold on a machine without a GPU too."""
    import ctypes as C
    L = mas._lib.lib()
    for bad, word in ((dict(max_source_positions=399), "max_source_positions"), (dict(d_model=288), "head size"), (dict(d_model=400, encoder_attention_heads=5), "32"),
                      (dict(encoder_ffn_dim=1000), "encoder_ffn_dim")):
        cfg = mas.SmartTurnConfig(encoder_config=mas.SmartTurnEncoderConfig(**bad)).to_c()
        h = C.c_void_p()
        assert L.mis_smartturn_create(C.byref(cfg), 0, C.byref(h)) == 3 and word in mas._lib.last_error(), (bad, mas._lib.last_error())
    for bad, word in ((dict(hop_length=161), "even"), (dict(n_fft=4096), "n_fft")):           # 795 frames; n_fft above the front end's
        cfg = mas.SmartTurnConfig(processor_config=mas.SmartTurnProcessorConfig(**bad)).to_c()
        h = C.c_void_p()
        assert L.mis_smartturn_create(C.byref(cfg), 0, C.byref(h)) == 3 and word in mas._lib.last_error(), (bad, mas._lib.last_error())
    assert L.mis_smartturn_launches(None) == 0


def test_sanitize_every_branch():
    t = lambda *s: torch.arange(int(np.prod(s)), dtype=torch.float32).reshape(*s)
    raw = {"inner.encoder.conv1.weight": t(8, 5, 3), "inner.encoder.conv2.weight": t(8, 8, 3), "inner.encoder.conv1.bias": t(8),
           "inner.encoder.layers.0.fc1.weight": t(8, 32), "inner.encoder.layers.0.fc2.weight": t(32, 8),
           "encoder.layers.1.fc1.weight": t(32, 8), "encoder.layers.1.fc2.weight": t(8, 32),
           "inner.pool_attention.0.weight": t(8, 256), "inner.pool_attention.0.bias": t(256), "inner.pool_attention.2.weight": t(256, 1),
           "inner.pool_attention.2.bias": t(1), "inner.classifier.0.weight": t(256, 8), "inner.classifier.1.weight": t(256),
           "inner.classifier.4.bias": t(64), "inner.classifier.6.weight": t(1, 64), "val_loss": t(1), "val_acc.history": t(3)}
    s = mas.smart_turn_sanitize(raw)
    assert not [k for k in s if k.startswith("val_") or k.startswith("inner.") or "pool_attention." in k or "classifier." in k]
    assert s["encoder.conv1.weight"].shape == (8, 3, 5) and torch.equal(s["encoder.conv1.weight"], raw["inner.encoder.conv1.weight"].permute(0, 2, 1))
    assert s["encoder.conv2.weight"].shape == (8, 3, 8) and s["encoder.conv1.bias"].shape == (8,)
    assert s["encoder.layers.0.fc1.weight"].shape == (32, 8) and torch.equal(s["encoder.layers.0.fc1.weight"], raw["inner.encoder.layers.0.fc1.weight"].t())
    assert s["encoder.layers.0.fc2.weight"].shape == (8, 32)
    assert torch.equal(s["encoder.layers.1.fc1.weight"], raw["encoder.layers.1.fc1.weight"])      # already [ffn, d] / [d, ffn]: untouched
    assert torch.equal(s["encoder.layers.1.fc2.weight"], raw["encoder.layers.1.fc2.weight"])
    assert s["pool_attention_0.weight"].shape == (256, 8) and s["pool_attention_2.weight"].shape == (1, 256)
    assert set(s) >= {"pool_attention_0.bias", "pool_attention_2.bias", "classifier_0.weight", "classifier_1.weight", "classifier_4.bias", "classifier_6.weight"}
    assert len(s) == len(raw) - 2
    n = mas.smart_turn_sanitize({"encoder.conv1.weight": np.zeros((8, 5, 3), np.float32)})       # numpy arrays take the same path
    assert n["encoder.conv1.weight"].shape == (8, 3, 5)
    cfg = _small_config()
    W = sr.make_weights(cfg, seed=1)
    back = mas.smart_turn_sanitize(sr.raw_checkpoint(W))                                         # raw_checkpoint is sanitize's inverse
    assert set(back) == set(W) == mas.smart_turn_expected_keys(cfg) and all(torch.equal(back[k], W[k]) for k in W)
    assert "encoder.layers.0.self_attn.k_proj.bias" in mas.smart_turn_expected_keys(_small_config(k_proj_bias=True))


def test_model_directory_parsing_round_trip(tmp_path):
    from safetensors.torch import save_file
    cfg = _small_config()
    W = sr.make_weights(cfg, seed=2)
    (tmp_path / "config.json").write_text(json.dumps({"model_type": "smart_turn", "encoder_config": dict(cfg.encoder_config.__dict__), "max_audio_seconds": 2,
                                                      "threshold": 0.6}))
    raw = sr.raw_checkpoint(W)
    half = len(raw) // 2
    save_file(dict(list(raw.items())[:half]), os.path.join(tmp_path, "model-00001.safetensors"))
    save_file(dict(list(raw.items())[half:]), os.path.join(tmp_path, "model-00002.safetensors"))
    got_cfg, got = mas.smart_turn_read_directory(str(tmp_path))
    assert got_cfg.encoder_config == cfg.encoder_config and (got_cfg.processor_config.max_audio_seconds, got_cfg.processor_config.threshold) == (2, 0.6)
    assert set(got) == set(W) and all(torch.equal(got[k], W[k]) for k in W)
    save_file({"inner.encoder.extra.weight": torch.zeros(3)}, os.path.join(tmp_path, "model-00003.safetensors"))
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.smart_turn_read_directory(str(tmp_path))
    assert e.value.case == "invalidInput" and "encoder.extra.weight" in str(e.value)
    os.remove(os.path.join(tmp_path, "model-00003.safetensors"))
    save_file({"inner.encoder.layers.0.fc1.scales": torch.zeros(3)}, os.path.join(tmp_path, "q.safetensors"))
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.smart_turn_read_directory(str(tmp_path))
    assert e.value.case == "invalidInput" and "quantised" in str(e.value)
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.SmartTurnModel.from_pretrained(os.path.join(tmp_path, "no-such-directory"))
    assert e.value.case == "invalidInput"


def test_decision_margins_leave_most_rows_decidable():
    """The rows and weights of test_gpu_smartturn.py's decision test: m = FLOOR_FACTOR |logit_f64acc - logit_bf16| + SLACK per row; at
    most a quarter of the rows may lie within m of a threshold's logit.  Also the scale of the synthetic head: logits of rms order 1,
    both signs."""
    cfg = sr.case_config(sr.DECISION_SHAPE)
    W, rows = sr.make_weights(cfg, seed=sr.DECISION_SEED), sr.case_rows(cfg)
    r32, r64 = sr.SmartTurnRef(cfg, W, round="bf16"), sr.SmartTurnRef(cfg, W, round="bf16", acc=torch.float64)
    l32 = np.asarray([r32.forward(r)["logit"] for r in rows]); l64 = np.asarray([r64.forward(r)["logit"] for r in rows])
    m = FLOOR_FACTOR * np.abs(l64 - l32) + SLACK
    print("smartturn decision logits", l32.tolist(), "margins", m.tolist())
    assert len(rows) == 8
    for thr in (0.5, 0.25, 0.8):
        near = np.abs(l32 - sr.threshold_logit(thr)) <= m
        assert near.sum() <= len(rows) // 4, (thr, l32, m)
    rms_l = float(np.sqrt(np.mean(l32 ** 2)))
    assert 0.3 < rms_l < 3.0 and (l32 > 0).any() and (l32 < 0).any(), l32
