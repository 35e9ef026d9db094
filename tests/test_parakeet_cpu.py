"""Parakeet without a GPU: the specification of tests/parakeet_ref.py against independent implementations (transformers' ParakeetEncoder at
head size 128, torch.nn.LSTM, a transliteration of the reference's decode loop), the host side of mlx-audio-swift_amd/parakeet.py, and
the margin of the decision seeds that tests/test_gpu_parakeet.py relies on."""
import copy

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
import parakeet_ref as P
import sortformer_ref as R

NEMO_CONFIG = {
    "target": "nemo.collections.asr.models.rnnt_bpe_models.EncDecRNNTBPEModel", "model_defaults": {"tdt_durations": [0, 1, 2, 3, 4]},
    "preprocessor": {"sample_rate": 16000, "normalize": "per_feature", "window_size": 0.025, "window_stride": 0.01, "window": "hann", "features": 128,
                     "n_fft": 512, "dither": 1e-5},
    "encoder": {"feat_in": 128, "n_layers": 24, "d_model": 1024, "n_heads": 8, "ff_expansion_factor": 4, "subsampling_factor": 8,
                "self_attention_model": "rel_pos", "subsampling": "dw_striding", "conv_kernel_size": 9, "subsampling_conv_channels": 256,
                "pos_emb_max_len": 5000},
    "decoder": {"blank_as_pad": True, "vocab_size": 1024, "prednet": {"pred_hidden": 640, "pred_rnn_layers": 2}},
    "joint": {"num_classes": 1024, "vocabulary": ["<unk>", "▁a"], "num_extra_outputs": 5,
              "jointnet": {"joint_hidden": 640, "activation": "relu", "encoder_hidden": 1024, "pred_hidden": 640}},
    "decoding": {"model_type": "tdt", "durations": [0, 1, 2, 3, 4], "greedy": {"max_symbols": 10}}}


def test_encoder_equals_transformers_parakeet_encoder_at_head_128():
    """One block and one row through the stack, float64, hidden 256 = 2 x 128; the bound and its reasoning are those of
    test_sortformer_cpu.test_conformer_stack_equals_transformers_parakeet_encoder."""
    from test_sortformer_cpu import _parakeet
    cfg = P.case_config(256)
    scfg = P.sf_config(cfg)
    W = R.synthetic_weights(scfg, 9)
    ref, enc = R.Ref(scfg, W, torch.float64), _parakeet(scfg, W)
    feats = R.features(R.test_wave(2, 16000 + 211), cfg.num_mel_bins, torch.float64, peak_normalize=False, pad_to=0)
    with torch.no_grad():
        x = torch.randn(41, 256, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
        blk = enc.layers[1](x[None], attention_mask=None, position_embeddings=ref.pos_emb(41)[None])[0]
        assert float((ref.fc_layer(1, x) - blk).abs().max()) <= 1e-5 * float(blk.abs().max())
        full = enc(feats[None]).last_hidden_state[0]
        got = ref.intake(ref.pre_encode(feats))
        for i in range(cfg.num_hidden_layers):
            got = ref.fc_layer(i, got)
        assert got.shape == full.shape and float((got - full).abs().max()) <= 1e-5 * float(full.abs().max())


def test_lstm_equals_torch_lstm():
    Pw = 32
    W = {k: v.astype(np.float64) for k, v in P.make_decoder(3, Pw, 32, 40).items()}
    lstm = torch.nn.LSTM(Pw, Pw, num_layers=2, batch_first=True).double()
    lstm.load_state_dict({k.split("lstm.")[1]: torch.as_tensor(v) for k, v in W.items() if "lstm." in k})
    rng = np.random.default_rng(0)
    h, c, tok = rng.standard_normal((2, Pw)), rng.standard_normal((2, Pw)), 5
    _, hn, cn = P.predict(W, tok, 40, h, c)
    with torch.no_grad():
        _, (th, tc) = lstm(torch.as_tensor(W["decoder.prediction.embed.weight"][tok])[None, None], (torch.as_tensor(h)[:, None], torch.as_tensor(c)[:, None]))
    assert np.allclose(hn, th[:, 0].numpy(), rtol=0, atol=1e-13) and np.allclose(cn, tc[:, 0].numpy(), rtol=0, atol=1e-13)


def _case_weights(W, bias):
    Wc = dict(W)
    if bias is not None:
        Wc["joint.joint_net.bias"] = bias
    return Wc


@pytest.mark.parametrize("index", range(9))
def test_tdt_loop_equals_the_transliteration(index):
    c = P.TDT
    W, rows = P.tdt_cases()
    name, e, T, bias = rows[index]
    Wc = _case_weights(W, bias)
    lit = P.literal_tdt(Wc, e[:T], c["vocab"], P.DURATIONS, c["max_symbols"])
    got = P.tdt_decode(Wc, e[:T], c["vocab"], P.DURATIONS, c["max_symbols"], cap=10 ** 6)
    assert list(zip(got["tokens"], got["frames"], got["durations"])) == lit
    capped = P.tdt_decode(Wc, e[:T], c["vocab"], P.DURATIONS, c["max_symbols"], c["cap"])
    assert capped["tokens"] == [t for t, _, _ in lit][:c["cap"]] and capped["flag"] == int(len(lit) > c["cap"])
    n = len(lit)
    expect = dict(one_frame=n >= 0, duration_0_always=n == 3 * T and all(d == 0 for _, _, d in lit), blank_duration_0=n == 0 and got["steps"] == 3 * T,
                  jump_past_end=got["steps"] == 1, all_blank=n == 0, capacity=capped["flag"] == 1 and n == T)
    assert expect.get(name, True), (name, n, got["steps"])


def test_decision_margin():
    """The smallest top-2 gap of either arg-max over every step of every case is at least 100 x the specification's own float32-vs-float64
    logit distance (the float32 run follows the float64 decisions), so the device's float32 sums cannot turn a decision."""
    c = P.TDT
    W, rows = P.tdt_cases()
    for name, e, T, bias in rows:
        Wc = _case_weights(W, bias)
        r64 = P.tdt_decode(Wc, e[:T], c["vocab"], P.DURATIONS, c["max_symbols"], c["cap"])
        r32 = P.tdt_decode(Wc, e[:T], c["vocab"], P.DURATIONS, c["max_symbols"], c["cap"], np.float32, follow=r64["decisions"])
        dist = max(float(np.abs(a - b).max()) for a, b in zip(r64["logits"], r32["logits"]))
        assert r64["gap"] >= 100.0 * dist, (name, r64["gap"], dist)


def test_config_sanitize_and_loader_errors(tmp_path):
    c = mas.ParakeetConfig.from_dict(NEMO_CONFIG, max_batch=2)
    assert (c.hidden_size, c.num_attention_heads, c.intermediate_size, c.num_mel_bins, c.pred_hidden, c.joint_hidden, c.vocab_size, c.durations,
            c.max_symbols, c.hop_length, c.win_length, c.max_batch) == (1024, 8, 4096, 128, 640, 640, 1024, [0, 1, 2, 3, 4], 10, 160, 400, 2)
    for change, word in ((dict(target="nemo.collections.asr.models.ctc_bpe_models.EncDecCTCModelBPE"), "CTC"),
                         (dict(target="nemo.collections.asr.models.hybrid_rnnt_ctc_bpe_models.EncDecHybridRNNTCTCBPEModel"), "TDT-CTC"),
                         (dict(model_defaults={}), "RNNT"), (dict(quantization={"group_size": 64, "bits": 4}), "quantised"), (dict(target="x"), "Unsupported")):
        bad = copy.deepcopy(NEMO_CONFIG)
        bad.update(change)
        with pytest.raises(mas.AudioGenerationError, match=word):
            mas.ParakeetConfig.from_dict(bad)
    z = lambda *s: np.zeros(s, np.float32)
    w = mas.parakeet_sanitize({
        "encoder.pre_encode.conv.0.weight": z(16, 1, 3, 3), "encoder.pre_encode.conv.3.weight": z(16, 16, 1, 1), "encoder.pre_encode.out.bias": z(8),
        "encoder.pre_encode.depthwise_layers.1.weight": z(16, 3, 3, 1), "encoder.layers.0.self_attn.linear_pos.weight": z(8, 8),
        "encoder.layers.0.self_attn.pos_bias_u": z(2, 4), "encoder.layers.0.conv.batch_norm.running_mean": z(8),
        "encoder.layers.0.conv.batch_norm.num_batches_tracked": z(1), "encoder.layers.0.conv.depthwise_conv.weight": z(8, 1, 9),
        "encoder.layers.0.conv.pointwise_conv1.weight": z(16, 8, 1), "joint.joint_net.2.weight": z(46, 8), "preprocessor.featurizer.window": z(400),
        "decoder.prediction.dec_rnn.lstm.1.Wx": z(32, 8), "decoder.prediction.dec_rnn.lstm.1.bias": z(32)})
    shapes = {k: tuple(v.shape) for k, v in w.items()}
    assert shapes == {
        "encoder.subsampling.layers_0.weight": (16, 3, 3, 1), "encoder.subsampling.layers_3.weight": (16, 1, 1, 16), "encoder.subsampling.linear.bias": (8,),
        "encoder.subsampling.layers_5.weight": (16, 3, 3, 1), "encoder.layers.0.self_attn.relative_k_proj.weight": (8, 8),
        "encoder.layers.0.self_attn.bias_u": (2, 4), "encoder.layers.0.conv.norm.running_mean": (8,), "encoder.layers.0.conv.depthwise_conv.weight": (8, 9, 1),
        "encoder.layers.0.conv.pointwise_conv1.weight": (16, 1, 8), "joint.joint_net.weight": (46, 8),
        "decoder.prediction.dec_rnn.lstm.weight_ih_l1": (32, 8), "decoder.prediction.dec_rnn.lstm.bias_ih_l1": (32,),
        "decoder.prediction.dec_rnn.lstm.bias_hh_l1": (32,)}
    with pytest.raises(mas.AudioGenerationError, match="quantised"):
        mas.parakeet_sanitize({"joint.enc.scales": z(2, 2)})
    assert set(P.make_weights(P.case_config(144), 1)) == mas.parakeet_expected_keys(P.case_config(144))
    with pytest.raises(mas.AudioGenerationError, match="not a local model directory"):
        mas.ParakeetModel.from_pretrained(str(tmp_path / "absent"))
