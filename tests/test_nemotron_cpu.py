"""CPU: what holds tests/nemotron_ref.py (the specification test_gpu_nemotron.py compares the device with) and the host side of
mlx-audio-swift_amd/nemotron.py: the mask against a hand-written table, the band / short-table form against the literal one, the decode loop's
cells against torch.nn.LSTM, the decision margin of the GPU tests' seeds, config defaults, sanitize, loader errors and refusals."""
import copy
import json

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
import nemotron_ref as N

# context -> rows of a 7 x 7 table, '1' where query (row) sees key (column); written by hand from 0 <= q / C - k / C <= L
MASKS = {(56, 13): ["1111111"] * 7,                                                                     # C 14: one chunk
         (4, 1): ["1100000", "1100000", "1111000", "1111000", "1111110", "1111110", "0011111"],        # C 2, L 2
         (0, 0): ["1000000", "0100000", "0010000", "0001000", "0000100", "0000010", "0000001"],        # C 1, L 0
         (-1, 3): ["1111000", "1111000", "1111000", "1111000", "1111111", "1111111", "1111111"]}       # C 4, unlimited


@pytest.mark.parametrize("ctx", list(MASKS))
def test_mask_against_a_hand_written_table(ctx):
    want = np.array([[ch == "1" for ch in row] for row in MASKS[ctx]])
    assert np.array_equal(N.mask(7, *ctx) == 0, want)
    big = N.mask(100, 56, 13) == 0                                         # C 14, L 4: query 70 (chunk 5) sees the keys 14 .. 83
    assert big[70].nonzero()[0].tolist() == list(range(14, 84)) and big[99].nonzero()[0].tolist() == list(range(42, 100))


@pytest.mark.parametrize("ctx", [(56, 13), (4, 1), (0, 0), (-1, 3), (70, 0)])
def test_band_form_equals_the_literal_form(ctx):
    H, hd, n, Tcap = 2, 8, 45, 50
    rng = np.random.default_rng(3)
    qkv, table = rng.standard_normal((n, 3 * H * hd)).astype(np.float32), rng.standard_normal((2 * Tcap - 1, H * hd)).astype(np.float32)
    u, v = (rng.uniform(-0.5, 0.5, (H, hd)).astype(np.float32) for _ in range(2))
    C, L = N.context(*ctx)
    short = np.full_like(table, np.nan)                                    # the band form may read the rows -(C - 1) .. L C + C - 1 alone
    short[Tcap - 1 - (C - 1): Tcap + min(L * C + C - 1, Tcap - 1)] = table[Tcap - 1 - (C - 1): Tcap + min(L * C + C - 1, Tcap - 1)]
    lit = N.attention(qkv, table, u, v, n, H, hd, Tcap, ctx, torch.float64)
    band = N.attention(qkv, short, u, v, n, H, hd, Tcap, ctx, torch.float64, band=True)
    assert np.isfinite(band).all() and np.abs(lit - band).max() < 1e-12


@pytest.mark.parametrize("layers", [1, 2])
def test_predict_equals_torch_lstm(layers):
    c = N.RNNT
    W = {k: v.astype(np.float64) for k, v in N.make_decoder(3, c["P"], c["J"], c["vocab"], layers).items()}
    lstm = torch.nn.LSTM(c["P"], c["P"], num_layers=layers).double()
    with torch.no_grad():
        for name, p in lstm.named_parameters():
            p.copy_(torch.as_tensor(W["decoder.prediction.dec_rnn.lstm." + name]))
    h, cc = np.zeros((layers, c["P"])), np.zeros((layers, c["P"]))
    state = None
    for tok in (c["vocab"], 3, 17):                                        # the blank feeds zeros
        pp, h, cc = N.predict(W, tok, c["vocab"], h, cc)
        x = torch.zeros(1, 1, c["P"], dtype=torch.float64) if tok == c["vocab"] else torch.as_tensor(W["decoder.prediction.embed.weight"][tok])[None, None]
        y, state = lstm(x, state)
        assert np.abs(h - state[0][:, 0].detach().numpy()).max() < 1e-12 and np.abs(cc - state[1][:, 0].detach().numpy()).max() < 1e-12
        assert np.abs(pp - (W["joint.pred.weight"] @ y[0, 0].detach().numpy() + W["joint.pred.bias"])).max() < 1e-12


@pytest.mark.parametrize("layers", [1, 2])
def test_decode_loop_edge_cases_and_decision_margin(layers):
    """rnntStep's rules on the edge cases; and the smallest top-2 gap over every step of every case is at least 100 x the specification's own
    float32-vs-float64 logit distance (the float32 run follows the float64 decisions), so the device's float32 sums cannot turn a decision."""
    c = N.RNNT
    W, rows = N.rnnt_cases(layers)
    for name, e, T, bias, ms in rows:
        Wc = dict(W, **({"joint.joint_net.bias": bias} if bias is not None else {}))
        r64 = N.rnnt_decode(Wc, e[:T], c["vocab"], ms, c["cap"])
        r32 = N.rnnt_decode(Wc, e[:T], c["vocab"], ms, c["cap"], np.float32, follow=r64["decisions"])
        dist = max(float(np.abs(a - b).max()) for a, b in zip(r64["logits"], r32["logits"]))
        assert r64["gap"] >= 100.0 * dist, (name, r64["gap"], dist)
        if name == "all_blank":
            assert (r64["tokens"], r64["steps"], r64["flag"]) == ([], T, 0)
        if name == "always_emit":                                          # max_symbols emissions a frame, the last of them advances
            assert r64["frames"] == [t for t in range(T) for _ in range(ms)] and r64["steps"] == T * ms
        if name == "no_max_symbols_capacity":
            assert (len(r64["tokens"]), set(r64["frames"]), r64["flag"], r64["steps"]) == (c["cap"], {0}, 1, c["cap"] + 1)


def test_end_to_end_decision_margin():
    """the seeds of test_gpu_nemotron's end-to-end models: float32 specification tokens equal the float64 ones, with the margin above"""
    import sortformer_ref as R
    for hidden in (256, 144):
        cfg = N.case_config(hidden, bias=hidden == 256)
        W = N.make_weights(cfg, 21)
        r = N.Encoder(cfg, W, torch.float64)
        x = r.intake(r.pre_encode(r.features(R.test_wave(41, 16037))))
        for i in range(cfg.num_hidden_layers):
            x = r.fc_layer(i, x)
        encp = r.joint_enc(r.prompt(x, 0)).numpy()
        r64 = N.rnnt_decode(W, encp, cfg.vocab_size, cfg.max_symbols, cfg.max_tokens)
        r32 = N.rnnt_decode(W, encp, cfg.vocab_size, cfg.max_symbols, cfg.max_tokens, np.float32, follow=r64["decisions"])
        dist = max(float(np.abs(a - b).max()) for a, b in zip(r64["logits"], r32["logits"]))
        assert r64["gap"] >= 100.0 * dist, (hidden, r64["gap"], dist)


CONFIG = {"model_type": "nemotron_asr", "decoder": {"vocab_size": 1024, "prednet": {"pred_hidden": 640, "pred_rnn_layers": 2}},
          "joint": {"num_classes": 1025, "jointnet": {"joint_hidden": 640, "activation": "relu", "encoder_hidden": 1024, "pred_hidden": 640}},
          "prompt": {"prompt_dictionary": {"en-US": 0, "auto": 7}}, "vocabulary": ["▁a", "<en-US>"]}


def test_config_defaults_sanitize_and_refusals(tmp_path):
    c = mas.NemotronConfig.from_dict(copy.deepcopy(CONFIG), max_batch=2)
    assert (c.hidden_size, c.num_attention_heads, c.intermediate_size, c.num_mel_bins, c.conv_pads, c.contexts, c.default_context, c.attention_bias,
            c.num_prompts, c.prompt_hidden, c.default_language, c.pred_rnn_layers, c.max_symbols, c.normalize, c.hop_length, c.win_length, c.max_batch) == (
        1024, 8, 4096, 128, (8, 0), [(56, 13)], (56, 13), False, 128, 2048, "auto", 2, None, "NA", 160, 400, 2)
    plain = mas.NemotronConfig.from_dict({k: v for k, v in CONFIG.items() if k != "prompt"})
    assert (plain.prompt_hidden, plain.default_language) == (0, "en")
    enc = lambda **kw: dict(copy.deepcopy(CONFIG), encoder=kw)
    assert mas.NemotronConfig.from_dict(enc(conv_context_size=[5, 3])).conv_pads == (5, 3)
    assert mas.NemotronConfig.from_dict(enc(att_context_style="regular")).contexts == [(0, 1 << 30)]
    for bad, word in ((enc(conv_norm_type="batch_norm"), "conv_norm_type"), (enc(att_context_style="chunked_limited_with_rc"), "att_context_style"),
                      (enc(causal_downsampling=False), "non-causal"), (dict(CONFIG, quantization={"group_size": 64, "bits": 8}), "quantised"),
                      ({"joint": CONFIG["joint"]}, "decoder")):
        with pytest.raises(mas.AudioGenerationError, match=word):
            mas.NemotronConfig.from_dict(bad)
    z = np.zeros
    raw = {"encoder.pre_encode.conv.0.weight": z((4, 1, 3, 3)), "encoder.pre_encode.conv.2.weight": z((4, 1, 3, 3)), "encoder.pre_encode.conv.3.weight": z((4, 4, 1, 1)),
           "encoder.pre_encode.out.bias": z(8), "encoder.layers.0.self_attn.linear_pos.weight": z((8, 8)), "encoder.layers.0.self_attn.pos_bias_u": z((2, 4)),
           "encoder.layers.0.conv.batch_norm.weight": z(8), "encoder.layers.0.conv.depthwise_conv.weight": z((8, 1, 9)), "prompt_kernel.0.weight": z((6, 10)),
           "prompt_kernel.2.bias": z(8), "joint.joint_net.2.bias": z(5), "decoder.prediction.dec_rnn.lstm.0.Wx": z((16, 4)), "preprocessor.featurizer.window": z(4)}
    got = {k: v.shape for k, v in mas.nemotron_sanitize(raw).items()}
    assert got == {"encoder.subsampling.layers_0.weight": (4, 3, 3, 1), "encoder.subsampling.layers_2.weight": (4, 3, 3, 1),
                   "encoder.subsampling.layers_3.weight": (4, 1, 1, 4), "encoder.subsampling.linear.bias": (8,),
                   "encoder.layers.0.self_attn.relative_k_proj.weight": (8, 8), "encoder.layers.0.self_attn.bias_u": (2, 4),
                   "encoder.layers.0.conv.norm.weight": (8,), "encoder.layers.0.conv.depthwise_conv.weight": (8, 9, 1),
                   "prompt_kernel.linear0.weight": (6, 10), "prompt_kernel.linear2.bias": (8,), "joint.joint_net.bias": (5,),
                   "decoder.prediction.dec_rnn.lstm.weight_ih_l0": (16, 4)}
    with pytest.raises(mas.AudioGenerationError, match="quantised"):
        mas.nemotron_sanitize({"joint.enc.scales": z(4)})
    small = N.case_config(144)
    assert set(N.make_weights(small, 1)) == mas.nemotron_expected_keys(small)
    nobias = N.case_config(144, bias=False, prompt=False, rnn_layers=1)
    assert set(N.make_weights(nobias, 1)) == mas.nemotron_expected_keys(nobias)
    (tmp_path / "config.json").write_text(json.dumps(CONFIG).replace("1025", "Infinity"))
    with pytest.raises(mas.AudioGenerationError, match="SentencePiece|safetensors"):
        mas.NemotronASR.from_model_directory(str(tmp_path))
    with pytest.raises(mas.AudioGenerationError, match="not a local model directory"):
        mas.NemotronASR.from_pretrained("mlx-community/nemotron")
