"""CPU tier of the Moonshine family: the torch reference of the GPU tests (tests/moonshine_ref.py) is held to an independent
implementation (transformers' MoonshineForConditionalGeneration, same weights loaded key for key), and the host-side pieces of
mlx_audio_swift_amd.moonshine (config, tokenizer, sanitize, frame arithmetic, loader checks) are checked without a GPU."""
import json
import os

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
import moonshine_ref as mr

TINY = dict(vocab_size=512, hidden_size=288, intermediate_size=320, encoder_num_hidden_layers=2, decoder_num_hidden_layers=2)   # hd 36
BASE = dict(vocab_size=512, hidden_size=416, intermediate_size=448, encoder_num_hidden_layers=2, decoder_num_hidden_layers=2)   # hd 52


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("shape", [TINY, BASE, dict(TINY, attention_bias=True, tie_word_embeddings=False)],
                         ids=["hd36", "hd52", "hd36_bias_untied"])
def test_reference_matches_transformers(shape):
    """Encoder output and teacher-forced logits of the f32 reference against transformers 5.x with the same weights.  Measured here:
    encoder 6.0e-7 / logits 4.6e-7 of the largest value (hd 36), the same order for hd 52 - float32 round-off of two summation orders.
    Gate: 1e-5, about 20x that and three orders below any modelling difference (a wrong RoPE pairing or gate half gives > 1e-1)."""
    transformers = pytest.importorskip("transformers")
    cfg = mas.MoonshineConfig(**shape)
    hc = transformers.MoonshineConfig(**{k: v for k, v in shape.items()}, encoder_num_attention_heads=8, decoder_num_attention_heads=8)
    hf = transformers.MoonshineForConditionalGeneration(hc).eval()
    W = mr.make_weights(cfg, seed=3)
    load = dict(W)
    load.setdefault("proj_out.weight", W["model.decoder.embed_tokens.weight"])
    res = hf.load_state_dict(load, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    audio = torch.randn(1, 16000, generator=torch.Generator().manual_seed(1)) * 0.2
    toks = torch.randint(0, cfg.vocab_size, (1, 7), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        out = hf(input_values=audio, decoder_input_ids=toks)
    ref = mr.MoonshineRef(cfg, W, round=None)
    enc = ref.encode(audio[0])
    assert enc.shape == (40, cfg.hidden_size) == tuple(out.encoder_last_hidden_state.shape[1:])
    e_enc, e_lg = _rel(enc, out.encoder_last_hidden_state[0]), _rel(ref.decode_all(toks[0], enc), out.logits[0])
    print("moonshine ref vs transformers", e_enc, e_lg)
    assert e_enc < 1e-5 and e_lg < 1e-5


def test_full_recompute_and_cached_decoding_choose_the_same_tokens():
    cfg = mas.MoonshineConfig(**dict(TINY, eos_token_id=511))
    W = mr.make_weights(cfg, seed=5)
    audio = torch.randn(4000, generator=torch.Generator().manual_seed(4)) * 0.2
    for mode in (None, "bf16"):
        ref = mr.MoonshineRef(cfg, W, round=mode)
        full, n_full = ref.generate(audio, max_tokens=12, cached=False)
        cached, n_cached = ref.generate(audio, max_tokens=12, cached=True)
        assert full == cached and n_full == n_cached == len(full) + 1 and len(full) == 12


def test_frame_count_formula_against_the_reference_shapes():
    cfg = mas.MoonshineConfig(**TINY)
    ref = mr.MoonshineRef(cfg, mr.make_weights(cfg, seed=1), round=None)
    lens = [895, 896, 1000, 1278, 1279, 1663, 4000, 16000, 16001, 33333]
    for n in lens:
        t3 = ref.stem(torch.zeros(n))[3].shape[0]
        assert t3 == mas.moonshine_frames(n) == mr.frames(n) >= 1, n
    assert mas.moonshine_frames(894) == 0 and mas.moonshine_frames(895) == 1 and mas.moonshine_frames(0) == 0
    assert mas.moonshine_frames(16000) == 40 and mas.moonshine_frames(480000) == 1248
    with pytest.raises(RuntimeError):
        ref.stem(torch.zeros(894))                       # the reference has no frame to give either
    # the library's own arithmetic (no GPU needed: the handle may be NULL)
    l = np.asarray(lens + [894, 126, 0], np.int64)
    out = np.zeros(len(l), np.int32)
    assert mas._lib.lib().mis_moonshine_frames(None, l.ctypes.data, len(l), out.ctypes.data) == 0
    assert out.tolist() == [mas.moonshine_frames(int(n)) for n in l]


@pytest.mark.parametrize("shape", [TINY, BASE], ids=["hd36", "hd52"])
def test_head_padding_to_64_is_a_no_op(shape):
    cfg = mas.MoonshineConfig(**shape)
    W = mr.make_weights(cfg, seed=7)
    Wp = mr.pad_heads(cfg, W, 64)
    assert Wp["model.encoder.layers.0.self_attn.q_proj.weight"].shape == (8 * 64, cfg.hidden_size)
    audio = torch.randn(3000, generator=torch.Generator().manual_seed(8)) * 0.2
    toks = torch.tensor([1, 5, 9, 200])
    a, b = mr.MoonshineRef(cfg, W, round=None), mr.MoonshineRef(cfg, Wp, round=None)
    ea, eb = a.encode(audio), b.encode(audio)
    assert _rel(eb, ea) < 1e-6                            # (only the summation order over the zero columns may differ)
    assert _rel(b.decode_all(toks, eb), a.decode_all(toks, ea)) < 1e-6


def test_rotary_dims():
    for hd, rot in ((36, 32), (52, 46), (64, 56)):
        assert mas.moonshine_rotary_dim(hd, 0.9) == mr.rotary_dim(hd, 0.9) == rot
    assert mas.moonshine_rotary_dim(2, 0.9) == 2 and mas.moonshine_rotary_dim(36, 1.0) == 36 and mas.moonshine_rotary_dim(36, 0.01) == 2


def _tokenizer_dir(tmp_path):
    vocab = {"<s>": 0, "</s>": 1, "▁hello": 2, "▁wor": 3, "ld": 4, "<0xC3>": 5, "<0xA9>": 6, "<0xE2>": 7, "<0x82>": 8, "<0xAC>": 9, "▁": 10,
             "<0xFF>": 11, "<0xZZ>": 12}
    tj = {"model": {"type": "BPE", "vocab": vocab}, "added_tokens": [{"id": 0, "content": "<s>", "special": True},
                                                                     {"id": 1, "content": "</s>", "special": True},
                                                                     {"id": 4, "content": "ld", "special": False}]}
    (tmp_path / "tokenizer.json").write_text(json.dumps(tj), encoding="utf-8")
    return str(tmp_path)


def test_tokenizer_decode(tmp_path):
    tk = mas.MoonshineTokenizer(_tokenizer_dir(tmp_path))
    assert tk.decode([0, 2, 3, 4, 1]) == "hello world"                       # specials skipped, U+2581 -> space, trimmed
    assert tk.decode([2, 5, 6]) == "helloé"                                   # two byte tokens fold into one character
    assert tk.decode([5, 6, 10, 7, 8, 9, 10]) == "é €"                        # three-byte character; trailing space trimmed
    assert tk.decode([2, 11, 3]) == "hello wor"                               # an invalid UTF-8 run is dropped
    assert tk.decode([5, 2, 6]) == "hello"                                    # a run broken by a piece: both halves invalid
    assert tk.decode([12, 999]) == "<0xZZ>"                                   # not hex: an ordinary piece; unknown id skipped
    assert tk.decode([]) == ""
    (tmp_path / "tokenizer.json").write_text(json.dumps({"model": {"vocab": {}}}))
    with pytest.raises(mas.AudioGenerationError):
        mas.MoonshineTokenizer(str(tmp_path))


def test_decode_without_a_tokenizer_uses_ascii_or_id():
    m = mas.MoonshineModel.__new__(mas.MoonshineModel)
    m.tokenizer, m._h = None, None
    assert m.decode([72, 105, 300, 33]) == "Hi<300>!"


def test_sanitize_tied_and_untied():
    keys = {"model.encoder.conv1.weight": 1, "model.decoder.norm.weight": 2, "proj_out.weight": 3, "other.key": 4}
    tied = mas.moonshine_sanitize(keys, True)
    assert tied == {"encoder.conv1.weight": 1, "decoder.norm.weight": 2, "other.key": 4}
    untied = mas.moonshine_sanitize(keys, False)
    assert untied == {"encoder.conv1.weight": 1, "decoder.norm.weight": 2, "proj_out.weight": 3, "other.key": 4}
    conv = np.zeros((4, 2, 7), np.float32)
    assert mas.moonshine_sanitize({"model.encoder.conv2.weight": conv})["encoder.conv2.weight"].shape == (4, 2, 7)   # published layout kept


def test_config_defaults_and_from_dict():
    c = mas.MoonshineConfig()
    assert (c.model_type, c.vocab_size, c.hidden_size, c.intermediate_size) == ("moonshine", 32768, 288, 1152)
    assert (c.encoder_num_hidden_layers, c.decoder_num_hidden_layers, c.encoder_num_attention_heads, c.decoder_num_attention_heads) == (6, 6, 8, 8)
    assert (c.encoder_num_key_value_heads, c.decoder_num_key_value_heads) == (8, 8)
    assert (c.encoder_hidden_act, c.decoder_hidden_act, c.max_position_embeddings, c.attention_bias, c.attention_dropout) == ("gelu", "silu", 512, False, 0.0)
    assert (c.partial_rotary_factor, c.rope_theta, c.bos_token_id, c.eos_token_id, c.decoder_start_token_id) == (0.9, 10000.0, 1, 2, 1)
    assert c.tie_word_embeddings is True and c.pad_head_dim_to_multiple_of is None
    b = mas.MoonshineConfig.from_dict({"hidden_size": 416, "intermediate_size": 1664, "encoder_num_hidden_layers": 8, "decoder_num_hidden_layers": 8,
                                       "encoder_num_attention_heads": 8, "decoder_num_attention_heads": 4, "encoder_num_key_value_heads": None,
                                       "unknown": 1, "tie_word_embeddings": False})
    assert (b.hidden_size, b.encoder_num_key_value_heads, b.decoder_num_key_value_heads, b.tie_word_embeddings) == (416, 8, 4, False)
    cc = b.to_c()
    assert (cc.hidden_size, cc.decoder_num_key_value_heads, cc.encoder_hidden_act, cc.decoder_hidden_act, cc.tie_word_embeddings) == (416, 4, 0, 1, 0)
    assert abs(cc.partial_rotary_factor - 0.9) < 1e-7 and cc.rope_theta == 10000.0
    p = mas.MoonshineModel.default_generation_parameters.fget(None)
    assert (p.max_tokens, p.temperature) == (200, 0.0)


def test_quantised_directory_is_rejected_before_any_device_work(tmp_path):
    from safetensors.torch import save_file
    cfg = mas.MoonshineConfig(**TINY)
    (tmp_path / "config.json").write_text(json.dumps(TINY))
    W = {k: v.contiguous() for k, v in mr.make_weights(cfg, seed=1).items()}
    k = "model.decoder.layers.0.mlp.fc2.weight"
    W[k[: -len("weight")] + "scales"] = torch.ones(288, 5)
    W[k[: -len("weight")] + "biases"] = torch.zeros(288, 5)
    save_file(W, os.path.join(tmp_path, "model.safetensors"))
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.MoonshineModel.from_model_directory(str(tmp_path))
    assert e.value.case == "invalidInput" and "quantised" in str(e.value) and ".scales" in str(e.value) or ".biases" in str(e.value)
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.MoonshineModel.from_pretrained(os.path.join(tmp_path, "no-such-directory"))
    assert e.value.case == "invalidInput"
