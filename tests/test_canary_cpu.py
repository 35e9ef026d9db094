"""Canary on the CPU: tests/canary_ref.py held to torch's own modules, the cached step held to the reference's whole-prefix form, the host
side of mlx-audio-swift_amd/canary.py (config, checkpoint layouts, tokenizer), and the decision margin that lets test_gpu_canary.py compare
tokens for equality."""
import functools

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
import canary_ref as CR
import parakeet_ref as P
import sortformer_ref as R

CASES = ((256, 4), (144, 2))                  # h, decoder heads: head sizes 64 and 72
SECONDS = (0.3, 1.0, 2.5)


@functools.lru_cache(maxsize=None)
def _case(h, heads):
    cfg = CR.case_config(h, heads)
    W = CR.make_weights(cfg, 31)
    enc = P.Encoder(CR.encoder_view(cfg), W, torch.float64)
    waves = [R.test_wave(50 + i, int(16000 * s) + 37 * i) for i, s in enumerate(SECONDS)]
    outs = []
    for w in waves:
        x = enc.intake(enc.pre_encode(enc.features(w)))
        for l in range(cfg.encoder.n_layers):
            x = enc.fc_layer(l, x)
        outs.append(x)
    return cfg, W, outs


@pytest.mark.parametrize("h,heads", CASES)
def test_cached_step_equals_the_whole_prefix(h, heads):
    cfg, W, enc = _case(h, heads)
    d = CR.Decoder(W, heads, torch.float64)
    tokens = [0, 1, 2, 17, 5, 99, 3, 42]
    full, hid = d.prefix(tokens, d.project(enc[1]))
    cache = [None] * d.L
    for i, t in enumerate(tokens):
        lg, x = d.step(t, i, d.project(enc[1]), cache)
        assert torch.allclose(lg, full[i], rtol=0, atol=1e-11) and torch.allclose(x, hid[i], rtol=0, atol=1e-11)
    assert torch.equal(d.embed([5], 2000), d.embed([5], 1023))            # the last row repeats beyond the table


def test_block_equals_torch_modules():
    h, heads = 144, 2
    _, W, enc = _case(h, heads)
    d = CR.Decoder(W, heads, torch.float64)
    x, e = d.embed([0, 1, 2, 9]), d.project(enc[0])
    q = "decoder.blocks.0."
    out = x
    for at, kv in (("self_attn", None), ("cross_attn", e)):
        mha = torch.nn.MultiheadAttention(h, heads, bias=True, dtype=torch.float64)
        with torch.no_grad():
            mha.in_proj_weight.copy_(torch.cat([d.W[f"{q}{at}.{n}.weight"] for n in ("q_proj", "k_proj", "v_proj")]))
            mha.in_proj_bias.copy_(torch.cat([d.W[f"{q}{at}.{n}.bias"] for n in ("q_proj", "k_proj", "v_proj")]))
            mha.out_proj.weight.copy_(d.W[f"{q}{at}.out_proj.weight"]); mha.out_proj.bias.copy_(d.W[f"{q}{at}.out_proj.bias"])
        ln = torch.nn.LayerNorm(h, dtype=torch.float64)
        with torch.no_grad():
            ln.weight.copy_(d.W[f"{q}{at}_norm.weight"]); ln.bias.copy_(d.W[f"{q}{at}_norm.bias"])
        n = ln(out)
        mask = torch.triu(torch.ones(4, 4, dtype=torch.bool), 1) if kv is None else None
        out = out + mha(n, n if kv is None else kv, n if kv is None else kv, attn_mask=mask, need_weights=False)[0]
    ln = torch.nn.LayerNorm(h, dtype=torch.float64)
    with torch.no_grad():
        ln.weight.copy_(d.W[q + "ff_norm.weight"]); ln.bias.copy_(d.W[q + "ff_norm.bias"])
    out = out + d.lin(q + "ff2", torch.relu(d.lin(q + "ff1", ln(out))))
    mask = torch.triu(torch.full((4, 4), -1e9, dtype=torch.float64), 1)
    assert torch.allclose(out, d.block(0, x, e, mask), rtol=0, atol=1e-12)


def test_config_defaults_and_refusals():
    c = mas.CanaryConfig.from_dict({})
    e, dc = c.encoder, c.decoder
    assert (c.preprocessor.features, e.n_layers, e.d_model, e.n_heads, e.xscaling, e.use_bias) == (128, 32, 1024, 8, True, True)
    assert (dc.num_layers, dc.hidden_size, dc.num_attention_heads, dc.inner_size, c.vocab_size, c.enc_output_dim) == (8, 1024, 16, 4096, 16384, 1024)
    assert (c.startofcontext_id, c.startoftranscript_id, c.emo_undefined_id, c.endoftext_id) == (0, 1, 2, 3) and len(c.supported_languages) == 25
    t = c.to_c()
    assert (t.hop_length, t.win_length, t.scale_input, t.intermediate_size) == (160, 400, 1, 4096)
    nested = mas.CanaryConfig.from_dict({"transf_decoder": {"decoder": {"num_layers": 4}}, "decoder": {"num_layers": 6}, "tokenizer": {"model_base64": "QQ=="}})
    assert nested.decoder.num_layers == 4 and nested.tokenizer_model_base64 == "QQ=="
    with pytest.raises(mas.AudioGenerationError, match="quantised"):
        mas.CanaryConfig.from_dict({"quantization": {"bits": 4}})
    with pytest.raises(mas.AudioGenerationError, match="enc_output_dim"):
        mas.CanaryConfig.from_dict({"decoder": {"hidden_size": 512}}).to_c()
    with pytest.raises(mas.AudioGenerationError, match="rel_pos"):
        mas.CanaryConfig.from_dict({"encoder": {"self_attention_model": "abs_pos"}}).to_c()


def _layouts():
    z = lambda *s: np.zeros(s, np.float32)
    att = lambda pre, names: {f"{pre}{n}.{p}": z(4, 4) if p == "weight" else z(4) for n in names for p in ("weight", "bias")}
    enc = {"encoder.pre_encode.conv.0.weight": z(4, 1, 3, 3), "encoder.pre_encode.conv.2.weight": z(4, 1, 3, 3), "encoder.pre_encode.conv.3.weight": z(4, 4, 1, 1),
           "encoder.pre_encode.out.weight": z(4, 8), "encoder.layers.0.self_attn.linear_q.weight": z(4, 4), "encoder.layers.0.self_attn.pos_bias_u": z(2, 2),
           "encoder.layers.0.conv.batch_norm.weight": z(4), "encoder.layers.0.conv.depthwise_conv.weight": z(4, 1, 9)}
    nemo = dict(enc)
    nemo.update({"encoder.pre_encode.conv.1.weight": z(1), "encoder.pre_encode.conv.4.weight": z(1), "transf_decoder._embedding.token_embedding.weight": z(9, 4),
                 "transf_decoder._embedding.position_embedding.pos_enc": z(8, 4), "transf_decoder._embedding.layer_norm.weight": z(4),
                 "transf_decoder._decoder.final_layer_norm.weight": z(4), "transf_decoder._decoder.layers.0.layer_norm_1.weight": z(4),
                 "transf_decoder._decoder.layers.0.layer_norm_2.weight": z(4), "transf_decoder._decoder.layers.0.layer_norm_3.weight": z(4),
                 "transf_decoder._decoder.layers.0.third_sub_layer.dense_in.weight": z(8, 4), "transf_decoder._decoder.layers.0.third_sub_layer.dense_out.weight": z(4, 8),
                 "log_softmax.mlp.layer0.weight": z(9, 4), "log_softmax.mlp.log_softmax": z(1), "encoder_decoder_proj.weight": z(4, 4),
                 "encoder.layers.0.conv.batch_norm.num_batches_tracked": z(1), "transf_decoder._decoder.layers.0.first_sub_layer.attn_dropout.p": z(1)})
    nemo.update(att("transf_decoder._decoder.layers.0.first_sub_layer.", ("query_net", "key_net", "value_net", "out_projection")))
    nemo.update(att("transf_decoder._decoder.layers.0.second_sub_layer.", ("query_net", "key_net", "value_net", "out_projection")))
    mlx = {k: (v.transpose(0, 2, 3, 1) if v.ndim == 4 else v.transpose(0, 2, 1) if v.ndim == 3 else v) for k, v in enc.items()}
    mlx.update({"transf_decoder.token_embedding.weight": z(9, 4), "transf_decoder.embedding_layer_norm.weight": z(4), "transf_decoder.final_layer_norm.weight": z(4),
                "transf_decoder.layers.0.layer_norm_1.weight": z(4), "transf_decoder.layers.0.layer_norm_2.weight": z(4), "transf_decoder.layers.0.layer_norm_3.weight": z(4),
                "transf_decoder.layers.0.third_sub_layer.linear1.weight": z(8, 4), "transf_decoder.layers.0.third_sub_layer.linear2.weight": z(4, 8),
                "head.classifier.weight": z(9, 4)})
    mlx.update(att("transf_decoder.layers.0.first_sub_layer.", ("linear_q", "linear_k", "linear_v", "linear_out")))
    mlx.update(att("transf_decoder.layers.0.second_sub_layer.", ("linear_q", "linear_k", "linear_v", "linear_out")))
    return nemo, mlx


def test_three_checkpoint_layouts_map_to_one_key_set():
    nemo, mlx = _layouts()
    a, b = mas.canary_reference_keys(nemo), mas.canary_reference_keys(mlx)
    assert set(a) == set(b) and mas.canary_reference_keys(a) == a
    assert {k: v.shape for k, v in a.items()} == {k: v.shape for k, v in b.items()}        # the NeMo conv weights arrive channels last
    assert {"encoder.conformer.pre_encode.conv0.weight", "encoder.conformer.pre_encode.depthwise_layers.0.weight",
            "encoder.conformer.pre_encode.pointwise_layers.0.weight", "encoder.conformer.layers.0.self_attn.posBiasU", "decoder.output_proj.weight",
            "decoder.blocks.0.cross_attn.out_proj.bias", "decoder.blocks.0.ff1.weight", "decoder.blocks.0.ff_norm.weight"} <= set(a)
    assert not any("conv.1." in k or "conv.4." in k or "position_embedding" in k or "dropout" in k for k in a)
    eng = mas.canary_sanitize(nemo)
    assert set(eng) == set(mas.canary_sanitize(mlx)) == set(mas.canary_sanitize(a))
    assert {"encoder.subsampling.layers_0.weight", "encoder.subsampling.layers_3.weight", "encoder.subsampling.linear.weight",
            "encoder.layers.0.self_attn.bias_u", "encoder.layers.0.conv.norm.weight", "decoder.embedding.weight"} <= set(eng)
    assert eng["encoder.subsampling.layers_0.weight"].shape == (4, 3, 3, 1) and eng["encoder.layers.0.conv.depthwise_conv.weight"].shape == (4, 9, 1)
    assert set(CR.make_weights(CR.case_config(144, 2, d_model=128), 1)) == mas.canary_expected_keys(CR.case_config(144, 2, d_model=128))


def test_tokenizer_prompt_and_fallbacks(tmp_path):
    cfg = mas.CanaryConfig()
    (tmp_path / "tokens.txt").write_text("<|startoftranscript|> 4\n<|en|> 62\n<|de|> 76\n<|pnc|> 5\n<|notimestamp|> 11\n<|endoftext|> 9\n ▁hel 20\nlo 21\n 22\n<|x|> 23\n")
    tok = mas.CanaryTokenizer.from_model_directory(str(tmp_path), cfg)
    assert tok.token_to_id[" ▁hel"] == 20 and tok.id_to_token[22] == " "                    # the leading-space rule, the id-only line
    assert tok.build_prompt_tokens(cfg, "en", "de") == [0, 4, 2, 62, 76, 5, 11]               # fallbacks first, then only what is present
    assert tok.build_prompt_tokens(cfg, "xx", "en", pnc=False) == [0, 4, 2, 62, 11]
    assert tok.eos_token_id(cfg) == 9 and mas.CanaryTokenizer().eos_token_id(cfg) == 3
    assert tok.decode([4, 20, 21, 22, 23, 21, 999]) == "hello lo"                            # <|...|> dropped, unknown ids skipped
    assert mas.CanaryTokenizer.from_model_directory(str(tmp_path / "nothing"), cfg) is None


def test_decision_margin():
    """Over every step of every decode case the float64 top-2 logit gap is at least 100 x the float32 specification's own logit distance
    to float64 (the float32 run follows the float64 decisions).  In the eos case the rows' lengths differ and one lies strictly inside
    0..MAX_TOKENS."""
    for h, heads in CASES:
        cfg, W, enc = _case(h, heads)
        for name, bias in CR.decode_cases(W, cfg.vocab_size).items():
            Wc = dict(W); Wc["decoder.output_proj.bias"] = bias
            d64, d32 = CR.Decoder(Wc, heads, torch.float64), CR.Decoder(Wc, heads, torch.float32)
            lens = []
            for prompt, e in zip(CR.PROMPTS, enc):
                r64 = d64.generate(prompt, d64.project(e), CR.EOS, CR.MAX_TOKENS)
                follow = r64["tokens"] + [CR.EOS]
                r32 = d32.generate(prompt, d32.project(e.to(torch.float32)), CR.EOS, CR.MAX_TOKENS, follow=follow)
                err = max(float((a.double() - b).abs().max()) for a, b in zip(r32["logits"], r64["logits"]))
                print(f"h {h} {name}: gap {r64['gap']:.3e} f32 distance {err:.3e} tokens {r64['tokens']}")
                assert len(r32["logits"]) == len(r64["logits"]) and r64["gap"] >= 100 * err
                lens.append(len(r64["tokens"]))
            if name == "plain":
                assert lens == [CR.MAX_TOKENS] * 3
            elif name == "eos_first":
                assert lens == [0, 0, 0]
            else:
                assert len(set(lens)) > 1 and any(0 < n < CR.MAX_TOKENS for n in lens)
