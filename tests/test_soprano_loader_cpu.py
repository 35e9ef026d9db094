"""CPU tier: the host half of SopranoModel.from_model_directory - soprano_checkpoint_plan (SopranoModel.sanitize, Soprano.swift:314-360,
and the quantisation pass of fromModelDirectory, :949-963) and SopranoConfiguration.from_model_config (the pre-1.1 decoder, :935-941)."""
import pytest

import mlx_audio_swift_amd as mas
from mlx_audio_swift_amd.soprano import soprano_checkpoint_plan

Q = {"group_size": 64, "bits": 4}


def _by_dst(plan):
    return {e[2] if e[0] == "dense" else e[4]: e for e in plan}


def test_key_forms_map_like_the_reference_sanitiser():
    dt = {"model.language_model.layers.0.input_layernorm.weight": "BF16",     # model.language_model.* -> model.*
          "language_model.layers.1.input_layernorm.weight": "BF16",            # language_model.* -> model.*
          "embed_tokens.weight": "BF16",                                       # bare inner key -> model.*
          "norm.weight": "BF16",
          "model.lm_head.weight": "BF16",                                      # model. stripped, lm_head kept
          "language_model.lm_head.weight": "F32",                              # language_model.lm_head -> lm_head
          "model.decoder.decoder.norm.weight": "BF16",
          "decoder.head.out.bias": "F16"}
    plan = soprano_checkpoint_plan(dt, None, tie_word_embeddings=False)
    assert [e[1] for e in plan] == sorted(dt)                                  # key order
    got = {e[1]: (e[2], e[3]) for e in plan}
    assert got["model.language_model.layers.0.input_layernorm.weight"] == ("model.layers.0.input_layernorm.weight", False)
    assert got["language_model.layers.1.input_layernorm.weight"] == ("model.layers.1.input_layernorm.weight", False)
    assert got["embed_tokens.weight"] == ("model.embed_tokens.weight", False)
    assert got["norm.weight"] == ("model.norm.weight", False)
    assert got["model.lm_head.weight"] == ("lm_head.weight", False)
    assert got["language_model.lm_head.weight"] == ("lm_head.weight", False)
    assert got["model.decoder.decoder.norm.weight"] == ("decoder.decoder.norm.weight", True)      # decoder tensors -> float32
    assert got["decoder.head.out.bias"] == ("decoder.head.out.bias", True)
    tied = soprano_checkpoint_plan(dt, None, tie_word_embeddings=True)
    assert all((e[2] if e[0] == "dense" else e[4]) != "lm_head.weight" for e in tied) and len(tied) == len(plan) - 2


def test_quantised_modules_keep_their_codes_and_take_global_or_per_layer_widths():
    dt = {}
    for base in ("model.language_model.layers.0.self_attn.q_proj", "language_model.layers.1.mlp.down_proj", "language_model.lm_head",
                 "decoder.decoder.convnext.0.pwconv1", "decoder.head.out"):
        dt.update({base + ".weight": "U32", base + ".scales": "BF16", base + ".biases": "BF16"})
    dt["decoder.decoder.convnext.0.pwconv1.bias"] = "BF16"
    q = {**Q, "model.layers.1.mlp.down_proj": {"group_size": 32, "bits": 8}, "decoder.head.out": {"group_size": 32, "bits": 8}}
    plan = soprano_checkpoint_plan(dt, q, tie_word_embeddings=False)
    m = _by_dst(plan)
    assert len(plan) == 6
    assert m["model.layers.0.self_attn.q_proj.weight"] == ("quantized", "model.language_model.layers.0.self_attn.q_proj.weight",
                                                           "model.language_model.layers.0.self_attn.q_proj.scales",
                                                           "model.language_model.layers.0.self_attn.q_proj.biases",
                                                           "model.layers.0.self_attn.q_proj.weight", 64, 4)
    assert m["model.layers.1.mlp.down_proj.weight"][5:] == (32, 8)                    # per-layer entry, keyed by the sanitised path
    assert m["lm_head.weight"][5:] == (64, 4)
    assert m["decoder.decoder.convnext.0.pwconv1.weight"][0] == "quantized"           # packed decoder weights are not cast
    assert m["decoder.head.out.weight"][5:] == (32, 8)
    assert m["decoder.decoder.convnext.0.pwconv1.bias"] == ("dense", "decoder.decoder.convnext.0.pwconv1.bias",
                                                            "decoder.decoder.convnext.0.pwconv1.bias", True)
    # quantization_config spelling is the same object to the plan; a tied head drops the quantised lm_head too
    assert "lm_head.weight" not in _by_dst(soprano_checkpoint_plan(dt, q, tie_word_embeddings=True))


@pytest.mark.parametrize("dt,quant", [
    ({"language_model.layers.0.mlp.up_proj.weight": "U32", "language_model.layers.0.mlp.up_proj.scales": "BF16",
      "language_model.layers.0.mlp.up_proj.biases": "BF16"}, None),                           # .scales without a quantization entry
    ({"language_model.layers.0.mlp.up_proj.scales": "BF16", "language_model.layers.0.mlp.up_proj.biases": "BF16"}, Q),   # no .weight
    ({"language_model.layers.0.mlp.up_proj.weight": "U32", "language_model.layers.0.mlp.up_proj.scales": "BF16"}, Q),    # no .biases
    ({"language_model.layers.0.mlp.up_proj.weight": "U32"}, Q),                                 # codes without .scales
    ({"language_model.layers.0.mlp.up_proj.weight": "I32"}, None),
], ids=["no-quantization-entry", "no-weight", "no-biases", "u32-without-scales", "i32-without-scales"])
def test_malformed_checkpoints_raise(dt, quant):
    with pytest.raises(mas.AudioGenerationError):
        soprano_checkpoint_plan(dt, quant, tie_word_embeddings=False)


def test_pre_1_1_repos_get_the_old_decoder():
    cj = {"hidden_size": 512, "num_hidden_layers": 17, "intermediate_size": 2304, "num_attention_heads": 4, "num_key_value_heads": 1,
          "head_dim": 128, "vocab_size": 8192}
    old = mas.SopranoConfiguration.from_model_config(cj, "mlx-community/Soprano-80M-bf16")
    assert (old.decoder_dim, old.decoder_intermediate_dim, old.input_kernel) == (512, 1536, 3)
    new = mas.SopranoConfiguration.from_model_config(cj, "mlx-community/Soprano-1.1-80M-8bit")
    assert (new.decoder_dim, new.decoder_intermediate_dim, new.input_kernel) == (768, 2304, 1)
    assert new.num_hidden_layers == 17 and new.vocab_size == 8192 and new.decoder_num_layers == 8        # SopranoConfig.swift defaults
