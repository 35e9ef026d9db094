"""CPU tier of the quantised Whisper path (no GPU).

* The checkpoint key grouping of WhisperModel.from_model_directory (stt.whisper_checkpoint_plan): HF and mlx-whisper names, the tied
  proj_out.* dropped, and the two malformed cases - a uint32 `.weight` without `.scales`, `.scales` without a `quantization` entry - as
  clear errors.
* The compiled gfx950 code: the f16-scale and EPI_GELU_PACKED instantiations of the code-streaming GEMMs (k_gemm_skinny_q streaming,
  k_gemm_skinny_q1 one-shot) that Whisper's decoder step launches exist and use no scratch."""
import re

import pytest

import mlx_audio_swift_amd as mas
from mlx_audio_swift_amd.stt import whisper_checkpoint_plan

Q = {"group_size": 64, "bits": 4}


def _quant(base, sdt="F16"):
    return {base + ".weight": "U32", base + ".scales": sdt, base + ".biases": sdt}


def test_plan_groups_hf_names():
    keys = {**_quant("model.decoder.layers.0.fc1", "BF16"), "model.decoder.layers.0.fc1.bias": "BF16",
            **_quant("model.decoder.embed_tokens", "BF16"), "model.encoder.conv1.weight": "BF16",
            "proj_out.weight": "U32", "proj_out.scales": "BF16", "proj_out.biases": "BF16"}
    plan = whisper_checkpoint_plan(keys, {"group_size": 32, "bits": 8})
    assert ("quantized", "model.decoder.layers.0.fc1.weight", "model.decoder.layers.0.fc1.scales", "model.decoder.layers.0.fc1.biases",
            32, 8) in plan
    assert ("quantized", "model.decoder.embed_tokens.weight", "model.decoder.embed_tokens.scales", "model.decoder.embed_tokens.biases",
            32, 8) in plan
    assert ("dense", "model.decoder.layers.0.fc1.bias") in plan and ("dense", "model.encoder.conv1.weight") in plan
    assert len(plan) == 4                                       # proj_out.* dropped, .scales / .biases folded into their .weight
    assert not any("proj_out" in e[1] for e in plan)


def test_plan_groups_mlx_whisper_names():
    keys = {**_quant("decoder.blocks.1.attn.query"), **_quant("decoder.blocks.1.cross_attn.out"), **_quant("decoder.token_embedding"),
            **_quant("encoder.blocks.0.mlp2"), "decoder.blocks.1.attn.query.bias": "F16", "encoder.conv1.weight": "F16",
            "decoder.positional_embedding": "F16", "alignment_heads": "I64"}
    keys.pop("alignment_heads")
    plan = whisper_checkpoint_plan(keys, Q)
    quant = sorted(e[1] for e in plan if e[0] == "quantized")
    assert quant == ["decoder.blocks.1.attn.query.weight", "decoder.blocks.1.cross_attn.out.weight", "decoder.token_embedding.weight",
                     "encoder.blocks.0.mlp2.weight"]
    assert all(e[4:] == (64, 4) for e in plan if e[0] == "quantized")
    assert sorted(e[1] for e in plan if e[0] == "dense") == ["decoder.blocks.1.attn.query.bias", "decoder.positional_embedding",
                                                              "encoder.conv1.weight"]


def test_plan_without_quantization_is_dense():
    keys = {"model.decoder.layers.0.fc1.weight": "F16", "model.decoder.layers.0.fc1.bias": "F16"}
    assert whisper_checkpoint_plan(keys, None) == [("dense", "model.decoder.layers.0.fc1.bias"), ("dense", "model.decoder.layers.0.fc1.weight")]


def test_plan_uint32_weight_without_scales_is_an_error():
    keys = {"decoder.blocks.0.mlp1.weight": "U32", "decoder.blocks.0.mlp1.bias": "F16"}
    with pytest.raises(mas.AudioGenerationError, match="without .scales"):
        whisper_checkpoint_plan(keys, Q)


def test_plan_scales_without_quantization_entry_is_an_error():
    with pytest.raises(mas.AudioGenerationError, match="no quantization entry"):
        whisper_checkpoint_plan(_quant("decoder.blocks.0.mlp1"), None)
    with pytest.raises(mas.AudioGenerationError, match="companions"):
        whisper_checkpoint_plan({"decoder.blocks.0.mlp1.weight": "U32", "decoder.blocks.0.mlp1.scales": "F16"}, Q)


# k_gemm_skinny_q<MT, R, EPI, KSB, BITS, U, SBT> / k_gemm_skinny_q1<...>: EPI 0 partial, 1 bf16, 3 GELU packed; SBT 0 bf16, 1 f16 scales
_NAME = re.compile(r"k_gemm_skinny_q(1?)ILi(\d)ELi(\d)ELi(\d)ELi(\d)ELi(\d)ELi(\d)ELi(\d)EE")


def test_whisper_quantised_instantiations_exist_and_do_not_spill():
    from test_isa_cpu import HIPCC, _resource_usage
    import os
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    use = _resource_usage("lm_qgemm.hip")
    inst = {}
    for k, v in use.items():
        m = _NAME.search(k)
        if m:
            one, *t = m.groups()
            inst[(one == "1",) + tuple(int(x) for x in t)] = v
    assert inst
    for key, v in inst.items():
        assert v.get("scratch", 1) == 0 and v["vgprs"] <= 256, (key, v)
    for bits in (8, 4):
        for mt in (1, 2, 3, 4):
            u = 2 if mt <= 2 else 1
            for sbt in (0, 1):                                   # streaming: fc1 GELU (both scale dtypes), f16 slabs and vocab
                assert (False, mt, 2, 3, 4, bits, u, sbt) in inst, ("GELU", mt, bits, sbt)
            assert (False, mt, 2, 0, 4, bits, u, 1) in inst and (False, mt, 2, 1, 1, bits, u, 1) in inst, (mt, bits)
        for mt in (1, 2):                                        # one-shot: the split-K roles and fc1 at <= 32 rows
            for u in (2, 4, 6):
                for sbt in (0, 1):
                    assert (True, mt, 2, 3, 4, bits, u, sbt) in inst, ("GELU q1", mt, bits, u, sbt)
                assert (True, mt, 2, 0, 4, bits, u, 1) in inst, ("f16 q1", mt, bits, u)
