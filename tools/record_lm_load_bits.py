"""sha256 of what tiny models compute after every way of loading LM and MLX-quantised tensors -> tests/golden/lm_load_bits.json.

    python tools/record_lm_load_bits.py [--out tests/golden/lm_load_bits.json]

tests/test_gpu_lm_load_bits.py recomputes the same hashes and asserts equality.  The load paths are host code (csrc/lm_tensor_roles.h:
which checkpoint key lands where; csrc/quant_intake.h: how an MLX affine-quantised tensor is checked, staged and dequantised), shared by
the LM handle, Whisper, Qwen3-TTS, Marvis and Soprano: a change to either header, or to one engine's use of it, must not move a bit of
what any of them computes afterwards.  The file was recorded from the engines as they were before the two headers existed (six
hand-written copies of the key parsing, five of the intake).  Regenerate it only when numerics change on purpose, and say why in that
commit.  Only the public wrappers are called, so the same file runs on any earlier commit.

main() builds every case twice, with fresh handles, and refuses to write an entry whose two hashes differ.

LM cases (two teacher-forced steps at batch 3, fixed ids, float32 logits).  Dims A: hidden 256, 2 layers, ffn 512, 2 / 1 heads x 128,
vocabulary 640, untied.  Dims B: hidden 256, 2 layers, ffn 512, 4 / 2 heads x 64, vocabulary 100, tied, qk_norm.
  dense_f32 / _f16 / _bf16   set_tensor of every key in that dtype (A)
  synthetic, synthetic_q4/8  init_synthetic, init_synthetic_quantized (A); b_synthetic (B: the q/k norm slots, the 100 -> 112 head rows)
  quant_q4 / quant_q8        every matrix as codes with bf16 scales: every role streams (A)
  quant_f16_scales           f16 scales: every role falls back to the dense copy
  quant_group32_one          layers.1.mlp.down_proj at group 32: that role falls back, the others stream
  dense_override             a dense set_tensor of a name whose role already holds codes
  tied_quant_head            a quantised lm_head.weight given to the tied model (B): skipped
  v100_quant_q4              A at vocabulary 100: the streamed head's rows padded to 112
Whisper (vocabulary 700, width 256, 2 + 2 layers; the decoder logits of one step after a fixed encode): dense synthetic; synthetic
quantised at {4, 8} bits x {bf16, f16} scales; a load with f32 scales (dequantised at intake); a load whose layer-1 q/k/v disagree in bits
(dequantised at finalize).  Qwen3-TTS (oracle.qwen3tts TINY at 8 bits, TINY_PROJ at 4): quantised embeddings, text projection, predictor
tables and LM keys; the greedy codes of two frames.  Marvis (tests/marvis_ref.py TINY at 8 bits): quantised embeddings, projection and LM
keys, q/k matrices through the row de-interleave; the forced logits of two frames.  Soprano: quantised decoder.* keys (8 bit, group 32,
widened on the host); the decoded samples of four frames."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import mlx_audio_swift_amd as mas                                   # noqa: E402
from oracle import llama as ollama                                  # noqa: E402
from oracle import mlxquant as mq                                   # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "lm_load_bits.json")
SEED = 4321
IDS = np.asarray([[5, 17, 99], [3, 40, 98]], np.int32)              # two steps x batch 3, every id below the smallest vocabulary


def _lm_cfg(**kw):
    base = dict(hidden_size=256, num_hidden_layers=2, intermediate_size=512, num_attention_heads=2, num_key_value_heads=1, head_dim=128,
                vocab_size=640, tie_word_embeddings=False)
    base.update(kw)
    return ollama.LlamaConfig(**base)


DIMS_A = _lm_cfg()
DIMS_B = _lm_cfg(num_attention_heads=4, num_key_value_heads=2, head_dim=64, vocab_size=100, tie_word_embeddings=True, qk_norm=True)
DIMS_A100 = _lm_cfg(vocab_size=100)


def host_cfg(o):
    return mas.LlamaTTSConfiguration(
        hidden_size=o.hidden_size, num_hidden_layers=o.num_hidden_layers, intermediate_size=o.intermediate_size,
        num_attention_heads=o.num_attention_heads, num_key_value_heads=o.num_key_value_heads, head_dim=o.head_dim,
        rms_norm_eps=o.rms_norm_eps, vocab_size=o.vocab_size, rope_theta=o.rope_theta,
        rope_scaling=dict(o.rope_scaling) if o.rope_scaling else None, tie_word_embeddings=o.tie_word_embeddings, qk_norm=o.qk_norm,
        rope_plain=o.rope_plain, rope_ops_in_dtype=o.rope_ops_in_dtype)


def digest(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + repr(tuple(a.shape)).encode() + a.tobytes())
    return h.hexdigest()


def quantised(v, group, bits, sdt=torch.bfloat16):
    wq, s, b = mq.quantize(torch.as_tensor(v).float().numpy(), group, bits)
    return np.asarray(wq, np.uint32), torch.from_numpy(np.asarray(s, np.float32)).to(sdt), torch.from_numpy(np.asarray(b, np.float32)).to(sdt), group, bits


def lm_logits(m) -> str:
    """the calls of tests/gpu_util.py teacher_forced: one lm_reset, one lm_forward per step"""
    try:
        m.lm_reset(IDS.shape[1], 64)
        out = [np.asarray(m.lm_forward(IDS[t]), np.float32).copy() for t in range(IDS.shape[0])]
        assert out[0].shape == (IDS.shape[1], m.configuration.vocab_size)
        return digest(*out)
    finally:
        m.close()


def lm_dense(dtype):
    def case():
        W = ollama.make_synthetic_weights(DIMS_A, seed=SEED)
        return lm_logits(mas.LlamaTTSModel.from_weights(host_cfg(DIMS_A), {k: v.to(dtype) for k, v in W.items()}))
    return case


def lm_synthetic(cfg, bits=None):
    return lambda: lm_logits(mas.LlamaTTSModel.synthetic(host_cfg(cfg), seed=SEED, quant_bits=bits))


def lm_quant(cfg, spec, want, after=None, extra=None):
    """spec(key) -> (group, bits, scale dtype) for every matrix; want: native_quant_bits after finalize; after(m, W): calls between the
    load and finalize; extra(m, W): calls before the load"""
    def case():
        W = ollama.make_synthetic_weights(cfg, seed=SEED)
        m = mas.LlamaTTSModel(host_cfg(cfg))
        if extra:
            extra(m, W)
        for k, v in W.items():
            if v.ndim == 2:
                g, b, sdt = spec(k)
                m.set_quantized_tensor(k, *quantised(v, g, b, sdt))
            else:
                m.set_tensor(k, v)
        if after:
            after(m, W)
        m.finalize()
        got = m.native_quant_bits
        assert got == dict(zip(("qkv", "o", "gate_up", "down", "lm_head"), want)), got
        return lm_logits(m)
    return case


def _uniform(bits, sdt=torch.bfloat16):
    return lambda k: (64, bits, sdt)


def _tied_head(m, W):
    v = ollama.make_synthetic_weights(_lm_cfg(num_attention_heads=4, num_key_value_heads=2, head_dim=64, vocab_size=100, qk_norm=True), seed=SEED)
    m.set_quantized_tensor("lm_head.weight", *quantised(v["lm_head.weight"], 64, 8))


LM_CASES = {
    "lm.dense_f32": lm_dense(torch.float32), "lm.dense_f16": lm_dense(torch.float16), "lm.dense_bf16": lm_dense(torch.bfloat16),
    "lm.synthetic": lm_synthetic(DIMS_A), "lm.synthetic_q4": lm_synthetic(DIMS_A, 4), "lm.synthetic_q8": lm_synthetic(DIMS_A, 8),
    "lm.b_synthetic": lm_synthetic(DIMS_B),
    "lm.quant_q4": lm_quant(DIMS_A, _uniform(4), [4] * 5), "lm.quant_q8": lm_quant(DIMS_A, _uniform(8), [8] * 5),
    "lm.quant_f16_scales": lm_quant(DIMS_A, _uniform(4, torch.float16), [0] * 5),
    "lm.quant_group32_one": lm_quant(DIMS_A, lambda k: (32, 8, torch.bfloat16) if k == "model.layers.1.mlp.down_proj.weight" else (64, 4, torch.bfloat16),
                                     [4, 4, 4, 0, 4]),
    "lm.dense_override": lm_quant(DIMS_A, _uniform(4), [4, 0, 4, 4, 4],
                                  after=lambda m, W: m.set_tensor("model.layers.0.self_attn.o_proj.weight", W["model.layers.1.self_attn.o_proj.weight"])),
    "lm.tied_quant_head": lm_quant(DIMS_B, _uniform(8), [8, 8, 8, 8, 0], extra=_tied_head),
    "lm.v100_quant_q4": lm_quant(DIMS_A100, _uniform(4), [4] * 5),
}


# ---------------------------------------------------------------------------------------------------------------- Whisper
def _whisper_cfg():
    from oracle import whisper as ow
    return ow.WhisperConfig(vocab_size=700, num_mel_bins=80, d_model=256, encoder_layers=2, encoder_attention_heads=4, encoder_ffn_dim=1024,
                            decoder_layers=2, decoder_attention_heads=4, decoder_ffn_dim=1024)


def _whisper_host(c):
    return mas.WhisperConfig(**{k: getattr(c, k) for k in mas.WhisperConfig.__dataclass_fields__})


def whisper_logits(m) -> str:
    try:
        i = np.arange(2 * 3000 * 80, dtype=np.int64)
        feats = ((((i * 2654435761) >> 7) % 2001).astype(np.float32) / 1000.0 - 1.0).reshape(2, 3000, 80)
        m.encode(feats, want_output=False)
        m.decoder_reset()
        return digest(np.asarray(m.decoder_forward(np.asarray([11, 650], np.int64)), np.float32))
    finally:
        m.close()


def whisper_synthetic(bits=None, sdt="bf16"):
    return lambda: whisper_logits(mas.WhisperModel.synthetic(_whisper_host(_whisper_cfg()), seed=777, quant_bits=bits, scale_dtype=sdt))


def whisper_load(spec):
    """spec(key) -> (group, bits, scale dtype) for every Linear and the token embedding"""
    def case():
        from oracle import whisper as ow
        cfg = _whisper_cfg()
        W = ow.make_synthetic_weights(cfg, seed=777)
        m = mas.WhisperModel(_whisper_host(cfg))
        for k, v in W.items():
            if k.endswith(".weight") and v.dim() == 2 and "embed_positions" not in k and "layer_norm" not in k:
                g, b, sdt = spec(k)
                m.set_quantized_tensor(k, *quantised(v, g, b, sdt))
            else:
                m.set_tensor(k, v)
        m.finalize()
        return whisper_logits(m)
    return case


WHISPER_CASES = {
    "whisper.synthetic": whisper_synthetic(),
    **{f"whisper.synthetic_q{b}_{s}": whisper_synthetic(b, s) for b in (4, 8) for s in ("bf16", "f16")},
    "whisper.quant_f32_scales": whisper_load(lambda k: (64, 4, torch.float32)),
    "whisper.quant_mixed_qkv": whisper_load(lambda k: (64, 8 if k == "model.decoder.layers.1.self_attn.q_proj.weight" else 4, torch.bfloat16)),
}


# ---------------------------------------------------------------------------------------------------------------- Qwen3-TTS
def qwen3tts(name, bits):
    def case():
        from oracle import qwen3tts as oq
        o = getattr(oq, name)
        dec = mas.Qwen3TTSDecoderConfiguration(**{k: getattr(o.decoder, k) for k in mas.Qwen3TTSDecoderConfiguration.__dataclass_fields__})
        cfg = mas.Qwen3TTSConfiguration(
            talker=host_cfg(o.talker), predictor=host_cfg(o.predictor), num_code_groups=o.num_code_groups, text_hidden_size=o.text_hidden_size,
            text_vocab_size=o.text_vocab_size, codec_eos_token_id=o.codec_eos_token_id, codec_think_id=o.codec_think_id,
            codec_nothink_id=o.codec_nothink_id, codec_think_bos_id=o.codec_think_bos_id, codec_think_eos_id=o.codec_think_eos_id,
            codec_pad_id=o.codec_pad_id, codec_bos_id=o.codec_bos_id, tts_pad_token_id=o.tts_pad_token_id, tts_bos_token_id=o.tts_bos_token_id,
            tts_eos_token_id=o.tts_eos_token_id, decoder=dec)
        dev = mas.Qwen3TTSModel(cfg)
        try:
            for k, v in oq.make_synthetic_weights(o).items():
                v = torch.as_tensor(v)
                if v.ndim == 2 and v.shape[1] % 64 == 0:
                    dev.set_quantized_tensor("talker." + k, *quantised(v, 64, bits))
                else:
                    dev.set_tensor("talker." + k, v)
            for k, v in oq.make_synthetic_decoder_weights(o.decoder).items():
                dev.set_tensor(k, v)
            dev.finalize()
            rng = np.random.default_rng(2)

            def prompt(n_text, n_trail):
                text = list(rng.integers(0, o.text_vocab_size - 20, n_text))
                t = text[4:] + text[:3] + [o.tts_pad_token_id] * 2 + [o.tts_bos_token_id] + [text[3]]
                c = [-1] * (len(text) - 4) + [-1, -1, -1, o.codec_nothink_id, o.codec_think_bos_id, o.codec_think_eos_id, o.codec_bos_id]
                trailing = list(rng.integers(0, o.text_vocab_size - 20, n_trail)) + [o.tts_eos_token_id]
                return mas.PreparedPrompt(np.asarray(t, np.int32), np.asarray(c, np.int32), np.asarray(trailing, np.int32), 0)
            gp = mas.Qwen3TTSGenerateParameters(max_tokens=2, temperature=0.0, repetition_penalty=1.05, seed=1)
            codes = dev.generate_codes([prompt(9, 3), prompt(4, 1), prompt(6, 5)], gp)
            return digest(*[np.asarray(c, np.int32) for c in codes])
        finally:
            dev.close()
    return case


# ---------------------------------------------------------------------------------------------------------------- Marvis
def marvis(bits):
    def case():
        import marvis_ref as mr
        from mlx_audio_swift_amd import marvis as mv
        cfg = mr.TINY

        def lm_json(c):
            return dict(hidden_size=c.hidden_size, num_hidden_layers=c.num_hidden_layers, intermediate_size=c.intermediate_size,
                        num_attention_heads=c.num_attention_heads, num_key_value_heads=c.num_key_value_heads, head_dim=c.resolved_head_dim,
                        rms_norm_eps=c.rms_norm_eps, rope_theta=c.rope_theta, rope_scaling=dict(c.rope_scaling), max_position_embeddings=2048)
        cj = dict(model_type="csm", text_vocab_size=cfg.text_vocab_size, audio_vocab_size=cfg.audio_vocab_size,
                  audio_num_codebooks=cfg.audio_num_codebooks, **lm_json(cfg.backbone),
                  depth_decoder_config=dict(vocab_size=cfg.audio_vocab_size, num_codebooks=cfg.audio_num_codebooks, **lm_json(cfg.decoder)),
                  quantization=dict(group_size=64, bits=bits))
        W = {k: (quantised(v, 64, bits) if v.ndim == 2 and k != "model.audio_head" else v) for k, v in mr.make_weights(cfg).items()}
        dev = mas.MarvisTTSModel.from_weights(mas.CSMModelArgs.from_json(cj), W)
        try:
            assert dev.native_quant_bits() == [[bits] * 5, [bits] * 4 + [0]]
            rng = np.random.default_rng(2)
            K = cfg.audio_num_codebooks
            prompts = [mv.tokenize_segment(rng.integers(0, cfg.text_vocab_size, nt), rng.integers(1, cfg.audio_vocab_size, (K, na)), K, add_eos=False)
                       for nt, na in ((9, 3), (4, 1), (6, 5))]
            gp = mas.MarvisGenerateParameters(max_frames=2, quality_level=8, temperature=0.0, seed=1)
            forced = np.stack(dev.generate_codes(prompts, gp))
            logits, sampled, nf = dev.forced_logits(prompts, forced, gp)
            return digest(np.asarray(logits, np.float32), np.asarray(sampled, np.int32), np.asarray(nf, np.int32))
        finally:
            dev.close()
    return case


# ---------------------------------------------------------------------------------------------------------------- Soprano
def soprano():
    from oracle import soprano as osop
    lm = _lm_cfg(rope_theta=10000.0, rope_scaling=None, qk_norm=True, rope_plain=True, rms_norm_eps=1e-6)
    dec = dict(decoder_num_layers=2, decoder_dim=96, decoder_intermediate_dim=160, hop_length=32, n_fft=128, upscale=4, input_kernel=3,
               dw_kernel=3, token_size=128)
    cfg = mas.SopranoConfiguration(hidden_size=lm.hidden_size, num_hidden_layers=lm.num_hidden_layers, intermediate_size=lm.intermediate_size,
                                   num_attention_heads=lm.num_attention_heads, num_key_value_heads=lm.num_key_value_heads, head_dim=lm.head_dim,
                                   vocab_size=lm.vocab_size, rms_norm_eps=lm.rms_norm_eps, rope_theta=lm.rope_theta, tie_word_embeddings=False,
                                   stop_token_id=3, **dec)
    quant = ("decoder.decoder.convnext.0.pwconv1.weight", "decoder.decoder.convnext.0.pwconv2.weight", "decoder.decoder.convnext.1.pwconv1.weight",
             "decoder.decoder.convnext.1.pwconv2.weight", "decoder.head.out.weight")
    m = mas.SopranoModel(cfg)
    try:
        for k, v in ollama.make_synthetic_weights(lm, seed=SEED).items():
            m.set_tensor(k, v)
        Wd = osop.make_synthetic_weights(osop.SopranoDecoderConfig(hidden_size=lm.hidden_size, **dec), seed=99)
        assert all(k in Wd for k in quant)
        for k, v in Wd.items():
            if k in quant:
                m.set_quantized_tensor(k, *quantised(v, 32, 8))
            else:
                m.set_tensor(k, v)
        m.finalize()
        i = np.arange(4 * lm.hidden_size, dtype=np.int64)
        hidden = ((((i * 2246822519) >> 9) % 4001).astype(np.float32) / 1000.0 - 2.0).reshape(1, 4, lm.hidden_size)
        return digest(np.asarray(m.decode(hidden), np.float32))
    finally:
        m.close()


CASES = {**LM_CASES, **WHISPER_CASES, "qwen3tts.tiny_q8": qwen3tts("TINY", 8), "qwen3tts.tiny_proj_q4": qwen3tts("TINY_PROJ", 4),
         "marvis.tiny_q8": marvis(8), "soprano.quant_decoder": soprano}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    got, unstable = {}, []
    for name, fn in CASES.items():
        a, b = fn(), fn()
        print(name, a, "" if a == b else f"!= second build {b}", flush=True)
        if a == b:
            got[name] = a
        else:
            unstable.append(name)
    with open(args.out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    if unstable:
        sys.exit("not written (two builds of the case disagree): " + ", ".join(unstable))


if __name__ == "__main__":
    main()
