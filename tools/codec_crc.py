"""CRC-32 of what the seven exact-f32 codec engines compute (SNAC, DAC, EnCodec, Mimi, the Qwen3-TTS speech-tokenizer decoder, the
tokenizer encoder of q3_reference.hip - reached through Mimi's encode - and Soprano's decoder): every engine is built as its GPU test
builds it at that test's smallest configuration, at batch 2 and a frame count that is no multiple of any tile, and runs decode, encode where it has one,
and - Mimi and Qwen3-TTS - a streaming decode in chunks of 1, 2 and 3 frames.  One JSON line per engine with the CRC-32 of every output
buffer.  Run it once per library build (MIS_LIB_PATH selects the library): two builds that print the same lines compute the same bits,
which the parity tolerances of the tests would not show."""
import json, os, sys, zlib
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mlx_audio_swift_amd as mas
from oracle import dac as od, encodec as oe, snac as osnac, soprano as osop, llama as ollama, qwen3tts as oq
import mimi_ref as mr
from gpu_util import lm_host_config


def q3_host_cfg(o):
    dec = mas.Qwen3TTSDecoderConfiguration(**{k: getattr(o.decoder, k) for k in mas.Qwen3TTSDecoderConfiguration.__dataclass_fields__})
    return mas.Qwen3TTSConfiguration(
        talker=lm_host_config(o.talker), predictor=lm_host_config(o.predictor), num_code_groups=o.num_code_groups,
        text_hidden_size=o.text_hidden_size, text_vocab_size=o.text_vocab_size, codec_eos_token_id=o.codec_eos_token_id,
        codec_think_id=o.codec_think_id, codec_nothink_id=o.codec_nothink_id, codec_think_bos_id=o.codec_think_bos_id,
        codec_think_eos_id=o.codec_think_eos_id, codec_pad_id=o.codec_pad_id, codec_bos_id=o.codec_bos_id,
        tts_pad_token_id=o.tts_pad_token_id, tts_bos_token_id=o.tts_bos_token_id, tts_eos_token_id=o.tts_eos_token_id, decoder=dec)

B = 2


def crc(a) -> str:
    return "%08x" % zlib.crc32(np.ascontiguousarray(a).tobytes())


def chunked(step, codes, sizes=(1, 2, 3)):
    """the frames of codes [B][nq][T] through step() in chunks of 1, 2, 3, 1, 2, 3, ... frames"""
    out, a, i = [], 0, 0
    while a < codes.shape[-1]:
        b = min(codes.shape[-1], a + sizes[i % len(sizes)])
        out.append(step(codes[:, :, a:b]))
        a, i = b, i + 1
    return np.concatenate(out, -1)


def snac():
    ocfg = osnac.SnacConfig(**osnac.TINY)
    W = osnac.make_synthetic_weights(ocfg, with_encoder=True)
    dev = mas.SNAC.from_weights(mas.SNACConfig(**{k: getattr(ocfg, k) for k in mas.SNACConfig.__dataclass_fields__}), W)
    codes, noise = osnac.synthetic_codes(ocfg, B, 7), osnac.synthetic_noise(ocfg, B, 7)
    audio = (0.3 * np.random.default_rng(4).standard_normal((B, 1000))).astype(np.float32)
    ecodes, z = dev.encode(audio, return_latent=True)
    return {"decode": crc(dev.decode(codes, noise)), "encode_z": crc(z), "encode_codes": [crc(c) for c in ecodes]}


def dac():
    ocfg = od.TINY
    W = od.make_synthetic_weights(ocfg)
    dev = mas.DescriptDAC.from_weights(mas.DescriptDACConfig(**{k: getattr(ocfg, k) for k in mas.DescriptDACConfig.__dataclass_fields__}), W)
    codes = np.random.default_rng(0).integers(0, ocfg.codebook_size, (B, ocfg.n_codebooks, 7)).astype(np.int32)
    hop = int(np.prod(ocfg.encoder_rates))
    audio = (0.3 * np.random.default_rng(5).standard_normal((B, 9 * hop - 3))).astype(np.float32)
    ecodes, z = dev.encode(audio, return_latent=True)
    return {"decode": crc(dev.decode_from_codes(codes)), "encode_z": crc(z), "encode_codes": crc(ecodes)}


def encodec():
    out = {}
    for name, ocfg in (("tiny", oe.TINY), ("tiny_48k", oe.TINY_48K)):
        W = oe.make_synthetic_weights(ocfg)
        fields = {k: getattr(ocfg, k) for k in mas.EncodecConfig.__dataclass_fields__ if hasattr(ocfg, k)}
        dev = mas.Encodec.from_weights(mas.EncodecConfig(**fields), W)
        codes = np.random.default_rng(0).integers(0, ocfg.codebook_size, (B, ocfg.num_quantizers, 9)).astype(np.int32)
        out["decode_" + name] = crc(dev.decode_frame(codes, scale=0.5))
    return out


def _mimi():
    c = mr.TINY
    return c, mas.Mimi.from_weights(mas.MimiConfig(
        num_codebooks=c.num_quantizers, sample_rate=c.sample_rate, frame_rate=c.frame_rate, dimension=c.dimension, n_filters=c.n_filters,
        n_residual_layers=c.n_residual_layers, ratios=list(c.ratios), kernel_size=c.kernel_size, residual_kernel_size=c.residual_kernel_size,
        last_kernel_size=c.last_kernel_size, dilation_base=c.dilation_base, compress=c.compress, num_layers=c.num_layers,
        num_heads=c.num_heads, dim_feedforward=c.dim_feedforward, context=c.context, max_period=c.max_period, bins=c.bins,
        quantizer_dim=c.quantizer_dim), mr.make_synthetic_weights(c))


def mimi():
    c, dev = _mimi()
    codes = mr.synthetic_codes(c, B, 8, 13, seed=11)
    sd = mas.MimiStreamingDecoder(dev, batch=B)
    out = {"decode": crc(dev.decode(codes)), "stream_123": crc(chunked(sd.decode_frames, codes))}
    dev.close()
    return out


def q3_reference():
    c, dev = _mimi()
    audio = (0.3 * np.random.default_rng(2).standard_normal((B, 1, 6 * 2 * 23 + 5))).astype(np.float32)
    out = {"encode_codes": crc(dev.encode(audio)), "encode_codes_nq3": crc(dev.encode(audio, n_q=3))}
    dev.close()
    return out


def qwen3tts():
    ocfg = oq.TINY
    allw = {("talker." + k): v for k, v in oq.make_synthetic_weights(ocfg).items()}
    allw.update(oq.make_synthetic_decoder_weights(ocfg.decoder))
    dev = mas.Qwen3TTSModel.from_weights(q3_host_cfg(ocfg), allw)
    d = ocfg.decoder
    codes = np.random.default_rng(11).integers(0, d.codebook_size, (B, d.num_quantizers, 13)).astype(np.int32)
    out = {"decode": crc(dev.decode_codes(codes))}
    for exact in (True, False):          # False: the reference's arithmetic (bias twice after a chunk boundary)
        dev.set_stream_exact(exact)
        dev.reset_streaming_state(batch=B, max_frames=13, max_chunk_frames=3)
        out["stream_123_exact" if exact else "stream_123"] = crc(chunked(dev.streaming_step, codes))
    dev.end_streaming()
    return out


def soprano():
    LM = ollama.TINY_QWEN3
    base = dict(decoder_num_layers=2, decoder_dim=96, decoder_intermediate_dim=160, hop_length=32, n_fft=128, upscale=4, input_kernel=3,
                dw_kernel=3, token_size=128)
    cfg = mas.SopranoConfiguration(hidden_size=LM.hidden_size, num_hidden_layers=LM.num_hidden_layers, intermediate_size=LM.intermediate_size,
                                   num_attention_heads=LM.num_attention_heads, num_key_value_heads=LM.num_key_value_heads,
                                   head_dim=LM.head_dim, vocab_size=LM.vocab_size, rms_norm_eps=LM.rms_norm_eps, rope_theta=LM.rope_theta,
                                   tie_word_embeddings=False, stop_token_id=3, **base)
    W = dict(ollama.make_synthetic_weights(LM, seed=4321))
    W.update(osop.make_synthetic_weights(osop.SopranoDecoderConfig(hidden_size=LM.hidden_size, **base), seed=99))
    dev = mas.SopranoModel.from_weights(cfg, W)
    hid = np.random.default_rng(0).standard_normal((B, 9, cfg.hidden_size)).astype(np.float32)
    return {"decode": crc(dev.decode(hid))}


for name, fn in (("snac", snac), ("dac", dac), ("encodec", encodec), ("mimi", mimi), ("q3_reference", q3_reference), ("q3_codec", qwen3tts), ("soprano", soprano)):
    print(json.dumps({"engine": name, **fn()}), flush=True)
