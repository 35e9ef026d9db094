"""-m gpu: SopranoModel.from_model_directory (SopranoModel.fromModelDirectory, Soprano.swift:926-979) on synthetic checkpoint directories in
MLX's key layout - bf16, and MLX-quantised (uint32 codes + bf16 scales / biases; decoder pwconv1 / pwconv2 / head.out quantised too) - and
batch-1 generate on them: the quantised LM runs on the code-streaming token engine (lm_path 1) and the audio is the oracle decoder's on the
engine's own hidden rows (decoder tolerance of test_gpu_soprano.py: 2e-4 x max |ref|)."""
import json

import numpy as np
import pytest
import torch
from safetensors.torch import save_file

import mlx_audio_swift_amd as mas
from oracle import llama as ollama
from oracle import mlxquant as mq
from oracle import soprano as osop

pytestmark = pytest.mark.gpu

LM = ollama.LlamaConfig(hidden_size=512, num_hidden_layers=2, intermediate_size=2304, num_attention_heads=4, num_key_value_heads=1,
                        head_dim=128, vocab_size=1200, rope_theta=10000.0, rope_scaling=None, tie_word_embeddings=False, qk_norm=True,
                        rope_plain=True, rms_norm_eps=1e-6)
DEC = dict(decoder_num_layers=2, decoder_dim=96, decoder_intermediate_dim=160, hop_length=32, n_fft=128, upscale=4, input_kernel=3,
           dw_kernel=3, token_size=128)
DEC_Q = ("decoder.decoder.convnext.0.pwconv1", "decoder.decoder.convnext.0.pwconv2", "decoder.decoder.convnext.1.pwconv1",
         "decoder.decoder.convnext.1.pwconv2", "decoder.head.out")
GP = mas.GenerateParameters(max_tokens=12, temperature=0.0, top_p=0.95, repetition_penalty=1.5, repetition_context_size=30, seed=1,
                            sampler_flavor=1)


def _stored_key(k):
    """an LM key as MLX conversions store it: three of the sanitiser's input forms"""
    if k == "lm_head.weight":
        return "language_model.lm_head.weight"
    if k.startswith("model.layers."):
        return "model.language_model." + k[len("model."):]
    return k[len("model."):]                                               # bare inner keys (embed_tokens, norm)


def _write(path, tensors):
    """safetensors with the packed words as U32, as MLX writes them (torch has no uint32: written as I32, header dtype patched)"""
    save_file(tensors, path)
    raw = open(path, "rb").read()
    n = int.from_bytes(raw[:8], "little")
    hdr = json.loads(raw[8:8 + n])
    for k in hdr:
        if k != "__metadata__" and hdr[k]["dtype"] == "I32":
            hdr[k]["dtype"] = "U32"
    hb = json.dumps(hdr, separators=(",", ":")).encode()
    hb += b" " * ((8 - len(hb) % 8) % 8)
    open(path, "wb").write(len(hb).to_bytes(8, "little") + hb + raw[8 + n:])


def _directory(root, name, bits, dense_override=None):
    """(directory, oracle LM weights, oracle decoder weights, raw LM weights, raw decoder weights).  bits 8 / 4: every LM Linear
    quantised at `bits` / group 64 (the embedding stays dense) - `dense_override` through a per-layer entry at group 32, which the LM
    dequantises at load -, decoder matrices at 8 bit / group 32 through per-layer entries.  bits None: a plain bf16 / float32 directory."""
    Wl = ollama.make_synthetic_weights(LM, seed=4321)
    Wd = osop.make_synthetic_weights(osop.SopranoDecoderConfig(hidden_size=LM.hidden_size, **DEC), seed=99)
    d = root / name
    d.mkdir()
    quant = None if bits is None else {"group_size": 64, "bits": bits, **{m: {"group_size": 32, "bits": 8} for m in DEC_Q}}
    if dense_override:
        quant[dense_override] = {"group_size": 32, "bits": 8}
    tensors = {}

    def put(stored, module, v, quantise):
        if quant is None or not quantise:
            tensors[stored] = v.contiguous() if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))
            return v
        g, b = (quant[module]["group_size"], quant[module]["bits"]) if module in quant else (64, bits)
        wq, s, bia = mq.quantize(torch.as_tensor(v).float().numpy(), g, b)
        s16, b16 = torch.from_numpy(s).bfloat16(), torch.from_numpy(bia).bfloat16()
        base = stored[: -len(".weight")]
        tensors[stored] = torch.from_numpy(wq.view(np.int32))
        tensors[base + ".scales"], tensors[base + ".biases"] = s16, b16
        return mq.dequantize(wq, s16.float().numpy(), b16.float().numpy(), g, b)

    Wl32 = {}
    for k, v in Wl.items():
        r = put(_stored_key(k), k[: -len(".weight")], v, v.ndim == 2 and k != "model.embed_tokens.weight")
        Wl32[k] = torch.from_numpy(r) if isinstance(r, np.ndarray) else r
    Wd32 = {k: put(k, k[: -len(".weight")], v, k[: -len(".weight")] in DEC_Q) for k, v in Wd.items()}
    cj = dict(hidden_size=LM.hidden_size, num_hidden_layers=LM.num_hidden_layers, intermediate_size=LM.intermediate_size,
              num_attention_heads=LM.num_attention_heads, num_key_value_heads=LM.num_key_value_heads, head_dim=LM.head_dim,
              vocab_size=LM.vocab_size, rms_norm_eps=LM.rms_norm_eps, rope_theta=LM.rope_theta, tie_word_embeddings=False,
              stop_token_id=-1, **DEC)
    if quant is not None:
        cj["quantization"] = quant
    (d / "config.json").write_text(json.dumps(cj))
    _write(str(d / "model.safetensors"), tensors)
    return d, Wl32, Wd32, Wl, Wd


def _prompt():
    return np.random.default_rng(2).integers(4, LM.vocab_size, 9).astype(np.int32)


@pytest.mark.parametrize("bits", [8, 4])
def test_quantised_directory_generates_on_the_code_streaming_engine(tmp_path, bits, monkeypatch):
    monkeypatch.delenv("MIS_TOKEN_ENGINE", raising=False)
    d, Wl32, Wd32, _, _ = _directory(tmp_path, "Soprano-1.1-q", bits)
    dev = mas.SopranoModel.from_model_directory(str(d))
    assert (dev.configuration.decoder_dim, dev.configuration.input_kernel) == (96, 3)       # "soprano-1.1" in the name: config.json's decoder
    assert dev.lm.native_quant_bits == {"qkv": bits, "o": bits, "gate_up": bits, "down": bits, "lm_head": bits}
    prompt = _prompt()
    pcm, toks = dev.generate_batch([prompt], GP, return_tokens=True)
    assert dev.lm_path == 1
    assert len(toks[0]) == 12 and pcm[0].shape == (12 * DEC["token_size"],)
    # the audio: the oracle decoder (float32 s*q+b decoder matrices) on the engine's own hidden rows of the same request
    eng = dev.lm.debug_token_engine(prompt, 12, xcds=4, want_hidden=True, sampling=GP, stop_id=-1)
    assert np.array_equal(eng["next_tokens"][len(prompt) - 1:len(prompt) + 11], toks[0])
    odec = osop.SopranoDecoderOracle(osop.SopranoDecoderConfig(hidden_size=LM.hidden_size, **DEC), Wd32)
    ref = odec.decode(eng["hidden"][None])[0]
    assert pcm[0].shape == ref.shape and np.abs(pcm[0] - ref).max() <= 2e-4 * np.abs(ref).max()
    # the engine's hidden rows: the oracle LM's on the float32-dequantised weights under teacher forcing, within 1 % rms
    olm = ollama.LlamaOracle(LM, Wl32, round="bf16")
    olm.reset(1)
    olm._forward_row(0, torch.as_tensor(np.asarray(list(prompt) + list(toks[0]), np.int64)))
    hid_ref = olm.last_hidden.numpy()[len(prompt) - 1:]
    assert float(np.sqrt(np.mean((eng["hidden"] - hid_ref) ** 2)) / np.sqrt(np.mean(hid_ref ** 2))) <= 0.01
    # generateStream: the same ids and samples
    evs = list(dev.generate_stream_batch([prompt], GP))
    assert dev.lm_path == 1
    ids = [e.token for e in evs if isinstance(e, mas.TokenEvent)]
    audio = [e.audio for e in evs if isinstance(e, mas.AudioEvent)]
    assert ids == [int(t) for t in toks[0]] and len(audio) == 1 and np.array_equal(audio[0], pcm[0])


def test_bf16_directory_equals_from_weights(tmp_path, monkeypatch):
    monkeypatch.delenv("MIS_TOKEN_ENGINE", raising=False)
    d, _, _, Wl, Wd = _directory(tmp_path, "Soprano-1.1-bf16", None)
    dev = mas.SopranoModel.from_pretrained(str(d))
    Wall = {(k[len("model."):] if k.startswith("model.") else k): v for k, v in Wl.items()}
    Wall.update(Wd)
    ref = mas.SopranoModel.from_weights(dev.configuration, Wall)
    a, ta = dev.generate_batch([_prompt()], GP, return_tokens=True)
    assert dev.lm_path == 1
    b, tb = ref.generate_batch([_prompt()], GP, return_tokens=True)
    assert np.array_equal(ta[0], tb[0]) and np.array_equal(a[0], b[0])


def test_directory_with_a_dense_role_falls_back_to_the_launch_chain(tmp_path, monkeypatch):
    """A per-layer override (group 32) leaves o_proj of one layer dequantised at load, so the o_proj role is dense: the engine does not
    take mixed roles and the launch chain runs the request (lm_path 0).  Its ids are the oracle's greedy choice under teacher forcing
    within the logit tolerance, and its audio is the oracle decoder on the oracle LM's hidden rows for those ids."""
    from oracle import soprano as osop_
    monkeypatch.delenv("MIS_TOKEN_ENGINE", raising=False)
    d, Wl32, Wd32, _, _ = _directory(tmp_path, "Soprano-1.1-mixed", 8, dense_override="model.layers.1.self_attn.o_proj")
    dev = mas.SopranoModel.from_model_directory(str(d))
    assert dev.lm.native_quant_bits["o"] == 0 and dev.lm.native_quant_bits["qkv"] == 8
    prompt = _prompt()
    pcm, toks = dev.generate_batch([prompt], GP, return_tokens=True)
    assert dev.lm_path == 0 and len(toks[0]) == 12
    olm = ollama.LlamaOracle(LM, Wl32, round="bf16")
    olm.reset(1)
    seq = list(prompt) + list(toks[0])
    lg = olm._forward_row(0, torch.as_tensor(np.asarray(seq, np.int64))).numpy()
    hid = olm.last_hidden.numpy()[len(prompt) - 1:]
    tol = 0.04 * float(np.abs(lg).max())
    for i, t in enumerate(toks[0]):
        l = osop_.soprano_repetition_penalty(lg[len(prompt) - 1 + i], list(toks[0][:i])[-30:], 1.5)
        assert l[t] >= l.max() - tol, i
    odec = osop.SopranoDecoderOracle(osop.SopranoDecoderConfig(hidden_size=LM.hidden_size, **DEC), Wd32)
    ref = odec.decode(hid[None])[0]
    assert pcm[0].shape == ref.shape
    assert float(np.sqrt(np.mean((pcm[0] - ref) ** 2)) / np.sqrt(np.mean(ref ** 2))) <= 0.05
