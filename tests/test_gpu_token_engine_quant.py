"""-m gpu: the batch-1 token engine on MLX-quantised checkpoints (csrc/token_engine_q.hip: the matrix waves stream 8- or 4-bit codes and
apply the groups' scale / bias in float32, QuantizedLinear / quantizedMatmul's arithmetic) against the oracle on the float32-dequantised
weights s*q+b and against the launch chain on the same handle.

Soprano-80M's LM widths with 2 layers and a 1 200-id vocabulary (the CFG of test_gpu_token_engine.py); every Linear quantised with
oracle.mlxquant (group 64, bf16 scales), the embedding dense.  Tolerances are the engine tests': logits max <= 0.016 x scale, rms <= 0.008
x rms, greedy ids equal wherever the oracle's margin is sure, hidden rows rms <= 0.01."""
import dataclasses
import functools
import gc

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
from gpu_util import lm_host_config, logits_errors, record
from oracle import llama as ollama
from oracle import mlxquant as mq

pytestmark = pytest.mark.gpu

CFG = ollama.LlamaConfig(hidden_size=512, num_hidden_layers=2, intermediate_size=2304, num_attention_heads=4, num_key_value_heads=1,
                         head_dim=128, vocab_size=1200, rope_theta=10000.0, rope_scaling=None, tie_word_embeddings=False, qk_norm=True,
                         rope_plain=True, rms_norm_eps=1e-6)


def quantised_lm(cfg, bits, head_q=True, seed=4321):
    """(device LM with every Linear set as MLX codes - the output projection dense unless head_q -, oracle weights: the float32 s*q+b
    of each quantised matrix, the others as they are)"""
    W = ollama.make_synthetic_weights(cfg, seed=seed)
    m = mas.LlamaTTSModel(lm_host_config(cfg))
    W32 = {}
    for k, v in W.items():
        if v.ndim == 2 and k != "model.embed_tokens.weight" and (head_q or k != "lm_head.weight"):
            wq, s, b = mq.quantize(v.float().numpy(), 64, bits)
            s16, b16 = torch.from_numpy(s).bfloat16(), torch.from_numpy(b).bfloat16()
            m.set_quantized_tensor(k, wq, s16, b16, 64, bits)
            W32[k] = torch.from_numpy(mq.dequantize(wq, s16.float().numpy(), b16.float().numpy(), 64, bits))
        else:
            m.set_tensor(k, v)
            W32[k] = v
    m.finalize()
    return m, W32


@functools.lru_cache(maxsize=None)
def _pair(bits, head_q):
    m, W32 = quantised_lm(CFG, bits, head_q)
    return m, ollama.LlamaOracle(CFG, W32, round="bf16")


@pytest.mark.parametrize("bits,head_q,xcds", [(8, True, 1), (8, True, 2), (8, True, 4), (8, True, 8), (4, True, 1), (4, True, 2), (4, True, 4),
                                              (4, True, 8), (8, False, 4), (4, False, 2)])
def test_quantised_engine_matches_the_float32_dequant_oracle_and_the_launch_chain(bits, head_q, xcds):
    dev, oracle = _pair(bits, head_q)
    want = {"qkv": bits, "o": bits, "gate_up": bits, "down": bits, "lm_head": bits if head_q else 0}
    assert dev.native_quant_bits == want
    rng = np.random.default_rng(7)
    prompt = rng.integers(0, CFG.vocab_size, 40).astype(np.int32)
    n_new = 24
    out = dev.debug_token_engine(prompt, n_new, xcds=xcds, want_logits=True, want_hidden=True)
    nxt = out["next_tokens"]
    seq = np.concatenate([prompt, nxt[len(prompt) - 1:len(prompt) - 1 + n_new]]).astype(np.int32)
    oracle.reset(1)
    ref = oracle.forward([seq])[0].numpy()
    e_max, e_rms, n_sure, agree = logits_errors(out["logits"], ref)
    assert e_max <= 0.016 and e_rms <= 0.008 and agree and n_sure > 0, (e_max, e_rms, n_sure)
    assert np.array_equal(out["logits"].argmax(1), nxt)
    hid_ref = oracle.last_hidden.numpy()
    h_rms = float(np.sqrt(np.mean((out["hidden"] - hid_ref) ** 2)) / np.sqrt(np.mean(hid_ref ** 2)))
    assert h_rms <= 0.01, h_rms
    dev.lm_reset(1, 128)
    chain = np.stack([dev.lm_forward(seq[t:t + 1])[0] for t in range(len(seq))])
    c_max, c_rms, _, c_agree = logits_errors(out["logits"], chain)
    assert c_max <= 0.016 and c_rms <= 0.008 and c_agree, (c_max, c_rms)
    record(f"token_engine_q{bits}_{'head_q' if head_q else 'head_dense'}_{xcds}xcd", logits_max_rel=e_max, logits_rms_rel=e_rms, hidden_rms_rel=h_rms,
           vs_launch_chain_max_rel=c_max, vs_launch_chain_rms_rel=c_rms, tol_max=0.016, tol_rms=0.008, ms_per_position=out["ms"] / len(seq))
    again = dev.debug_token_engine(prompt, n_new, xcds=xcds, want_logits=True)
    assert np.array_equal(again["logits"], out["logits"]) and np.array_equal(again["next_tokens"], nxt)


def test_quantised_engine_at_contexts_beyond_the_prefetched_tiles():
    dev, oracle = _pair(4, True)
    rng = np.random.default_rng(13)
    prompt = rng.integers(0, CFG.vocab_size, 280).astype(np.int32)
    out = dev.debug_token_engine(prompt, 20, xcds=4, want_logits=True)
    seq = np.concatenate([prompt, out["next_tokens"][len(prompt) - 1:len(prompt) - 1 + 20]]).astype(np.int32)
    keep = sorted({0, 15, 16, 17, 31, 32, 33, 63, 64, 127, 128, 129, 143, 144, 145, 159, 160, 161, 255, 256, 257, 271, 272, 279, 280, 299})
    oracle.reset(1)
    ref = oracle.forward([seq], logit_positions=[keep])[0].numpy()
    e_max, e_rms, n_sure, agree = logits_errors(out["logits"][keep], ref)
    assert e_max <= 0.016 and e_rms <= 0.008 and agree and n_sure > 0, (e_max, e_rms, n_sure)
    record("token_engine_q4_long_context", logits_max_rel=e_max, logits_rms_rel=e_rms, tol_max=0.016, tol_rms=0.008, positions=len(seq))


def test_quantised_generate_form_sampler_is_the_oracles_on_the_engines_own_logits():
    from oracle import sampler as osamp
    from oracle import soprano as osop
    dev, oracle = _pair(8, True)
    rng = np.random.default_rng(11)
    prompt = rng.integers(0, CFG.vocab_size, 21).astype(np.int32)
    n_new = 34
    for temp in (0.0, 0.7):
        gp = mas.GenerateParameters(max_tokens=n_new, temperature=temp, top_p=0.95, repetition_penalty=1.5, repetition_context_size=30, seed=5,
                                    row_offset=3, sampler_flavor=1)
        out = dev.debug_token_engine(prompt, n_new, xcds=4, want_logits=True, want_hidden=True, sampling=gp)
        assert out["chosen"] == n_new and out["positions"] == len(prompt) + n_new
        toks = out["next_tokens"][len(prompt) - 1:len(prompt) - 1 + n_new]
        for k in range(n_new):
            l = osop.soprano_repetition_penalty(out["logits"][k], list(toks[:k])[-30:], 1.5)
            assert toks[k] == osamp.sample(l, temp, 1.0, 5, 3, k), (temp, k)
        seq = np.concatenate([prompt, toks]).astype(np.int32)
        oracle.reset(1)
        ref_l = oracle.forward([seq])[0].numpy()
        hid_ref = oracle.last_hidden.numpy()[len(prompt) - 1:]
        assert float(np.sqrt(np.mean((out["hidden"] - hid_ref) ** 2)) / np.sqrt(np.mean(hid_ref ** 2))) <= 0.01
        e_max, e_rms, _, _ = logits_errors(out["logits"], ref_l[len(prompt) - 1:len(prompt) - 1 + n_new])
        assert e_max <= 0.016 and e_rms <= 0.008, (e_max, e_rms)


def test_quantised_engine_at_soprano_80m_depth():
    """17 layers, V = 8 192, 8-bit codes on 4 XCDs against the float32-dequant oracle, within the absolute 17-layer gate that
    test_gpu_fulldepth.py holds the dense engine to (logits max / rms <= 0.03, hidden rms <= 0.03, sure ids equal)."""
    full = dataclasses.replace(CFG, num_hidden_layers=17, vocab_size=8192)
    dev, W32 = quantised_lm(full, 8)
    rng = np.random.default_rng(23)
    prompt = rng.integers(0, full.vocab_size, 24).astype(np.int32)
    n_new = 64
    out = dev.debug_token_engine(prompt, n_new, xcds=4, want_logits=True, want_hidden=True)
    del dev
    gc.collect()
    nxt = out["next_tokens"]
    seq = np.concatenate([prompt, nxt[len(prompt) - 1:len(prompt) - 1 + n_new]]).astype(np.int32)
    o = ollama.LlamaOracle(full, W32, round="bf16")
    o.reset(1)
    ref = o.forward([seq])[0].numpy()
    e_max, e_rms, n_sure, agree = logits_errors(out["logits"], ref)
    hid = o.last_hidden.numpy()
    h_rms = float(np.sqrt(np.mean((out["hidden"] - hid) ** 2)) / np.sqrt(np.mean(hid ** 2)))
    record("token_engine_q8_soprano80m_17_layers_v8192", logits_max_rel=e_max, logits_rms_rel=e_rms, hidden_rms_rel=h_rms, tol=0.03,
           ms_per_position=out["ms"] / len(seq))
    assert agree and n_sure > 0, n_sure
    assert e_max <= 0.03 and e_rms <= 0.03 and h_rms <= 0.03, (e_max, e_rms, h_rms)
