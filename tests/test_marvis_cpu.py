"""CPU tier for Marvis / CSM: the q/k de-interleave and CSM's RoPE tables pinned on independent implementations, token frames, the
prompt limit, text pieces, both config shapes, the key map, the quantised checkpoint plan, and register bounds of the new kernels."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
from mlx_audio_swift_amd import marvis as mv
from oracle import llama as ollama
from oracle import mlxquant

import marvis_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.parametrize("D", [64, 128])
def test_csm_rope_tables_bit_for_bit(D):
    """Three statements of ropeInit / applyScaling agree bit for bit: the scalar literal (marvis_ref), the host mirror's vectorised one,
    and the engine's (csrc/marvis.hip, host arithmetic - no GPU needed).  This pins the three against each other, not against MLX: all
    share the choice of a correctly rounded float32 power, which MLX's pow is not known to make."""
    lit_c, lit_s = mr.rope_init_literal(D, 500000.0, 32.0, 1.0, 4.0, 8192.0, 2048)
    c, s = mv.csm_rope_tables(D, 500000.0, 32.0, 1.0, 4.0, 8192.0, 2048)
    assert np.array_equal(c.view(np.uint32), lit_c.view(np.uint32)) and np.array_equal(s.view(np.uint32), lit_s.view(np.uint32))
    ec, es = np.zeros((2048, D // 2), np.float32), np.zeros((2048, D // 2), np.float32)
    st = mas._lib.lib().mis_debug_marvis_rope_tables(D, 500000.0, 32.0, 1.0, 4.0, 8192.0, 2048, ec.ctypes.data, es.ctypes.data)
    assert st == 0
    assert np.array_equal(ec.view(np.uint32), lit_c.view(np.uint32)) and np.array_equal(es.view(np.uint32), lit_s.view(np.uint32))
    # the three regimes of applyScaling are all present at theta = 500000: unscaled, blended, divided by 32
    th = np.arctan2(lit_s[1].astype(np.float64), lit_c[1].astype(np.float64))
    plain = 500000.0 ** (-np.arange(0, D, 2) / D)
    assert np.isclose(th[0], plain[0], rtol=1e-6) and np.isclose(th[-1], plain[-1] / 32.0, rtol=1e-5)
    assert np.any((th < plain * 0.999) & (th > plain / 32.0 * 1.001))


def _rot_interleaved(x, c, s):
    y = np.empty_like(x)
    y[..., 0::2] = x[..., 0::2] * c - x[..., 1::2] * s
    y[..., 1::2] = x[..., 1::2] * c + x[..., 0::2] * s
    return y


def _rot_half(x, c, s):
    h = x.shape[-1] // 2
    return np.concatenate([x[..., :h] * c - x[..., h:] * s, x[..., h:] * c + x[..., :h] * s], -1)


@pytest.mark.parametrize("D", [64, 128])
def test_deinterleave_turns_pair_rotation_into_half_rotation_exactly(D):
    rng = np.random.default_rng(D)
    H = 3
    q = rng.standard_normal((5, H * D)).astype(np.float32)
    c, s = mv.csm_rope_tables(D, 500000.0, n_pos=5)
    perm = mv.deinterleave_rows(H * D, D)
    assert sorted(perm.tolist()) == list(range(H * D))
    a = _rot_interleaved(q.reshape(5, H, D), c[:, None, :], s[:, None, :]).reshape(5, H * D)
    b = _rot_half(q[:, perm].reshape(5, H, D), c[:, None, :], s[:, None, :]).reshape(5, H * D)
    assert np.array_equal(a[:, perm], b)                                 # exactly: the same products and sums per element
    # ... and as a row permutation of the projection: (W[perm] x) == (W x)[perm]
    Wq = rng.standard_normal((H * D, 32)).astype(np.float32)
    x = rng.standard_normal(32).astype(np.float32)
    assert np.array_equal(Wq[perm] @ x, (Wq @ x)[perm])


@pytest.mark.parametrize("bits", [4, 8])
def test_row_permutation_commutes_with_dequantisation(bits):
    rng = np.random.default_rng(bits)
    D, H, K = 64, 2, 128
    w = rng.standard_normal((H * D, K)).astype(np.float32)
    wq, sc, bi = mlxquant.quantize(w, 64, bits)
    perm = mv.deinterleave_rows(H * D, D)
    a = mlxquant.dequantize(wq, sc, bi, 64, bits)[perm]
    b = mlxquant.dequantize(np.asarray(wq)[perm], np.asarray(sc)[perm], np.asarray(bi)[perm], 64, bits)
    assert np.array_equal(a, b)


def test_float32_block_matches_transformers_after_deinterleave():
    """CSMLlamaRef in pure float32 == transformers.LlamaModel (inputs_embeds, llama3 rope_scaling) whose q/k rows were de-interleaved:
    pins the permutation and the scaling formula on an independent implementation.  Tolerance: tests/test_oracle_llama.py's."""
    tr = pytest.importorskip("transformers")
    cfg = mr._lm(256, 2, 512, 4, 2, 64, 97)
    W = ollama.make_synthetic_weights(cfg, dtype=torch.float32)
    hf_cfg = tr.LlamaConfig(hidden_size=256, num_hidden_layers=2, intermediate_size=512, num_attention_heads=4, num_key_value_heads=2,
                            head_dim=64, rms_norm_eps=cfg.rms_norm_eps, vocab_size=97, rope_theta=cfg.rope_theta,
                            rope_scaling=dict(cfg.rope_scaling), max_position_embeddings=2048, attention_bias=False, mlp_bias=False,
                            attn_implementation="eager")
    hf = tr.LlamaModel(hf_cfg).to(torch.float32).eval()
    sd = {}
    for k, v in W.items():
        if k == "lm_head.weight":
            continue
        v = v.to(torch.float32)
        if k.endswith("q_proj.weight") or k.endswith("k_proj.weight"):
            v = v[torch.from_numpy(mv.deinterleave_rows(v.shape[0], 64))]
        sd[k[len("model."):]] = v
    missing, unexpected = hf.load_state_dict(sd, strict=False)
    assert not [k for k in missing if "rotary" not in k] and not unexpected
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((1, 9, 256)).astype(np.float32))
    with torch.no_grad():
        ref = hf(inputs_embeds=x).last_hidden_state[0].numpy()
    o = mr.CSMLlamaRef(cfg, W, round=None)
    o.reset(1)
    with torch.no_grad():
        o.forward_embeds(0, x[0, :5], head=torch.zeros(1, 256))
        a = o.last_hidden.numpy()
        o.forward_embeds(0, x[0, 5:], head=torch.zeros(1, 256))
        b = o.last_hidden.numpy()
    np.testing.assert_allclose(np.concatenate([a, b]), ref, rtol=2e-4, atol=2e-4)


def test_token_frames_masks_and_limits():
    K = 4
    t, m = mv.tokenize_text_segment([7, 8, 9], K)
    assert t.tolist() == [[0, 0, 0, 0, 7], [0, 0, 0, 0, 8], [0, 0, 0, 0, 9]] and m.tolist() == [[0, 0, 0, 0, 1]] * 3
    codes = np.arange(8).reshape(K, 2)
    a, am = mv.tokenize_audio(codes, K, add_eos=True)
    assert a.tolist() == [[0, 2, 4, 6, 0], [1, 3, 5, 7, 0], [0, 0, 0, 0, 0]] and am.tolist() == [[1, 1, 1, 1, 0]] * 3
    s, sm = mv.tokenize_segment([7, 8], codes, K, add_eos=False)
    assert s.shape == (4, 5) and s[:2, K].tolist() == [7, 8] and sm[:2].sum() == 2 and sm[2:, :K].all() and not sm[2:, K].any()
    with pytest.raises(mas.AudioGenerationError):
        mv.tokenize_audio(np.zeros((K + 1, 2), np.int32), K)
    assert mv.MAX_SEQ_LEN - mv.MAX_AUDIO_FRAMES == 1298 and mv.MAX_AUDIO_FRAMES == 750
    assert [int(q) for q in mv.QualityLevel] == [8, 16, 24, 32]


def test_text_pieces():
    assert mv.text_pieces("  a b\n\nc\nd  \n") == ["a b", "c", "d"]
    assert mv.text_pieces("one") == ["one"]
    assert mv.text_pieces("a\nb", None) == ["a\nb"]


def test_both_config_shapes():
    a = mv.CSMModelArgs.from_json(dict(model_type="sesame/csm", backbone_flavor="llama-1B", decoder_flavor="llama-100M", text_vocab_size=128256,
                                       audio_vocab_size=2051, audio_num_codebooks=32))
    assert (a.backbone.hidden_size, a.backbone.num_hidden_layers, a.backbone.num_attention_heads, a.backbone.num_key_value_heads,
            a.backbone.resolved_head_dim, a.backbone.intermediate_size) == (2048, 16, 32, 8, 64, 8192)
    assert (a.decoder.hidden_size, a.decoder.num_hidden_layers, a.decoder.num_attention_heads, a.decoder.num_key_value_heads,
            a.decoder.resolved_head_dim, a.decoder.intermediate_size) == (1024, 4, 8, 2, 128, 8192)
    assert a.backbone.rope_theta == 500000.0 and a.backbone.rope_numbers() == (32.0, 1.0, 4.0, 8192.0)
    rs = dict(factor=16.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=4096, rope_type="llama3")
    b = mv.CSMModelArgs.from_json(dict(
        model_type="csm", text_vocab_size=500, audio_vocab_size=83, audio_num_codebooks=12, hidden_size=256, num_hidden_layers=3,
        intermediate_size=512, num_attention_heads=4, num_key_value_heads=2, head_dim=64, rms_norm_eps=1e-5, rope_theta=500000, rope_scaling=rs,
        depth_decoder_config=dict(hidden_size=128, num_hidden_layers=2, intermediate_size=256, num_attention_heads=1, num_key_value_heads=1,
                                  head_dim=128, rms_norm_eps=1e-5, rope_theta=500000, rope_scaling=rs, vocab_size=83, num_codebooks=12),
        quantization=dict(group_size=64, bits=8)))
    assert b.backbone.num_hidden_layers == 3 and b.decoder.hidden_size == 128 and b.decoder.resolved_head_dim == 128
    assert b.backbone.rope_numbers() == (16.0, 1.0, 4.0, 4096.0) and b.quantization == dict(group_size=64, bits=8)
    cc = b.to_c()
    assert cc.backbone.rope_ops_in_dtype == 1 and cc.audio_num_codebooks == 12 and cc.decoder.head_dim == 128
    assert C.sizeof(mas._lib.MarvisConfigC) == 2 * C.sizeof(mas._lib.LmConfigC) + 12 and C.sizeof(mas._lib.MarvisParamsC) == 32


def test_sanitize_raw_key_spellings():
    raw = {"backbone.layers.0.attn.q_proj.weight": 1, "backbone.layers.0.attn.output_proj.weight": 2, "backbone.layers.1.mlp.w1.weight": 3,
           "decoder.layers.0.mlp.w2.weight": 4, "decoder.layers.0.mlp.w3.weight": 5, "backbone.layers.0.sa_norm.scale": 6,
           "decoder.layers.1.mlp_norm.scale": 7, "backbone.norm.scale": 8, "decoder.norm.scale": 9, "text_embeddings.weight": 10,
           "audio_head": 11, "model.projection.weight": 12}
    out = mv.marvis_sanitize(raw)
    assert out == {"model.backbone.layers.0.self_attn.q_proj.weight": 1, "model.backbone.layers.0.self_attn.o_proj.weight": 2,
                   "model.backbone.layers.1.mlp.gate_proj.weight": 3, "model.decoder.layers.0.mlp.down_proj.weight": 4,
                   "model.decoder.layers.0.mlp.up_proj.weight": 5, "model.backbone.layers.0.input_layernorm.weight": 6,
                   "model.decoder.layers.1.post_attention_layernorm.weight": 7, "model.backbone.norm.weight": 8, "model.decoder.norm.weight": 9,
                   "model.text_embeddings.weight": 10, "model.audio_head": 11, "model.projection.weight": 12}
    W = mr.make_weights(mr.TINY)
    assert sorted(mv.marvis_sanitize({mr.raw_key(k): 0 for k in W})) == sorted(W)          # the helper's raw spelling round-trips


def test_quantised_checkpoint_plan():
    dt = {}
    for base in ("model.backbone.layers.0.self_attn.q_proj", "model.text_embeddings", "model.audio_embeddings", "model.projection",
                 "model.codebook0_head"):
        dt.update({base + ".weight": "U32", base + ".scales": "BF16", base + ".biases": "BF16"})
    dt.update({"model.audio_head": "BF16", "model.backbone.norm.weight": "BF16", "model.backbone.layers.0.self_attn.rotary_emb.inv_freq": "F32"})
    plan = mv.marvis_checkpoint_plan(dt, dict(group_size=64, bits=8))
    q = {e[4]: e for e in plan if e[0] == "quantized"}
    assert set(q) == {"model.backbone.layers.0.self_attn.q_proj.weight", "model.text_embeddings.weight", "model.audio_embeddings.weight",
                      "model.projection.weight", "model.codebook0_head.weight"}
    assert all(e[5:] == (64, 8) for e in q.values())
    assert [e for e in plan if e[0] == "dense"] == [("dense", "model.audio_head", "model.audio_head"),
                                                    ("dense", "model.backbone.norm.weight", "model.backbone.norm.weight")]
    with pytest.raises(mas.AudioGenerationError):
        mv.marvis_checkpoint_plan(dt, None)                              # .scales without a quantization entry
    with pytest.raises(mas.AudioGenerationError):
        mv.marvis_checkpoint_plan({"model.projection.weight": "U32"}, dict(group_size=64, bits=4))
    bad = dict(dt); del bad["model.projection.biases"]
    with pytest.raises(mas.AudioGenerationError):
        mv.marvis_checkpoint_plan(bad, dict(group_size=64, bits=8))
    # unquantised: the raw spellings go through the key map
    assert mv.marvis_checkpoint_plan({"backbone.layers.0.attn.output_proj.weight": "BF16"}, None) == [
        ("dense", "backbone.layers.0.attn.output_proj.weight", "model.backbone.layers.0.self_attn.o_proj.weight")]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_new_kernels_register_bounds():
    """csrc/marvis.hip cross-compiled for gfx950: no kernel uses scratch; the in-register sampler (16 logits, their masses and keys per
    thread) stays under 128 VGPRs so that two of its 256-thread blocks fit a SIMD set.  Recorded: the VGPR count of every kernel."""
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S",
                            os.path.join(ROOT, "mlx-audio-swift_amd", "csrc", "marvis.hip"), "-o", os.path.join(td, "k.s"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    use, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = use.setdefault(m.group(1), {})
        elif cur is not None:
            m = re.search(r"remark:\s+VGPRs: (\d+)", line)
            if m:
                cur["vgprs"] = int(m.group(1))
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
            if m:
                cur["scratch"] = int(m.group(1))
    print("MARVIS KERNELS", {k: v for k, v in use.items()})
    for name in ("k_mv_sample", "k_mv_frame_end", "k_mv_prompt_rows", "k_mv_prompt_feed", "k_mv_gather_pack", "k_mv_transpose"):
        hit = {k: v for k, v in use.items() if name in k}
        assert hit, name
        for k, v in hit.items():
            assert v["scratch"] == 0, (k, v)
    assert max(v["vgprs"] for k, v in use.items() if "k_mv_sample" in k) <= 128
