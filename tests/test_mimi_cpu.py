"""CPU tier for the Mimi codec: tests/mimi_ref.py pinned on HF transformers' MimiModel.decode, the restated per-frame stream against
the restated whole decode (equal while the attention window holds every key, departing where the window formula says), the
checkpoint sanitiser mimi_sanitize against a table of raw Kyutai names and shapes, the package's synthetic weights against the
oracle's, and the register / scratch bounds of the compiled kernels of csrc/mimi.hip."""
import dataclasses
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import mimi_ref as mr
import mlx_audio_swift_amd as mas
from mlx_audio_swift_amd.synthetic import mimi_synthetic_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _hf_model(c, W):
    from transformers import MimiConfig, MimiModel
    hd = c.dimension // c.num_heads
    hc = MimiConfig(sampling_rate=c.sample_rate, frame_rate=c.frame_rate, audio_channels=1, hidden_size=c.dimension, num_filters=c.n_filters,
                    num_residual_layers=c.n_residual_layers, upsampling_ratios=list(c.ratios), kernel_size=c.kernel_size,
                    last_kernel_size=c.last_kernel_size, residual_kernel_size=c.residual_kernel_size, dilation_growth_rate=c.dilation_base,
                    use_causal_conv=True, pad_mode="constant", compress=c.compress, codebook_size=c.bins, codebook_dim=c.quantizer_dim,
                    num_quantizers=c.num_quantizers, use_conv_shortcut=False, vector_quantization_hidden_dimension=c.quantizer_dim,
                    num_semantic_quantizers=1, num_hidden_layers=c.num_layers, intermediate_size=c.dim_feedforward,
                    num_attention_heads=c.num_heads, num_key_value_heads=c.num_heads, head_dim=hd, hidden_act="gelu", norm_eps=1e-5,
                    rope_theta=c.max_period, sliding_window=c.context, layer_scale_initial_scale=0.01, attention_bias=False,
                    upsample_groups=c.dimension)
    hf = MimiModel(hc).eval()
    sd = hf.state_dict()
    t = lambda k: torch.from_numpy(np.asarray(W[k]))
    conv = lambda k: t(k).permute(0, 2, 1).contiguous()                       # [out, k, in] -> [out, in, k]

    def put(hf_name, name, tr=False):
        sd[hf_name + ".conv.weight"] = t(name + ".weight").permute(2, 0, 1).contiguous() if tr else conv(name + ".weight")
        sd[hf_name + ".conv.bias"] = t(name + ".bias")
    # HF flattens the SEANet decoder: conv, then per ratio [ELU, transposed conv, resnet block], ELU, conv
    put("decoder.layers.0", "decoder.init_conv1d.conv.conv")
    idx = 1
    for li in range(len(c.ratios)):
        idx += 1
        put(f"decoder.layers.{idx}", f"decoder.layers.{li}.upsample.convtr.convtr", tr=True)
        idx += 1
        put(f"decoder.layers.{idx}.block.1", f"decoder.layers.{li}.residuals.0.block.0.conv.conv")
        put(f"decoder.layers.{idx}.block.3", f"decoder.layers.{li}.residuals.0.block.1.conv.conv")
        idx += 1
    put(f"decoder.layers.{idx + 1}", "decoder.final_conv1d.conv.conv")
    sd["upsample.conv.weight"] = t("upsample.convtr.convtr.convtr.weight").permute(0, 2, 1).contiguous()
    D, H = c.dimension, c.num_heads
    perm = torch.cat([torch.arange(0, hd, 2), torch.arange(1, hd, 2)])
    rows = torch.cat([h * hd + perm for h in range(H)])
    for li in range(c.num_layers):
        p, q = f"decoder_transformer.transformer.layers.{li}", f"decoder_transformer.layers.{li}"
        w = t(p + ".self_attn.in_proj.weight")
        sd[q + ".self_attn.q_proj.weight"] = w[:D][rows]
        sd[q + ".self_attn.k_proj.weight"] = w[D:2 * D][rows]
        sd[q + ".self_attn.v_proj.weight"] = w[2 * D:]
        sd[q + ".self_attn.o_proj.weight"] = t(p + ".self_attn.out_proj.weight")
        sd[q + ".mlp.fc1.weight"] = t(p + ".gating.linear1.weight")
        sd[q + ".mlp.fc2.weight"] = t(p + ".gating.linear2.weight")
        sd[q + ".input_layernorm.weight"], sd[q + ".input_layernorm.bias"] = t(p + ".norm1.weight"), t(p + ".norm1.bias")
        sd[q + ".post_attention_layernorm.weight"], sd[q + ".post_attention_layernorm.bias"] = t(p + ".norm2.weight"), t(p + ".norm2.bias")
        sd[q + ".self_attn_layer_scale.scale"], sd[q + ".mlp_layer_scale.scale"] = t(p + ".layer_scale_1.scale"), t(p + ".layer_scale_2.scale")
    for hf_grp, grp, nq in (("semantic", "rvq_first", 1), ("acoustic", "rvq_rest", c.num_quantizers - 1)):
        hp, op = f"quantizer.{hf_grp}_residual_vector_quantizer", f"quantizer.{grp}"
        sd[hp + ".output_proj.weight"] = conv(op + ".output_proj.weight")
        for i in range(nq):
            sd[f"{hp}.layers.{i}.codebook.embed_sum"] = t(f"{op}.vq.layers.{i}.codebook.embedding_sum")
            sd[f"{hp}.layers.{i}.codebook.cluster_usage"] = t(f"{op}.vq.layers.{i}.codebook.cluster_usage")
            sd[f"{hp}.layers.{i}.codebook.initialized"] = torch.ones(1)
    missing = [k for k in hf.state_dict() if k.startswith(("decoder", "upsample", "quantizer")) and k not in sd]
    assert not missing, missing[:5]
    hf.load_state_dict(sd)
    return hf


@pytest.mark.parametrize("nq,T", [(8, 23), (3, 125)])
def test_decode_matches_hf_mimi(nq, T):
    pytest.importorskip("transformers")
    c = mr.TINY
    W = mr.make_synthetic_weights(c)
    hf = _hf_model(c, W)
    codes = mr.synthetic_codes(c, 2, nq, T, seed=nq)
    ref = mr.MimiDecoderRef(c, W).decode(codes)
    with torch.no_grad():
        got = hf.decode(torch.from_numpy(codes.astype(np.int64))).audio_values.numpy()
    assert got.shape == ref.shape == (2, 1, T * c.samples_per_frame)
    np.testing.assert_allclose(ref, got, rtol=1e-4, atol=2e-5 * np.abs(got).max())


def test_stream_equals_whole_decode_until_the_window_trims():
    c = dataclasses.replace(mr.TINY, num_layers=1)
    W = mr.make_synthetic_weights(c)
    o = mr.MimiDecoderRef(c, W)
    f0 = mr.first_divergent_frame(c)
    assert f0 == 126                                                # s = 2, context 250: frame 126 is the first to lose key 0
    codes = mr.synthetic_codes(c, 1, 4, f0 + 4, seed=2)
    whole, stream = o.decode(codes), o.stream(codes)
    spf = c.samples_per_frame
    per_frame = np.abs(whole - stream).reshape(-1, spf).max(axis=1)
    scale = np.abs(whole).max()
    assert per_frame[:f0].max() < 2e-6 * scale
    assert per_frame[f0] > 1e-4 * scale
    # a short context moves the departure accordingly
    c6 = dataclasses.replace(c, context=6)
    o6 = mr.MimiDecoderRef(c6, W)
    d = np.abs(o6.decode(codes[:, :, :8]) - o6.stream(codes[:, :, :8])).reshape(-1, spf).max(axis=1)
    assert mr.first_divergent_frame(c6) == 4 and d[:4].max() < 2e-6 * scale and d[4:].min() > 1e-4 * scale


# raw Kyutai key, raw shape -> post-sanitize key, MLX shape (mimi_202407 widths)
SANITIZE_TABLE = [
    ("encoder.model.0.conv.conv.weight", (64, 1, 7), "encoder.init_conv1d.conv.conv.weight", (64, 7, 1)),
    ("encoder.model.0.conv.conv.bias", (64,), "encoder.init_conv1d.conv.conv.bias", (64,)),
    ("encoder.model.1.block.1.conv.conv.weight", (32, 64, 3), "encoder.layers.0.residuals.0.block.0.conv.conv.weight", (32, 3, 64)),
    ("encoder.model.1.block.3.conv.conv.weight", (64, 32, 1), "encoder.layers.0.residuals.0.block.1.conv.conv.weight", (64, 1, 32)),
    ("encoder.model.3.conv.conv.weight", (128, 64, 8), "encoder.layers.0.downsample.conv.conv.weight", (128, 8, 64)),
    ("encoder.model.10.block.3.conv.conv.bias", (512,), "encoder.layers.3.residuals.0.block.1.conv.conv.bias", (512,)),
    ("encoder.model.12.conv.conv.weight", (1024, 512, 16), "encoder.layers.3.downsample.conv.conv.weight", (1024, 16, 512)),
    ("encoder.model.14.conv.conv.weight", (512, 1024, 3), "encoder.final_conv1d.conv.conv.weight", (512, 3, 1024)),
    ("decoder.model.0.conv.conv.weight", (1024, 512, 7), "decoder.init_conv1d.conv.conv.weight", (1024, 7, 512)),
    ("decoder.model.2.convtr.convtr.weight", (1024, 512, 16), "decoder.layers.0.upsample.convtr.convtr.weight", (512, 16, 1024)),
    ("decoder.model.2.convtr.convtr.bias", (512,), "decoder.layers.0.upsample.convtr.convtr.bias", (512,)),
    ("decoder.model.3.block.1.conv.conv.weight", (256, 512, 3), "decoder.layers.0.residuals.0.block.0.conv.conv.weight", (256, 3, 512)),
    ("decoder.model.3.block.3.conv.conv.weight", (512, 256, 1), "decoder.layers.0.residuals.0.block.1.conv.conv.weight", (512, 1, 256)),
    ("decoder.model.11.convtr.convtr.weight", (128, 64, 8), "decoder.layers.3.upsample.convtr.convtr.weight", (64, 8, 128)),
    ("decoder.model.12.block.1.conv.conv.bias", (32,), "decoder.layers.3.residuals.0.block.0.conv.conv.bias", (32,)),
    ("decoder.model.14.conv.conv.weight", (1, 64, 3), "decoder.final_conv1d.conv.conv.weight", (1, 3, 64)),
    ("upsample.convtr.convtr.convtr.weight", (512, 1, 4), "upsample.convtr.convtr.convtr.weight", (512, 4, 1)),
    ("downsample.conv.conv.conv.weight", (512, 512, 4), "downsample.conv.conv.conv.weight", (512, 4, 512)),
    ("decoder_transformer.transformer.layers.0.self_attn.in_proj_weight", (1536, 512),
     "decoder_transformer.transformer.layers.0.self_attn.in_proj.weight", (1536, 512)),
    ("decoder_transformer.transformer.layers.7.self_attn.out_proj.weight", (512, 512),
     "decoder_transformer.transformer.layers.7.self_attn.out_proj.weight", (512, 512)),
    ("encoder_transformer.transformer.layers.3.linear1.weight", (2048, 512),
     "encoder_transformer.transformer.layers.3.gating.linear1.weight", (2048, 512)),
    ("decoder_transformer.transformer.layers.2.linear2.weight", (512, 2048),
     "decoder_transformer.transformer.layers.2.gating.linear2.weight", (512, 2048)),
    ("decoder_transformer.transformer.layers.2.norm1.bias", (512,), "decoder_transformer.transformer.layers.2.norm1.bias", (512,)),
    ("decoder_transformer.transformer.layers.2.layer_scale_2.scale", (512,),
     "decoder_transformer.transformer.layers.2.layer_scale_2.scale", (512,)),
    ("quantizer.rvq_first.output_proj.weight", (512, 256, 1), "quantizer.rvq_first.output_proj.weight", (512, 1, 256)),
    ("quantizer.rvq_rest.input_proj.weight", (256, 512, 1), "quantizer.rvq_rest.input_proj.weight", (256, 1, 512)),
    ("quantizer.rvq_first.vq.layers.0._codebook.embedding_sum", (2048, 256),
     "quantizer.rvq_first.vq.layers.0.codebook.embedding_sum", (2048, 256)),
    ("quantizer.rvq_rest.vq.layers.30._codebook.cluster_usage", (2048,), "quantizer.rvq_rest.vq.layers.30.codebook.cluster_usage", (2048,)),
]


@pytest.mark.parametrize("raw,raw_shape,key,shape", SANITIZE_TABLE)
def test_mimi_sanitize_table(raw, raw_shape, key, shape):
    a = np.arange(int(np.prod(raw_shape)), dtype=np.float32).reshape(raw_shape)
    k, v = mas.mimi_sanitize(raw, a)
    assert (k, tuple(v.shape)) == (key, shape)
    kt, vt = mas.mimi_sanitize(raw, torch.from_numpy(a))
    assert kt == key and np.array_equal(vt.numpy(), v)


def test_mimi_sanitize_layouts():
    w = np.arange(4 * 3 * 5, dtype=np.float32).reshape(4, 3, 5)                       # PyTorch convtr [in, out, k]
    _, v = mas.mimi_sanitize("decoder.model.5.convtr.convtr.weight", w)
    assert v.shape == (3, 5, 4) and v[1, 2, 3] == w[3, 1, 2]                          # [out, k, in]
    dw = np.arange(6 * 4, dtype=np.float32).reshape(6, 1, 4)
    _, v = mas.mimi_sanitize("upsample.convtr.convtr.convtr.weight", dw)
    assert v.shape == (6, 4, 1) and v[2, 3, 0] == dw[2, 0, 3]
    cw = np.arange(4 * 3 * 5, dtype=np.float32).reshape(4, 3, 5)                      # conv [out, in, k]
    _, v = mas.mimi_sanitize("decoder.model.0.conv.conv.weight", cw)
    assert v.shape == (4, 5, 3) and v[1, 4, 2] == cw[1, 2, 4]


def test_package_synthetic_weights_are_the_oracle_weights():
    c = mr.TINY
    hc = mas.MimiConfig(num_codebooks=c.num_quantizers, sample_rate=c.sample_rate, frame_rate=c.frame_rate, dimension=c.dimension,
                        n_filters=c.n_filters, ratios=list(c.ratios), num_layers=c.num_layers, num_heads=c.num_heads,
                        dim_feedforward=c.dim_feedforward, bins=c.bins, quantizer_dim=c.quantizer_dim)
    A, B = mimi_synthetic_weights(hc, 77), mr.make_synthetic_weights(c, 77)
    assert sorted(A) == sorted(B) and all(np.array_equal(A[k], B[k]) for k in A)
    assert hc.samples_per_frame == c.samples_per_frame and mas.MimiConfig().samples_per_frame == 1920


@pytest.fixture(scope="module")
def usage():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    # mimi.hip's own kernels and the ones it shares with the Qwen3-TTS decoder (codec_stream.hip: gather-sum, carry, final conv)
    stderr = ""
    with tempfile.TemporaryDirectory() as td:
        for src in ("mimi.hip", "codec_stream.hip"):
            r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S",
                                os.path.join(ROOT, "mlx-audio-swift_amd", "csrc", src), "-o", os.path.join(td, "k.s"),
                                "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]
            stderr += r.stderr
    use, cur = {}, None
    for line in stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = use.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        m = re.search(r"remark:\s+VGPRs: (\d+)", line)
        if m:
            cur["vgprs"] = int(m.group(1))
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m:
            cur["scratch"] = int(m.group(1))
    return {k: v for k, v in use.items() if "k_mimi_" in k or "k_codec_" in k}


def test_mimi_kernels_do_not_spill(usage):
    want = {"k_codec_embed", "k_mimi_upsample", "k_mimi_elu", "k_codec_hist", "k_mimi_kv_ring", "k_codec_final"}
    assert {re.search(r"k_(mimi|codec)_[a-z_]+?(?=P|I)", k).group(0) for k in usage} == want, sorted(usage)
    assert sum("k_codec_final" in k for k in usage) == 2, sorted(usage)          # the ELU and the SnakeBeta instantiation
    for k, v in usage.items():
        assert v["scratch"] == 0, (k, v)
        assert v["vgprs"] <= 64, (k, v)
