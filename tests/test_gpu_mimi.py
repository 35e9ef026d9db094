"""-m gpu: the Mimi codec (csrc/mimi.hip) against tests/mimi_ref.py (decoder, per-frame stream) and oracle/mimi_encoder.py (encode):
whole decode at reduced and mimi_202407 widths, stage taps, batch independence, the stream (bitwise equal to whole decode while the
attention window holds every key, the reference's window after that), stream lifecycle and argument errors, encode, and the raw
Kyutai checkpoint loader."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
import mimi_ref as mr
from oracle import mimi_encoder as om

pytestmark = pytest.mark.gpu

BOUND = 1e-4          # relative RMS error bound of the decoder (observed: profiles/mimi/parity_observed.jsonl)


def _host_cfg(c: mr.MimiRefConfig) -> mas.MimiConfig:
    return mas.MimiConfig(num_codebooks=c.num_quantizers, sample_rate=c.sample_rate, frame_rate=c.frame_rate, dimension=c.dimension,
                          n_filters=c.n_filters, n_residual_layers=c.n_residual_layers, ratios=list(c.ratios), kernel_size=c.kernel_size,
                          residual_kernel_size=c.residual_kernel_size, last_kernel_size=c.last_kernel_size, dilation_base=c.dilation_base,
                          compress=c.compress, num_layers=c.num_layers, num_heads=c.num_heads, dim_feedforward=c.dim_feedforward,
                          context=c.context, max_period=c.max_period, bins=c.bins, quantizer_dim=c.quantizer_dim)


_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_handles():
    """The handles shared by this module's tests are destroyed when it ends: a live handle keeps a HIP stream and gigabytes of work
    buffers, which later modules must not inherit."""
    yield
    for _, dev, _ in _CACHE.values():
        dev.close()
    _CACHE.clear()


def _pair(c: mr.MimiRefConfig):
    key = repr(c)
    if key not in _CACHE:
        W = mr.make_synthetic_weights(c)
        _CACHE[key] = (mr.MimiDecoderRef(c, W), mas.Mimi.from_weights(_host_cfg(c), W), W)
    return _CACHE[key]


def _rel(got, ref):
    return float(np.sqrt(np.mean((got - ref) ** 2)) / max(np.sqrt(np.mean(ref ** 2)), 1e-12))


def _record(**kw):
    path = os.environ.get("MIS_MIMI_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(kw) + "\n")


@pytest.mark.parametrize("B,T,nq", [(b, t, q) for b in (1, 3, 8) for t in (1, 7, 40) for q in (2, 8)])
def test_decode_reduced_matches_oracle(B, T, nq):
    orc, dev, _ = _pair(mr.TINY)
    codes = mr.synthetic_codes(mr.TINY, B, nq, T, seed=B * 100 + T)
    got, ref = dev.decode(codes), orc.decode(codes)
    assert got.shape == ref.shape == (B, 1, T * mr.TINY.samples_per_frame)
    e = _rel(got, ref)
    _record(test="decode_tiny", B=B, T=T, nq=nq, rel_rms=e)
    assert e < BOUND, e


@pytest.mark.parametrize("B,T,nq", [(1, 1, 32), (3, 7, 8), (8, 40, 32), (1, 40, 8), (3, 1, 32)])
def test_decode_mimi_202407_matches_oracle(B, T, nq):
    orc, dev, _ = _pair(mr.MIMI)
    codes = mr.synthetic_codes(mr.MIMI, B, nq, T, seed=B * 100 + T + nq)
    got, ref = dev.decode(codes), orc.decode(codes)
    assert got.shape == ref.shape == (B, 1, T * 1920)
    e = _rel(got, ref)
    _record(test="decode_mimi_202407", B=B, T=T, nq=nq, rel_rms=e)
    assert e < BOUND, e


def test_stage_taps_match_oracle():
    orc, dev, _ = _pair(mr.MIMI)
    codes = mr.synthetic_codes(mr.MIMI, 2, 16, 5, seed=9)
    stages = ["rvq", "upsample", "transformer", "init"] + [f"layer{i}" for i in range(4)]
    for i, name in enumerate(stages):
        got, ref = dev.debug_tap(codes, i), orc.decode(codes, stop=name)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        e = _rel(got, ref)
        _record(test="tap", stage=name, rel_rms=e)
        assert e < BOUND, (name, e)
    assert np.array_equal(dev.debug_tap(codes, 8), dev.decode(codes))


def test_batch_rows_are_independent():
    _, dev, _ = _pair(mr.MIMI)
    codes = mr.synthetic_codes(mr.MIMI, 5, 32, 6, seed=3)
    full = dev.decode(codes)
    for b in (0, 3):
        assert np.array_equal(dev.decode(codes[b:b + 1])[0], full[b])


@pytest.mark.parametrize("c", [mr.TINY, mr.MIMI], ids=["tiny", "mimi_202407"])
def test_stream_is_bitwise_whole_decode_through_frame_125(c):
    _, dev, _ = _pair(c)
    T = mr.first_divergent_frame(c)                                  # 126 frames: every step still sees every key
    codes = mr.synthetic_codes(c, 2, 8, T, seed=11)
    whole = dev.decode(codes)
    sd = mas.MimiStreamingDecoder(dev, batch=2)
    single = np.concatenate([sd.decode_frames(codes[:, :, f:f + 1]) for f in range(T)], axis=2)
    assert np.array_equal(single, whole)
    sd.reset()
    cuts = [0, 3, 4, 41, 90, 125, T]                                 # multi-frame steps, one of them above the internal sub-step
    multi = np.concatenate([sd.decode_frames(codes[:, :, a:b]) for a, b in zip(cuts[:-1], cuts[1:])], axis=2)
    assert np.array_equal(multi, whole)


def test_stream_window_matches_oracle_and_departs_after_frame_125():
    c = mr.TINY
    orc, dev, _ = _pair(c)
    T = 140
    codes = mr.synthetic_codes(c, 2, 8, T, seed=13)
    sd = mas.MimiStreamingDecoder(dev, batch=2)
    got = np.concatenate([sd.decode_frames(codes[:, :, a:a + 7]) for a in range(0, T, 7)], axis=2)
    ref = orc.stream(codes)
    e = _rel(got, ref)
    _record(test="stream_window_tiny", T=T, rel_rms=e)
    assert e < BOUND, e
    whole = dev.decode(codes)
    spf, f0 = c.samples_per_frame, mr.first_divergent_frame(c)
    assert np.array_equal(got[..., : f0 * spf], whole[..., : f0 * spf])
    assert not np.allclose(got[..., f0 * spf:(f0 + 1) * spf], whole[..., f0 * spf:(f0 + 1) * spf], rtol=0, atol=1e-5)


def test_stream_lifecycle_and_bad_n_q():
    c = mr.TINY
    _, dev, _ = _pair(c)
    lib = mas._lib.lib()
    codes = mr.synthetic_codes(c, 1, 8, 2)
    out = np.empty(2 * c.samples_per_frame, np.float32)
    fresh = mas.Mimi.from_weights(_host_cfg(c), mr.make_synthetic_weights(c))
    assert lib.mis_mimi_decode_stream_step(fresh._h, codes.ctypes.data, 8, 2, out.ctypes.data) == 1       # no begin
    assert lib.mis_mimi_decode_stream_end(fresh._h) == 1
    assert lib.mis_mimi_decode_stream_begin(fresh._h, 1) == 0
    assert lib.mis_mimi_decode_stream_step(fresh._h, codes.ctypes.data, 8, 2, out.ctypes.data) == 0
    first = out.copy()
    assert lib.mis_mimi_decode_stream_begin(fresh._h, 1) == 0                                           # a second begin resets
    assert lib.mis_mimi_decode_stream_step(fresh._h, codes.ctypes.data, 8, 2, out.ctypes.data) == 0
    assert np.array_equal(out, first)
    assert lib.mis_mimi_decode_stream_end(fresh._h) == 0
    assert lib.mis_mimi_decode_stream_step(fresh._h, codes.ctypes.data, 8, 2, out.ctypes.data) == 1      # ended
    for nq in (0, 1, c.num_quantizers + 1):
        cd = mr.synthetic_codes(c, 1, max(nq, 1), 2)
        assert lib.mis_mimi_decode(dev._h, cd.ctypes.data, 1, nq, 2, out.ctypes.data) == 3
    with pytest.raises(mas.AudioGenerationError):
        dev.decode(mr.synthetic_codes(c, 1, 1, 2))
    fresh.close()


def _oracle_codes_with_margin(c, W, audio):
    """oracle/mimi_encoder codes and, per (row, quantizer, frame), whether every decision up to it had a margin above 1e-4."""
    o = om.MimiEncoderOracle(c.encoder_config(), W)
    codes, x = o.encode(audio, return_hidden=True)
    w = o.w
    ok = np.ones(codes.shape, bool)
    row = 0
    for grp, nq in (("rvq_first", 1), ("rvq_rest", c.num_quantizers - 1)):
        z = torch.nn.functional.conv1d(torch.from_numpy(x), w[f"quantizer.{grp}.input_proj.weight"].permute(0, 2, 1).contiguous())
        resid = z.transpose(1, 2).double()
        alive = np.ones((codes.shape[0], codes.shape[2]), bool)
        for i in range(nq):
            q = f"quantizer.{grp}.vq.layers.{i}.codebook"
            emb = (w[q + ".embedding_sum"] / torch.clamp(w[q + ".cluster_usage"], min=1e-5)[:, None]).double()
            dist = (emb * emb).sum(-1) / 2 - resid @ emb.T
            two = torch.topk(dist, 2, dim=-1, largest=False).values
            alive &= ((two[..., 1] - two[..., 0]) > 1e-4).numpy()
            ok[:, row] = alive
            resid = resid - emb[torch.argmin(dist, dim=-1)]
            row += 1
    return codes, ok


@pytest.mark.parametrize("c,n", [(mr.TINY, 6 * 2 * 23 + 5), (mr.MIMI, 1920 * 9 + 700)], ids=["tiny", "mimi_202407"])
def test_encode_matches_oracle(c, n):
    _, dev, W = _pair(c)
    audio = (0.3 * np.random.default_rng(2).standard_normal((2, 1, n))).astype(np.float32)
    ref, ok = _oracle_codes_with_margin(c, W, audio)
    got = dev.encode(audio)
    assert got.shape == ref.shape == (2, c.num_quantizers, dev.encode_num_frames(n))
    assert ok.mean() > 0.5
    assert np.array_equal(got[ok], ref[ok])
    assert np.array_equal(dev.encode(audio, n_q=3), got[:, :3])
    _record(test="encode", cfg="tiny" if c is mr.TINY else "mimi_202407", checked=float(ok.mean()),
            agree_all=float((got == ref).mean()))


def _unsanitize(k, v):
    """post-sanitize MLX key / layout -> raw Kyutai PyTorch key / layout (the inverse of Mimi.sanitize)."""
    import re
    k = re.sub(r"^encoder\.init_conv1d\.", "encoder.model.0.", k)
    k = re.sub(r"^encoder\.final_conv1d\.", "encoder.model.14.", k)
    k = re.sub(r"^encoder\.layers\.(\d)\.residuals\.0\.", lambda m: f"encoder.model.{1 + 3 * int(m.group(1))}.", k)
    k = re.sub(r"^encoder\.layers\.(\d)\.downsample\.", lambda m: f"encoder.model.{3 + 3 * int(m.group(1))}.", k)
    k = re.sub(r"^decoder\.init_conv1d\.", "decoder.model.0.", k)
    k = re.sub(r"^decoder\.final_conv1d\.", "decoder.model.14.", k)
    k = re.sub(r"^decoder\.layers\.(\d)\.upsample\.", lambda m: f"decoder.model.{2 + 3 * int(m.group(1))}.", k)
    k = re.sub(r"^decoder\.layers\.(\d)\.residuals\.0\.", lambda m: f"decoder.model.{3 + 3 * int(m.group(1))}.", k)
    k = k.replace(".block.1.", ".block.3.").replace(".block.0.", ".block.1.")
    k = k.replace(".in_proj.weight", ".in_proj_weight").replace(".gating.linear", ".linear").replace(".codebook.", "._codebook.")
    v = np.asarray(v)
    if k.endswith(".convtr.weight"):
        v = np.swapaxes(v, 1, 2) if v.shape[2] == 1 else np.transpose(v, (2, 0, 1))
    elif (k.endswith(".conv.weight") or k.endswith("_proj.weight")) and v.ndim == 3:
        v = np.swapaxes(v, 1, 2)
    return k, np.ascontiguousarray(v, np.float32)


def _write_safetensors(path, tensors):
    hdr, off, blobs = {}, 0, []
    for k, v in tensors.items():
        b = v.tobytes()
        hdr[k] = {"dtype": "F32", "shape": list(v.shape), "data_offsets": [off, off + len(b)]}
        off += len(b)
        blobs.append(b)
    h = json.dumps(hdr).encode()
    h += b" " * (-len(h) % 8)
    with open(path, "wb") as f:
        f.write(len(h).to_bytes(8, "little"))
        f.write(h)
        for b in blobs:
            f.write(b)


def test_raw_kyutai_checkpoint_loads_and_decodes_identically(tmp_path):
    c = mr.TINY
    _, dev, W = _pair(c)
    raw = dict(_unsanitize(k, v) for k, v in W.items())
    assert dict(mas.mimi_sanitize(k, torch.from_numpy(v)) for k, v in raw.items()).keys() == W.keys()
    _write_safetensors(os.path.join(tmp_path, "tokenizer-e351c8d8-checkpoint125.safetensors"), raw)
    loaded = mas.Mimi.from_pretrained(str(tmp_path), _host_cfg(c))
    codes = mr.synthetic_codes(c, 2, 8, 9, seed=21)
    assert np.array_equal(loaded.decode(codes), dev.decode(codes))
    audio = (0.3 * np.random.default_rng(4).standard_normal((1, 1, 200))).astype(np.float32)
    assert np.array_equal(loaded.encode(audio), dev.encode(audio))
    with pytest.raises(mas.AudioGenerationError):
        mas.Mimi.from_pretrained("kyutai/moshiko-pytorch-bf16")


def test_synthetic_matches_the_oracle_weights():
    c = dataclasses.replace(mr.TINY)
    orc, _, _ = _pair(c)
    m = mas.Mimi.synthetic(_host_cfg(c), seed=77)
    codes = mr.synthetic_codes(c, 1, 8, 4, seed=1)
    assert _rel(m.decode(codes), orc.decode(codes)) < BOUND
    assert m.codec_sample_rate == c.sample_rate and m.frame_rate == c.frame_rate
