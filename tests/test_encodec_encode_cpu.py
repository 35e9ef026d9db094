"""The EnCodec encode specification (tests/encodec_encode_ref.py) against transformers' EncodecModel, its own invariants, and the host
pieces of mlx_audio_swift_amd that need no GPU (chunk walk, preprocess_encodec_audio, the bandwidth table)."""
import math
from dataclasses import replace

import numpy as np
import pytest
import torch

import encodec_encode_ref as er
from oracle import encodec as oe


def hf_model(cfg, W, normalize):
    from transformers import EncodecConfig, EncodecModel
    hc = EncodecConfig(
        target_bandwidths=list(cfg.target_bandwidths), sampling_rate=cfg.sampling_rate, audio_channels=cfg.audio_channels, normalize=normalize,
        chunk_length_s=None, overlap=None, hidden_size=cfg.hidden_size, num_filters=cfg.num_filters, num_residual_layers=cfg.num_residual_layers,
        upsampling_ratios=list(cfg.upsampling_ratios), norm_type=cfg.norm_type, kernel_size=cfg.kernel_size, last_kernel_size=cfg.last_kernel_size,
        residual_kernel_size=cfg.residual_kernel_size, dilation_growth_rate=cfg.dilation_growth_rate, use_causal_conv=cfg.use_causal_conv,
        pad_mode=cfg.pad_mode, compress=cfg.compress, num_lstm_layers=cfg.num_lstm_layers, trim_right_ratio=cfg.trim_right_ratio,
        codebook_size=cfg.codebook_size, codebook_dim=cfg.codebook_dim, use_conv_shortcut=cfg.use_conv_shortcut)
    m = EncodecModel(hc).double().eval()
    sd = m.state_dict()
    new = {}
    for k in sd:
        if not (k.startswith("encoder.") or k.startswith("quantizer.")):
            continue
        if k.endswith("codebook.embed"):
            if k in W:                                                       # transformers sizes the layer list by log2(codebook_size) bits
                new[k] = torch.as_tensor(np.asarray(W[k], np.float64))
        elif ".lstm." in k:
            p, leaf = k.rsplit(".lstm.", 1)                              # weight_ih_l0 ...
            kind, layer = leaf.rsplit("_l", 1)
            base = f"{p}.lstm.{layer}"
            if kind == "weight_ih":
                new[k] = torch.as_tensor(np.asarray(W[base + ".Wx"], np.float64))
            elif kind == "weight_hh":
                new[k] = torch.as_tensor(np.asarray(W[base + ".Wh"], np.float64))
            elif kind == "bias_ih":
                new[k] = torch.as_tensor(np.asarray(W[base + ".bias"], np.float64))
            else:
                new[k] = torch.zeros_like(sd[k])
        elif k.endswith("parametrizations.weight.original1") or k.endswith("conv.weight"):
            p = k.split(".conv.")[0]
            new[k] = torch.as_tensor(np.asarray(W[p + ".conv.weight"], np.float64)).permute(0, 2, 1).contiguous()      # [co, ci, k]
        elif k.endswith("parametrizations.weight.original0"):
            p = k.split(".conv.")[0]
            w = torch.as_tensor(np.asarray(W[p + ".conv.weight"], np.float64))
            new[k] = w.reshape(w.shape[0], -1).norm(dim=1).reshape(-1, 1, 1)
        elif k.endswith("conv.bias"):
            new[k] = torch.as_tensor(np.asarray(W[k], np.float64))
        elif ".norm." in k:
            new[k] = torch.as_tensor(np.asarray(W[k], np.float64))
        elif k.endswith("codebook.inited") or k.endswith("cluster_size") or k.endswith("embed_avg"):
            continue
        else:
            raise AssertionError("unmapped transformers key " + k)
    missing, unexpected = m.load_state_dict(new, strict=False)
    assert not unexpected and not [k for k in missing if k.startswith("encoder.")], (missing, unexpected)
    return m


@pytest.mark.parametrize("name", ["tiny", "tiny_48k"])                     # transformers takes power-of-two codebooks only
def test_reference_matches_transformers(name):
    cfg, normalize = er.CONFIGS[name], er.is_normalize(name)
    W = er.make_synthetic_weights(cfg)
    ref = er.EncodeRef(cfg, W, normalize=normalize)
    m = hf_model(cfg, W, normalize)
    hop = cfg.hop_length
    # the last two need extra padding at every level; every conv sees more samples than its padding, where transformers' reflect
    # rule (zero-extend, then reflect) and the reference's (clamped indices) are the same function
    for L in (9 * hop, 7 * hop - 3, 8 * hop + 1):
        x = er.audio_rows(cfg, L, 2, seed=L)                                # [B, L, C]
        for bw in cfg.target_bandwidths[:2]:
            with torch.no_grad():
                out = m.encode(torch.as_tensor(x, dtype=torch.float64).permute(0, 2, 1), bandwidth=bw)
                emb = m.encoder(torch.as_tensor(ref.normalise(np.swapaxes(x, 1, 2))[0]))
            codes, scales = ref.encode(x, bandwidth=bw)
            mine = ref.encoder(np.swapaxes(x, 1, 2))
            assert mine.shape == (2, cfg.hidden_size, er.num_frames(cfg, L))
            assert np.abs(mine - emb.numpy()).max() <= 1e-10 * np.abs(mine).max()
            assert codes.shape == tuple(out.audio_codes.shape) == (1, 2, er.num_quantizers_for_bandwidth(cfg, bw), er.num_frames(cfg, L))
            assert np.array_equal(codes, out.audio_codes.numpy())
            if normalize:
                assert np.allclose(scales[0], out.audio_scales[0].numpy().ravel(), rtol=1e-12, atol=0)
            else:
                assert scales[0] is None


def test_frame_counts_are_ceil_chains():
    for cfg in er.CONFIGS.values():
        ref = er.EncodeRef(cfg, er.make_synthetic_weights(cfg))
        for L in er.row_lengths(cfg) + [2, cfg.hop_length + 1]:
            n = L
            for r in reversed(cfg.upsampling_ratios):
                n = math.ceil(n / r)
            assert ref.encoder(np.zeros((1, cfg.audio_channels, L))).shape[-1] == n == er.num_frames(cfg, L)


def test_bandwidth_table():
    cfg = oe.EncodecConfig()                                               # 24 kHz: 75 frames/s, 10 bits a code
    assert cfg.num_quantizers == 32
    assert [er.num_quantizers_for_bandwidth(cfg, b) for b in cfg.target_bandwidths] == [2, 4, 8, 16, 32]
    assert er.num_quantizers_for_bandwidth(cfg, None) == 32 and er.num_quantizers_for_bandwidth(cfg, 0.1) == 1
    c48 = oe.EncodecConfig(audio_channels=2, upsampling_ratios=(8, 5, 4, 2), sampling_rate=48000, target_bandwidths=(3.0, 6.0, 12.0, 24.0))
    assert [er.num_quantizers_for_bandwidth(c48, b) for b in c48.target_bandwidths] == [2, 4, 8, 16]
    import mlx_audio_swift_amd as mas
    hc = mas.EncodecConfig()
    assert [hc.num_quantizers_for_bandwidth(b) for b in hc.target_bandwidths] == [2, 4, 8, 16, 32] and hc.num_quantizers_for_bandwidth(None) == 32


def _walk_literal(L, chunk_length, chunk_stride):
    """Encodec.swift:266-287, line by line"""
    chunk_len = chunk_length if chunk_length is not None else L
    stride = chunk_stride if chunk_stride is not None else L
    step = chunk_len - stride
    if chunk_length is None:
        chunk_len = L
    out, offset = [], 0
    while offset < L - step:
        out.append((offset, offset + chunk_len))
        offset += stride
    return out


def _preprocess_literal(raw, chunk_length, chunk_stride):
    """Encodec.swift:484-514, line by line"""
    audio = [x[:, None] if x.ndim == 1 else x for x in raw]
    max_length = max(x.shape[0] for x in audio)
    if chunk_length is not None and chunk_stride is not None:
        max_length += chunk_length - (max_length % chunk_stride)
    inputs, masks = [], []
    for x in audio:
        length = x.shape[0]
        mask = np.ones(length, bool)
        difference = max_length - length
        if difference > 0:
            mask = np.pad(mask, (0, difference))
            x = np.pad(x, ((0, difference), (0, 0)))
        inputs.append(x)
        masks.append(mask)
    return np.stack(inputs), np.stack(masks)


def test_chunk_walk_and_preprocess_match_transliterations():
    import mlx_audio_swift_amd as mas
    cfg = oe.TINY
    for L, chunk, stride in ((300, 120, 90), (120, 120, 90), (121, 120, 90), (390, 120, 90), (77, None, None), (240, 120, 120)):
        ref = er.EncodeRef(cfg, {}, chunk_length=chunk, chunk_stride=stride)
        offs, n = ref.chunk_offsets(L)
        assert [(o, o + n) for o in offs] == _walk_literal(L, chunk, stride)
    rng = np.random.default_rng(3)
    for lens, chunk, stride in (((100, 37), None, None), ((100, 37), 120, 90), ((90,), 120, 90), ((250, 251), 120, 90)):
        raw = [rng.standard_normal((n, 2)).astype(np.float32) for n in lens]
        a, m = mas.preprocess_encodec_audio(raw, 1200, chunk, stride)
        b, k = _preprocess_literal(raw, chunk, stride)
        assert a.dtype == np.float32 and m.dtype == bool and np.array_equal(a, b) and np.array_equal(m, k)
    a, m = mas.preprocess_encodec_audio([np.ones(5, np.float32)])
    assert a.shape == (1, 5, 1) and m.all()
    # a preprocessed input walks into whole chunks only
    a, m = mas.preprocess_encodec_audio([np.ones(250, np.float32)], 1200, 120, 90)
    assert all(e <= a.shape[1] for _, e in _walk_literal(a.shape[1], 120, 90))


# ---- the exact-grid RVQ case shared with the GPU test
def exact_grid_case(cfg, frames, rows, seed=5):
    """Embeddings on the grid 2^-3 Z, |x| <= 2, codebooks on 2^-2 Z, |e| <= 1 (D <= 32): products are multiples of 2^-5 below 4, the
    D-term sums multiples of 2^-5 below 2^9 - exact in float32 in any order, as are |e|^2, 2 r.e - |e|^2 and every r - e.  Row 1 of
    each codebook duplicates row 0 (an exact tie on every frame that picks it) and frame 0 sits midway between rows 2 and 3."""
    rng = np.random.default_rng(seed)
    nq, CB, D = cfg.num_quantizers, cfg.codebook_size, cfg.codebook_dim
    W = {}
    for q in range(nq):
        E = rng.integers(-4, 5, (CB, D)) / 4.0
        E[1] = E[0]
        E[3] = E[2]
        E[3, 0] = E[2, 0] + 0.5
        W[f"quantizer.layers.{q}.codebook.embed"] = E.astype(np.float32)
    emb = (rng.integers(-16, 17, (rows, D, frames)) / 8.0).astype(np.float32)
    E0 = W["quantizer.layers.0.codebook.embed"]
    emb[:, :, 0] = ((E0[2] + E0[3]) / 2.0)[None, :]                          # equidistant from rows 2 and 3 (grid 2^-3)
    if frames > 1:
        emb[:, :, 1] = E0[0][None, :]                                         # exactly rows 0 and 1
    return W, emb


def test_exact_grid_case_is_exact_and_has_ties():
    cfg = oe.TINY
    W, emb = exact_grid_case(cfg, 33, 2)
    full = dict(er.make_synthetic_weights(cfg))
    full.update(W)
    ref = er.EncodeRef(cfg, full)
    codes, res, gaps, _ = ref.rvq(emb, cfg.num_quantizers)
    assert (gaps[:, 0, :2] == 0).all() and (codes[:, 0, 1] == 0).all() and (codes[:, 0, 0] <= 2).all()        # planted ties, lower index wins
    assert (gaps == 0).sum() >= 4
    # every residual stays on the float32-exact grid, and float32 scores in two different summation orders equal the float64 ones
    assert np.array_equal(res.astype(np.float32).astype(np.float64), res) and np.abs(res * 8 - np.round(res * 8)).max() == 0
    r32 = np.swapaxes(res[0], 1, 2).astype(np.float32)
    E32 = W["quantizer.layers.0.codebook.embed"]
    for order in (np.arange(cfg.codebook_dim), np.random.default_rng(0).permutation(cfg.codebook_dim)):
        acc = np.zeros(r32.shape[:2] + (E32.shape[0],), np.float32)
        for d in order:
            acc = (acc + r32[..., d, None] * E32[None, None, :, d]).astype(np.float32)
        s32 = (np.float32(2) * acc - (E32 ** 2).sum(-1, dtype=np.float32)).astype(np.float32)
        s64 = 2 * (r32.astype(np.float64) @ E32.astype(np.float64).T) - (E32.astype(np.float64) ** 2).sum(-1)
        assert np.array_equal(s32.astype(np.float64), s64)


@pytest.mark.parametrize("fault", ["extra0", "reflect_swap", "tie_high", "no_update"])
def test_planted_faults_change_the_expected_outputs(fault):
    cfg = oe.TINY
    W = er.make_synthetic_weights(cfg)
    x = er.audio_rows(cfg, 7 * cfg.hop_length - 3, 1, seed=11)
    good, bad = er.EncodeRef(cfg, W), er.EncodeRef(cfg, W, fault=fault)
    if fault in ("extra0", "reflect_swap"):
        a, b = good.encoder(np.swapaxes(x, 1, 2)), bad.encoder(np.swapaxes(x, 1, 2))
        assert a.shape != b.shape or np.abs(a - b).max() > 1e-3 * np.abs(a).max()
    else:
        Wg, emb = exact_grid_case(cfg, 5, 1)
        full = dict(W)
        full.update(Wg)
        a, b = er.EncodeRef(cfg, full).rvq(emb, cfg.num_quantizers), er.EncodeRef(cfg, full, fault=fault).rvq(emb, cfg.num_quantizers)
        assert not np.array_equal(a[0], b[0]) or not np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", ["tiny", "tiny_48k", "wide"])
def test_exempt_share_of_the_end_to_end_inputs(name):
    cfg = er.CONFIGS[name]
    ref = er.EncodeRef(cfg, er.make_synthetic_weights(cfg), normalize=er.is_normalize(name))
    for i, L in enumerate(er.row_lengths(cfg)):
        x = er.audio_rows(cfg, L, 1 + i % 3, seed=100 + i)
        emb = ref.encoder(np.swapaxes(x, 1, 2))
        _, _, gaps, bounds = ref.rvq(emb, cfg.num_quantizers)
        assert er.exempt_mask(gaps, bounds).mean() <= er.EXEMPT_CAP, (name, L)


def test_config_from_dict_and_expected_keys():
    import mlx_audio_swift_amd as mas
    from mlx_audio_swift_amd.codecs import encodec_expected_shapes
    d = dict(model_type="encodec", audio_channels=2, normalize=True, chunk_length_s=1.0, overlap=0.01, norm_type="time_group_norm",
             use_causal_conv=False, upsampling_ratios=[8, 5, 4, 2], target_bandwidths=[3.0, 6.0], sampling_rate=48000, architectures=["x"])
    c = mas.EncodecConfig.from_dict(d)
    assert c.normalize and c.audio_channels == 2 and c.upsampling_ratios == (8, 5, 4, 2) and c.chunk_length == 48000 and c.chunk_stride == 47520
    for name, cfg in er.CONFIGS.items():
        hc = mas.EncodecConfig(**{k: getattr(cfg, k) for k in mas.EncodecConfig.__dataclass_fields__ if hasattr(cfg, k)})
        W = er.make_synthetic_weights(cfg)
        assert {k: tuple(v.shape) for k, v in W.items()} == encodec_expected_shapes(hc)
        assert set(oe.make_synthetic_weights(cfg)) == set(encodec_expected_shapes(hc, encoder=False))
