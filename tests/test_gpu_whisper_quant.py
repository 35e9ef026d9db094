"""-m gpu: Whisper on MLX affine-quantised checkpoints (mis_whisper_set_tensor_quantized) vs the oracle.

Arithmetic contract (include/mi_speech.h): the decoder matrices every step re-reads and the tied vocab projection stream their codes with
quantizedMatmul's arithmetic (float32 group sums, scale and bias applied to them - no per-weight rounding) when they are 8 / 4 bit, group 64,
bf16 or f16 scales; the encoder, the cross-attention K/V projections and the token-embedding gather use s*q+b rounded to bf16 once at load.
So the oracle (WhisperOracle, round="bf16") gets float32 s*q+b for the streamed matrices and bf16-rounded s*q+b for everything else; the
fallbacks (2 bit, group 32) get bf16-rounded s*q+b everywhere.  Tolerances are those of test_gpu_whisper.py."""
import json

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
from mlx_audio_swift_amd import _lib
from gpu_util import observe, rms
from oracle import mel as omel
from oracle import mlxquant
from oracle import whisper as ow

pytestmark = pytest.mark.gpu

CFG = ow.WhisperConfig(vocab_size=700, num_mel_bins=80, d_model=256, encoder_layers=2, encoder_attention_heads=4, encoder_ffn_dim=1024,
                       decoder_layers=2, decoder_attention_heads=4, decoder_ffn_dim=1024)
ROLES = mas.stt.WHISPER_QUANT_ROLES
STREAMED = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "encoder_attn.q_proj",
            "encoder_attn.out_proj", "fc1", "fc2")
EMB = "model.decoder.embed_tokens.weight"
SDT = {"bf16": torch.bfloat16, "f16": torch.float16}


def _host_cfg(c):
    return mas.WhisperConfig(**{k: getattr(c, k) for k in mas.WhisperConfig.__dataclass_fields__})


def _linear_keys(W):
    """every Linear weight and the token embedding (WhisperModel.fromDirectory quantises exactly these, WhisperModel.swift:499-510)"""
    return [k for k, v in W.items() if k.endswith(".weight") and v.dim() == 2 and "embed_positions" not in k and "layer_norm" not in k]


def _is_streamed(k):
    return k == EMB or (k.startswith("model.decoder.layers.") and any(k.endswith(s + ".weight") for s in STREAMED))


def _quantize(W, spec):
    """spec(key) -> None (dense) or (bits, group, scale dtype name).  Returns {key: (wq, scales, biases, group, bits)} with scales / biases
    as torch tensors of the stored dtype, and the float32 s*q+b of each (from the STORED scales)."""
    Q, deq = {}, {}
    for k in _linear_keys(W):
        sp = spec(k)
        if sp is None:
            continue
        bits, group, sdt = sp
        wq, s, b = mlxquant.quantize(W[k].float().numpy(), group, bits)
        st, bt = torch.from_numpy(s).to(SDT[sdt]), torch.from_numpy(b).to(SDT[sdt])
        Q[k] = (wq, st, bt, group, bits)
        deq[k] = mlxquant.dequantize(wq, st.float().numpy(), bt.float().numpy(), group, bits)
    return Q, deq


def _native(k, Q, layer_qkv_ok):
    """would the engine stream this matrix as codes?"""
    if k not in Q or not _is_streamed(k):
        return False
    _, st, _, group, bits = Q[k]
    if bits not in (4, 8) or group != 64:
        return False
    if ".self_attn." in k and k.startswith("model.decoder.") and not k.endswith("out_proj.weight"):
        return layer_qkv_ok(k)
    return True


def _qkv_ok_fn(Q):
    def ok(k):
        base = k.rsplit(".self_attn.", 1)[0] + ".self_attn."
        ps = [base + p + "_proj.weight" for p in ("q", "k", "v")]
        if not all(p in Q for p in ps):
            return False
        sig = {(Q[p][4], Q[p][3], Q[p][1].dtype) for p in ps}
        return len(sig) == 1
    return ok


class _QOracle(ow.WhisperOracle):
    """WhisperOracle whose tied vocab projection uses its own matrix (float32 s*q+b where it streams natively) while the token gather keeps
    the bf16-rounded table."""

    def __init__(self, cfg, W, w_vocab):
        super().__init__(cfg, W, round="bf16")
        self.w_vocab = torch.as_tensor(w_vocab, dtype=torch.float32)

    def ln(self, x, p):
        y = super().ln(x, p)
        if p == "model.decoder.layer_norm":
            self._last = y
        return y

    def decode_row(self, b, tokens):
        super().decode_row(b, tokens)
        return self.r(self._last @ self.w_vocab.t())


def _build(cfg, W, Q, replicas=1):
    ms = []
    for _ in range(replicas):
        m = mas.WhisperModel(_host_cfg(cfg))
        for k, v in W.items():
            if k in Q:
                wq, st, bt, group, bits = Q[k]
                m.set_quantized_tensor(k, wq, st, bt, group, bits)
            else:
                m.set_tensor(k, v)
        m.finalize()
        ms.append(m)
    return ms if replicas > 1 else ms[0]


def _oracle(cfg, W, Q, deq):
    ok = _qkv_ok_fn(Q)
    OW = {}
    for k, v in W.items():
        if k in deq:
            f = torch.from_numpy(deq[k])
            OW[k] = f if (_native(k, Q, ok) and k != EMB) else f.bfloat16().float()
        else:
            OW[k] = v
    wv = deq[EMB] if _native(EMB, Q, ok) else OW[EMB].float().numpy()
    return _QOracle(cfg, OW, wv)


def _feats(B, n_mels, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, 3000, n_mels)) * 0.5).astype(np.float32)


def _check(dev, ref, max_tol=0.022, rms_tol=0.012):
    scale = float(np.abs(ref).max())
    assert observe("max_rel", float(np.abs(dev - ref).max()) / scale, max_tol), (float(np.abs(dev - ref).max()), scale)
    assert observe("rms_rel", rms(dev, ref) / float(np.sqrt(np.mean(ref.astype(np.float64) ** 2))), rms_tol)


def _teacher_forced(cfg, dev, oracle, B, steps, seed=2):
    feats = _feats(B, cfg.num_mel_bins, 1)
    oracle.reset(B)
    oracle.encode(feats)
    dev.encode(feats, want_output=False)
    rng = np.random.default_rng(seed)
    toks = rng.integers(0, cfg.vocab_size, (B, steps))
    dev.decoder_reset()
    got = [dev.decoder_forward(toks[:, t]) for t in range(steps)]
    ref = oracle.decode([toks[b] for b in range(B)])
    n_sure = 0
    for b in range(B):
        d = np.stack([g[b] for g in got]); r = ref[b].numpy()
        _check(d, r)
        err = float(np.abs(d - r).max())
        top2 = np.sort(r, axis=1)[:, -2:]
        sure = (top2[:, 1] - top2[:, 0]) > 2 * err
        n_sure += int(sure.sum())
        assert np.array_equal(d.argmax(1)[sure], r.argmax(1)[sure])
    assert n_sure > 0
    return got


def _all_bits(m):
    nb = m.native_quant_bits
    return {v for r in ROLES for v in nb[r]} | {nb["vocab"]}


@pytest.mark.parametrize("B", [2, 11, 17])
@pytest.mark.parametrize("sdt", ["bf16", "f16"])
@pytest.mark.parametrize("bits", [4, 8])
def test_quantised_decoder_matches_oracle(bits, sdt, B):
    W = ow.make_synthetic_weights(CFG, seed=777)
    Q, deq = _quantize(W, lambda k: (bits, 64, sdt))
    dev = _build(CFG, W, Q)
    assert _all_bits(dev) == {bits}                                   # every layer and role, and the vocab projection, stream codes
    _teacher_forced(CFG, dev, _oracle(CFG, W, Q, deq), B, 40)


def test_mixed_layers_match_oracle():
    # per-matrix formats across layers: every matrix is its own launch.  Layer 1's q|k|v mixes bits (-> the dense copy), its cross query
    # is dense (the fold into the attention kernel stays on for it), the vocab projection is dense.
    W = ow.make_synthetic_weights(CFG, seed=778)

    def spec(k):
        if k == EMB or k == "model.decoder.layers.1.encoder_attn.q_proj.weight":
            return None
        if k == "model.decoder.layers.1.self_attn.q_proj.weight":
            return (8, 64, "bf16")
        if k == "model.decoder.layers.1.fc1.weight":
            return (8, 64, "f16")
        return (4, 64, "bf16" if ".layers.0." in k else "f16")
    Q, deq = _quantize(W, spec)
    dev = _build(CFG, W, Q)
    nb = dev.native_quant_bits
    assert [nb[r][0] for r in ROLES] == [4] * 6
    assert [nb[r][1] for r in ROLES] == [0, 4, 0, 4, 8, 4] and nb["vocab"] == 0
    _teacher_forced(CFG, dev, _oracle(CFG, W, Q, deq), 3, 24)


@pytest.mark.parametrize("bits,group", [(4, 32), (2, 64)], ids=["group32", "2bit"])
def test_fallback_dequantises_at_load(bits, group):
    W = ow.make_synthetic_weights(CFG, seed=779)
    Q, deq = _quantize(W, lambda k: (bits, group, "bf16"))
    dev = _build(CFG, W, Q)
    assert _all_bits(dev) == {0}
    OW = {k: (torch.from_numpy(deq[k]).bfloat16().float() if k in deq else v) for k, v in W.items()}
    _teacher_forced(CFG, dev, ow.WhisperOracle(CFG, OW, round="bf16"), 2, 24)


def test_large_v3_widths_match_oracle():
    # d = 1280 (G = 20 scale groups), ffn 5120 (fc2: G = 80), V = 51866 (ragged Vpad), 8 rows: the bench's shapes
    cfg = ow.WhisperConfig(vocab_size=51866, num_mel_bins=128, d_model=1280, encoder_layers=1, encoder_attention_heads=20,
                           encoder_ffn_dim=5120, decoder_layers=2, decoder_attention_heads=20, decoder_ffn_dim=5120)
    W = ow.make_synthetic_weights(cfg, seed=780)
    Q, deq = _quantize(W, lambda k: (4, 64, "f16") if _is_streamed(k) else (8, 64, "bf16"))
    dev = _build(cfg, W, Q)
    assert _all_bits(dev) == {4}
    _teacher_forced(cfg, dev, _oracle(cfg, W, Q, deq), 8, 6)


def _sinusoid(d):
    half = d // 2
    inc = np.log(10000.0) / max(half - 1, 1)
    pos = np.arange(1500)[:, None] * np.exp(-inc * np.arange(half))[None]
    return torch.from_numpy(np.concatenate([np.sin(pos), np.cos(pos)], 1).astype(np.float32)).bfloat16()


def _mlx_name(k):
    attn = {"q_proj": "query", "k_proj": "key", "v_proj": "value", "out_proj": "out"}
    k2 = k[len("model."):]
    if k2 == "decoder.embed_positions.weight":
        return "decoder.positional_embedding"
    if k2.startswith("decoder.embed_tokens."):
        return "decoder.token_embedding." + k2.split(".", 2)[2]
    if k2.startswith("encoder.conv"):
        return k2
    if k2.startswith("encoder.layer_norm."):
        return "encoder.ln_post." + k2.split(".", 2)[2]
    if k2.startswith("decoder.layer_norm."):
        return "decoder.ln." + k2.split(".", 2)[2]
    stem, _, idx, rest = k2.split(".", 3)
    head, tail = rest.split(".", 1)
    if head == "self_attn_layer_norm":
        r = "attn_ln." + tail
    elif head == "encoder_attn_layer_norm":
        r = "cross_attn_ln." + tail
    elif head == "final_layer_norm":
        r = "mlp_ln." + tail
    elif head in ("fc1", "fc2"):
        r = ("mlp1." if head == "fc1" else "mlp2.") + tail
    else:
        proj, t2 = tail.split(".", 1)
        r = ("attn." if head == "self_attn" else "cross_attn.") + attn[proj] + "." + t2
    return f"{stem}.blocks.{idx}.{r}"


def test_model_directory_quantised_hf_and_mlx_layouts(tmp_path):
    # fromDirectory on quantised checkpoints (WhisperModel.swift:499-510): config.json's `quantization` + `.scales` / `.biases` per Linear.
    # The scale / bias values are bf16 values (exact in f16 as well): the HF directory stores them as bf16, the mlx-whisper one (MLX conv
    # layout, no encoder positions) as f16 - both stream natively and must give bit-identical logits, equal to set_quantized_tensor's.
    from safetensors.torch import save_file
    cfg = CFG
    W = ow.make_synthetic_weights(cfg, seed=781)
    W["model.encoder.embed_positions.weight"] = _sinusoid(cfg.d_model)
    Q, _ = _quantize(W, lambda k: (4, 64, "bf16"))
    ref = _build(cfg, W, Q)
    conf = {k: getattr(cfg, k) for k in mas.WhisperConfig.__dataclass_fields__}
    conf["quantization"] = {"group_size": 64, "bits": 4}
    for layout in ("hf", "mlx"):
        d = tmp_path / layout
        d.mkdir()
        T = {}
        for k, v in W.items():
            if layout == "mlx" and k == "model.encoder.embed_positions.weight":
                continue                                                 # mlx-whisper omits the fixed sinusoid
            name = k if layout == "hf" else _mlx_name(k)
            if layout == "mlx" and k in ("model.encoder.conv1.weight", "model.encoder.conv2.weight"):
                v = v.permute(0, 2, 1).contiguous()                      # [out, in, k] -> MLX [out, k, in]
            if k in Q:
                wq, st, bt, _, _ = Q[k]
                base = name[: -len(".weight")]
                sd = torch.bfloat16 if layout == "hf" else torch.float16
                T[name] = torch.from_numpy(wq.astype(np.uint32))
                T[base + ".scales"] = st.to(sd).contiguous()
                T[base + ".biases"] = bt.to(sd).contiguous()
            else:
                T[name] = v.contiguous()
        if layout == "hf":
            T["proj_out.weight"] = T["model.decoder.embed_tokens.weight"].clone()
            T["proj_out.scales"] = T["model.decoder.embed_tokens.scales"].clone()
            T["proj_out.biases"] = T["model.decoder.embed_tokens.biases"].clone()
        save_file(T, str(d / "model.safetensors"))
        (d / "config.json").write_text(json.dumps(conf))
    a = mas.WhisperModel.from_model_directory(str(tmp_path / "hf"))
    b = mas.WhisperModel.from_model_directory(str(tmp_path / "mlx"))
    assert _all_bits(a) == {4} and _all_bits(b) == {4}
    f = _feats(2, cfg.num_mel_bins, 3)
    outs = []
    for m in (ref, a, b):
        m.encode(f, want_output=False)
        m.decoder_reset()
        outs.append(np.stack([m.decoder_forward(np.asarray([3 + t, 5 + 2 * t], np.int32)) for t in range(4)]))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    # a uint32 weight without scales is refused loudly
    bad = tmp_path / "bad"
    bad.mkdir()
    save_file({"decoder.blocks.0.mlp1.weight": torch.from_numpy(Q["model.decoder.layers.0.fc1.weight"][0].astype(np.uint32))},
              str(bad / "model.safetensors"))
    (bad / "config.json").write_text(json.dumps(conf))
    with pytest.raises(mas.AudioGenerationError, match="without .scales"):
        mas.WhisperModel.from_model_directory(str(bad))


def _windows():
    rng = np.random.default_rng(4)
    t = np.arange(16000 * 4) / 16000.0
    return [(0.2 * np.sin(2 * np.pi * 330 * t) + 0.02 * rng.standard_normal(len(t))).astype(np.float32),
            (0.1 * rng.standard_normal(16000 * 2)).astype(np.float32),
            (0.05 * rng.standard_normal(16000 * 3)).astype(np.float32)]


def test_transcription_stream_oracle_and_fold_errors(monkeypatch):
    W = ow.make_synthetic_weights(CFG, seed=782)
    Q, deq = _quantize(W, lambda k: (4, 64, "f16"))
    dev = _build(CFG, W, Q)
    wins = _windows()
    prompt = [690, 691, 692, 693]
    eot, ts_begin = 699, 660
    gp = mas.STTGenerateParameters(max_tokens=12, temperature=0.0, eot_id=eot, timestamp_begin=ts_begin, suppress_tokens=[1, 2, 3],
                                   begin_suppress_tokens=[eot, 10])
    ids = dev.transcribe_windows(wins, prompt, gp)                    # default MIS_WHISPER_FOLD: the folds stand down for quantised matrices
    assert len(ids) == 3 and all(len(x) <= 12 for x in ids)
    ev = list(dev.transcribe_windows_stream(wins, prompt, gp))
    for row in range(3):
        assert [e.token for e in ev if e.row == row and isinstance(e, mas.TokenEvent)] == ids[row]
    oracle = _oracle(CFG, W, Q, deq)
    oracle.reset(3)
    oracle.encode([omel.encoder_features(w, 80)[0] for w in wins])
    for b in range(3):
        with torch.no_grad():
            lg = oracle.decode_row(b, prompt + ids[b]).numpy()
        tol = 0.05 * float(np.abs(lg).max())
        for i, tok in enumerate(ids[b]):
            l = ow.apply_suppress(lg[len(prompt) - 1 + i], i, [eot, 10], [1, 2, 3], ts_begin)
            assert tok < ts_begin and tok not in (1, 2, 3)
            assert l[tok] >= l.max() - tol, (b, i)
    # bit 8 of MIS_WHISPER_FOLD: the requested folds (cross q into the attention kernel, fc1 behind LayerNorm 3) cannot apply here
    dev.encode(_feats(3, 80, 5), want_output=False)
    monkeypatch.setenv("MIS_WHISPER_FOLD", "28")
    with pytest.raises(mas.AudioGenerationError, match="MIS_WHISPER_FOLD"):
        dev.decoder_forward(np.asarray([1, 2, 3], np.int32))
    monkeypatch.setenv("MIS_WHISPER_FOLD", "0")                       # the separate launches: same logits as the default step
    dev.decoder_reset()
    l0 = dev.decoder_forward(np.asarray([1, 2, 3], np.int32))
    monkeypatch.delenv("MIS_WHISPER_FOLD")
    dev.decoder_reset()
    assert np.array_equal(l0, dev.decoder_forward(np.asarray([1, 2, 3], np.int32)))


def test_two_shards_return_the_unsharded_ids():
    W = ow.make_synthetic_weights(CFG, seed=783)
    Q, _ = _quantize(W, lambda k: (8, 64, "bf16"))
    r0, r1 = _build(CFG, W, Q, replicas=2)
    wins = _windows() + _windows()[:1]
    gp = mas.STTGenerateParameters(max_tokens=10, temperature=0.0, eot_id=699, timestamp_begin=660)
    one = r0.transcribe_windows(wins, [690, 691], gp)
    two = r0.transcribe_windows(wins, [690, 691], gp, replicas=[r0, r1])
    assert one == two


def _weight_bytes(m):
    return int(_lib.lib().mis_debug_whisper_weight_bytes(m._h))


def test_footprint_of_a_4bit_model():
    cfg = CFG
    d, fe, fd, V, T, Le, Ld = cfg.d_model, cfg.encoder_ffn_dim, cfg.decoder_ffn_dim, cfg.vocab_size, cfg.max_target_positions, \
        cfg.encoder_layers, cfg.decoder_layers
    Vpad = -(-V // 16) * 16
    K1 = -(-3 * cfg.num_mel_bins // 32) * 32
    bits = 4
    # bf16 elements held by every model: conv stem, encoder positions (1500 rows), encoder layers (dequantised at load), the gather table,
    # decoder positions, cross K/V, every bias and LayerNorm
    common = d * K1 + d + d * 3 * d + d + 1500 * d + 2 * d
    common += Le * (3 * d * d + 3 * d + d * d + d + fe * d + fe + d * fe + d + 4 * d)
    common += V * d + T * d + 2 * d
    common += Ld * (3 * d + d + d + 2 * d * d + 2 * d + d + fd + d + 6 * d)
    streamed = Ld * (6 * d * d + 2 * fd * d) + Vpad * d                 # decoder matrices + the tied vocab projection (element count)
    dense_expected = 2 * (common + streamed)

    def qbytes(N, K):                                                   # codes + one (scale, bias) pair of 16-bit values per row and group
        return N * K * bits // 8 + N * (K // 64) * 4
    q_expected = 2 * common + Ld * (qbytes(3 * d, d) + 3 * qbytes(d, d) + qbytes(fd, d) + qbytes(d, fd)) + qbytes(Vpad, d)
    slots = Le * 12 + Ld * 20 + 16                                      # the arena's 64-element alignment allowance per tensor
    W = ow.make_synthetic_weights(cfg, seed=784)
    dense = mas.WhisperModel.from_weights(_host_cfg(cfg), W)
    Q, _ = _quantize(W, lambda k: (bits, 64, "bf16"))
    q = _build(cfg, W, Q)
    assert _all_bits(q) == {4}
    gd, gq = _weight_bytes(dense), _weight_bytes(q)
    assert 0 <= gd - dense_expected <= 128 * slots, (gd, dense_expected)
    assert 0 <= gq - q_expected <= 128 * slots + 2 * 256 * (6 * Ld + 1), (gq, q_expected)
    assert gd - gq >= 0.7 * 2 * streamed, (gd, gq, streamed)          # 4 bit: 0.5625 of 2 bytes per weight -> saves ~0.72
    syn = mas.WhisperModel.synthetic(_host_cfg(cfg), quant_bits=4, scale_dtype="f16")
    assert _all_bits(syn) == {4} and _weight_bytes(syn) == gq
