"""-m gpu: the bf16 form of Sortformer: the two kernels of csrc/sortformer_tf_bf16.h through their debug entry points, and the chain through
SortformerModel with encoder_dtype="bfloat16".  References are float64 torch with .to(torch.bfloat16) at the contract's rounding points
(include/mi_speech.h); the gate forms are test_gpu_parakeet_bf16.py's, derived there: a rounded-operand result <= 2 x rel(rounded float64
reference, float64) + 2^-23; a layer tap <= 4 x D_w + 2^-23 on the device's own previous tap, D_w the distance between the float64 layer with
bf16-rounded matrices and the one with unrounded matrices.  The chain's gates need the weights on the host, so those models are built by
from_weights; synthetic() is held to the launch formula and to finite probabilities.
MIS_SORTFORMER_BF16_PARITY_LOG=<file> keeps every observed value (profiles/sortformer_bf16/parity_observed.jsonl)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import mlx_audio_swift_amd as mas
from mlx_audio_swift_amd.generation import check
import sortformer_ref as R
from test_gpu_parakeet_bf16 import BLOCK_MATRICES, KEYS, _bits, _ptr, _rb, _rel, _wide

pytestmark = pytest.mark.gpu
F64 = torch.float64
TAIL_ROWS = (1, 15, 17, 33)
TF_MATRICES = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "fc1", "fc2")


def _gate(kind, value, tol):
    name = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].split("::")[-1]
    if os.environ.get("MIS_SORTFORMER_BF16_PARITY_LOG"):
        with open(os.environ["MIS_SORTFORMER_BF16_PARITY_LOG"], "a") as f:
            f.write(json.dumps(dict(test=name, kind=kind, value=float(value), tol=None if tol is None else float(tol))) + "\n")
    print(f"{name} {kind}: {value:.3e} (tol {tol if tol is None else format(tol, '.3e')})")
    return tol is None or value <= tol


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("hd", [24, 32, 64])
def test_tf_attention(hd):
    """one ragged launch, 5 heads (a head block of 4 and one of 1), NaN behind every count; a one-key row returns V bit for bit"""
    H, Tp, B = 5, max(KEYS), len(KEYS)
    g = torch.Generator().manual_seed(hd)
    w = H * hd
    qkv = torch.full((B, Tp, 3 * w), float("nan"), dtype=F64)
    for b, n in enumerate(KEYS):
        qkv[b, :n] = _rb(torch.randn(n, 3 * w, generator=g, dtype=F64))
    qb, cnt, out = _bits(qkv), np.asarray(KEYS, np.int32), np.zeros((B, Tp, w), np.uint16)
    scale = float(np.float32(hd) ** np.float32(-0.5))
    check(mas._lib.lib().mis_debug_sortformer_tf_attn_bf16(0, _ptr(qb), 3 * w, w, 2 * w, _ptr(cnt), B, Tp, H, hd, scale, w, _ptr(out)))
    dev, ok = _wide(out), True
    for b, n in enumerate(KEYS):
        q, k, v = (qkv[b, :n, i * w:(i + 1) * w].reshape(n, H, hd).transpose(0, 1) for i in range(3))
        r64 = (torch.softmax((q * scale) @ k.transpose(1, 2), -1) @ v).transpose(0, 1).reshape(n, w)
        s = _rb(q * scale) @ k.transpose(1, 2)
        e = torch.exp(s - s.max(-1, keepdim=True).values)
        rr = _rb(((_rb(e) @ v) / e.sum(-1, keepdim=True)).transpose(0, 1).reshape(n, w))
        ok &= _gate(f"tf attn hd {hd} keys {n}", _rel(dev[b, :n], r64), 2 * _rel(rr, r64) + 2.0 ** -23)
        assert not out[b, n:].any()
    assert np.array_equal(out[0, :1], qb[0, :1, 2 * w:])
    assert ok


def _tail64(att, g, P, eps, rounded):
    """x1 = LN1(g + o(att) + b_o), g' = LN2(x1 + fc2(ReLU(fc1(x1) + b1)) + b2) in float64; rounded: x1 as fc1's operand and the hidden tile"""
    rnd = _rb if rounded else (lambda t: t)
    x1 = Fn.layer_norm(g + att @ P["Wo"].T + P["bo"], g.shape[-1:], P["ln1w"], P["ln1b"], eps)
    h = rnd(torch.relu(rnd(x1) @ P["W1"].T + P["b1"]))
    return Fn.layer_norm(x1 + h @ P["W2"].T + P["b2"], g.shape[-1:], P["ln2w"], P["ln2b"], eps)


@pytest.mark.parametrize("dt,ft", [(192, 768), (32, 32), (256, 1024), (96, 160)])
def test_tf_tail(dt, ft):
    """one ragged launch over three 16-row tiles, NaN behind the counts in both inputs; g16 is bf16(g') bit for bit"""
    gen = torch.Generator().manual_seed(dt + ft)
    normal = lambda *s: torch.randn(*s, generator=gen, dtype=F64)
    B, Tp, eps = len(TAIL_ROWS), max(TAIL_ROWS), 1e-5
    att, g = (torch.full((B, Tp, dt), float("nan"), dtype=F64) for _ in range(2))
    for b, n in enumerate(TAIL_ROWS):
        att[b, :n], g[b, :n] = _rb(normal(n, dt)), normal(n, dt).float().to(F64)
    P = dict(Wo=_rb(0.5 * normal(dt, dt) / dt ** 0.5), W1=_rb(normal(ft, dt) / dt ** 0.5), W2=_rb(0.5 * normal(dt, ft) / ft ** 0.5))
    P.update({k: (0.05 * normal(ft if k == "b1" else dt) + (1.0 if k.endswith("w") else 0.0)).float().to(F64)
              for k in ("bo", "b1", "b2", "ln1w", "ln1b", "ln2w", "ln2b")})
    f32 = lambda t: np.ascontiguousarray(t.to(torch.float32).numpy())
    keep = [_bits(att), f32(g), np.asarray(TAIL_ROWS, np.int32)] + [_bits(P[k]) if k[0] == "W" else f32(P[k])
                                                                   for k in ("Wo", "bo", "ln1w", "ln1b", "W1", "b1", "W2", "b2", "ln2w", "ln2b")]
    gout, g16 = np.zeros((B, Tp, dt), np.float32), np.zeros((B, Tp, dt), np.uint16)
    check(mas._lib.lib().mis_debug_sortformer_tf_tail_bf16(0, *(_ptr(a) for a in keep[:3]), B, Tp, dt, ft, eps, *(_ptr(a) for a in keep[3:]), _ptr(gout),
                                                           _ptr(g16)))
    dev, ok = torch.from_numpy(gout).to(F64), True
    for b, n in enumerate(TAIL_ROWS):
        exact, rounded = (_tail64(att[b, :n], g[b, :n], P, eps, r) for r in (False, True))
        ok &= _gate(f"tf tail {dt}/{ft} rows {n}", _rel(dev[b, :n], exact), 2 * _rel(rounded, exact) + 2.0 ** -23)
        assert not gout[b, n:].any() and not g16[b, n:].any()
    assert np.array_equal(g16, _bits(torch.from_numpy(gout)))
    assert ok


def _cfg(wide, fc=None, tf=None, **kw):
    """two Conformer blocks, two BART layers: 128 / head 64 with the published tower 192 / 8 heads of 24 / 768, or the smallest legal widths;
    fc / tf override single fields"""
    fcd = (dict(hidden_size=128, intermediate_size=256, num_mel_bins=32, subsampling_conv_channels=32) if wide else
           dict(hidden_size=32, intermediate_size=32, num_mel_bins=16, subsampling_conv_channels=8, conv_kernel_size=5))
    tfd = dict(d_model=192, encoder_attention_heads=8, encoder_ffn_dim=768) if wide else dict(d_model=32, encoder_attention_heads=2, encoder_ffn_dim=32)
    e = mas.FCEncoderConfig(**{**dict(num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2), **fcd, **(fc or {})})
    t = mas.TFEncoderConfig(**{**dict(encoder_layers=2), **tfd, **(tf or {})})
    return mas.SortformerConfig(fc_encoder_config=e, tf_encoder_config=t, modules_config=mas.ModulesConfig(fc_d_model=e.hidden_size, tf_d_model=t.d_model),
                                processor_config=mas.ProcessorConfig(feature_size=e.num_mel_bins), max_batch=4, max_seconds=8, **kw)


def _waves():
    return [R.test_wave(40 + i, int(16000 * s) + 37 * i) for i, s in enumerate((0.3, 1.0, 2.5))]


def _bf16_launches(cfg, around=12):
    """include/mi_speech.h, bf16 mode: 15 launches a Conformer block, 3 a BART layer; 12 around them from samples, 5 from embeddings"""
    return around + 15 * cfg.fc_encoder_config.num_hidden_layers + 3 * cfg.tf_encoder_config.encoder_layers


@pytest.mark.parametrize("wide", [True, False])
def test_chain(wide):
    cfg = _cfg(wide)
    L, Lt = cfg.fc_encoder_config.num_hidden_layers, cfg.tf_encoder_config.encoder_layers
    W, waves = R.synthetic_weights(cfg, 5, R.HEAD_GAIN), _waves()
    Wr = dict(W)
    for key in [f"fc_encoder.layers.{i}.{n}.weight" for i in range(L) for n in BLOCK_MATRICES] + [f"tf_encoder.layers.{i}.{n}.weight" for i in range(Lt)
                                                                                                 for n in TF_MATRICES]:
        Wr[key] = torch.as_tensor(W[key]).to(torch.bfloat16).float().numpy()
    m, f32 = mas.SortformerModel.from_weights(cfg, W, encoder_dtype="bfloat16"), mas.SortformerModel.from_weights(cfg, W)
    probs = m.forward(waves, junk=np.nan)
    assert m.launches == _bf16_launches(cfg) == m.expected_launches["forward"]
    _, T = m.frames([len(w) for w in waves])
    taps = [m.tap(s) for s in range(L + Lt + 3)]
    assert np.array_equal(_u32(taps[-1]), _u32(probs)) and np.isfinite(probs).all() and probs.min() >= 0 and probs.max() <= 1
    exact, rounded, ok = R.Ref(cfg, W, F64), R.Ref(cfg, Wr, F64), True
    for b in range(len(waves)):
        n = int(T[b])
        for s in [*range(1, L + 1), *range(L + 2, L + Lt + 2)]:            # every Conformer block, every BART layer (the projection is f32 code)
            spec, plain = rounded.stage_after(s, taps[s - 1][b, :n]), exact.stage_after(s, taps[s - 1][b, :n])
            ok &= _gate(f"row {b} stage {s}", _rel(taps[s][b, :n], spec), 4 * _rel(spec, plain) + 2.0 ** -23)
            assert not taps[s][b, n:].any()
    assert ok
    ref = f32.forward(waves)
    assert np.array_equal(_u32(m.tap(0)), _u32(f32.tap(0)))                                        # the stem is untouched
    _gate("probabilities, bf16 mode to f32 mode, max abs", float(np.abs(probs - ref).max()), None)
    s = mas.SortformerModel.synthetic(cfg, encoder_dtype="bfloat16")
    p = s.forward(waves)
    assert s.launches == _bf16_launches(cfg) and np.isfinite(p).all() and p.min() >= 0 and p.max() <= 1


def test_row_bits_do_not_depend_on_batch():
    cfg = _cfg(True)
    m = mas.SortformerModel.from_weights(cfg, R.synthetic_weights(cfg, 5, R.HEAD_GAIN), encoder_dtype="bfloat16")
    waves, stages = _waves(), range(1, 2 + 2 + 3)
    alone = m.forward(waves[:1])
    alone_taps = [m.tap(s) for s in stages]
    n = alone.shape[1]
    batch = m.forward(waves, junk=np.nan)
    assert np.array_equal(_u32(batch[0, :n]), _u32(alone[0])) and not batch[0, n:].any()
    assert all(np.array_equal(_u32(m.tap(s)[0, :n]), _u32(a[0])) for s, a in zip(stages, alone_taps))
    rng = np.random.default_rng(3)
    counts, d = [9, 33, 40], cfg.fc_encoder_config.hidden_size
    emb = np.full((3, 40, d), np.nan, np.float32)
    for b, c in enumerate(counts):
        emb[b, :c] = rng.standard_normal((c, d))
    both = m.encode_embeddings(emb, counts)
    assert m.launches == _bf16_launches(cfg, 5) == m.expected_launches["encode_embeddings"]
    for b, c in enumerate(counts):
        assert np.array_equal(_u32(m.encode_embeddings(emb[b:b + 1, :c])[0]), _u32(both[b, :c])) and not both[b, c:].any()


def test_streaming_runs_on_bf16():
    """Segments are not compared with f32 mode's: thresholded decisions near 0.5 may differ.  Without AOSC a step encodes [spkcache, fifo + chunk]
    and writes its probabilities back over both, so the state behind a step holds the call's input and output: a fresh call must repeat them."""
    cfg = _cfg(True)
    m = mas.SortformerModel.from_weights(cfg, R.synthetic_weights(cfg, 5, R.HEAD_GAIN), encoder_dtype="bfloat16")
    outs = list(m.generate_stream(R.test_wave(70, 16000 * 6), chunk_duration=0.64, spkcache_max=16, fifo_max=16))
    assert len(outs) >= 6
    for o in outs:
        s = o.state
        fresh = m.encode_embeddings(np.concatenate([s.spkcache, s.fifo], axis=1))
        assert np.array_equal(_u32(fresh), _u32(np.concatenate([s.spkcache_preds, s.fifo_preds], axis=1)))
        after = mas.maybe_compress_state(s, 16, 16, cfg.modules_config)
        assert (after.spkcache_len, after.fifo_len) == R.expected_lengths(s.spkcache_len, s.fifo_len, 16, 16, cfg.modules_config)
    assert outs[-1].state.frames_processed == sum(o.speaker_probs.shape[0] for o in outs)


def test_refusals_and_defaults():
    for field, over in (("hidden_size", dict(fc=dict(hidden_size=80))), ("intermediate_size", dict(fc=dict(intermediate_size=100))),
                        ("tf_d_model", dict(tf=dict(d_model=48, encoder_attention_heads=2))), ("encoder_ffn_dim", dict(tf=dict(encoder_ffn_dim=100))),
                        ("tf_d_model", dict(tf=dict(d_model=288))), ("encoder_ffn_dim", dict(tf=dict(encoder_ffn_dim=1056)))):
        raw = mas.SortformerModel(_cfg(True, **over))
        with pytest.raises(mas.AudioGenerationError, match=field):
            raw.set_encoder_dtype("bfloat16")
        raw.set_encoder_dtype("float32")                                   # the handle is still usable after the refusal
    with pytest.raises(mas.AudioGenerationError, match="encoder_dtype"):
        mas.SortformerModel.from_weights(_cfg(True), {}, encoder_dtype="float16")
    cfg = _cfg(False)
    assert cfg.encoder_dtype == "float32" and mas.SortformerConfig.from_dict({}, encoder_dtype="bfloat16").encoder_dtype == "bfloat16"
    m = mas.SortformerModel.from_weights(cfg, R.synthetic_weights(cfg, 5))
    with pytest.raises(mas.AudioGenerationError, match="after finalize"):
        m.set_encoder_dtype("bfloat16")
    m.forward(_waves()[:1])                                                # still usable, and still the f32 engine
    assert m.launches == 11 + 15 * 2 + 7 * 2 == m.expected_launches["forward"]
