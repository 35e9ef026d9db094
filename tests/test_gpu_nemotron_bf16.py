"""-m gpu: the bf16 form of the Nemotron ASR encoder (csrc/nemotron_encoder_bf16.h): its two kernels and the LN + SiLU operand load through
the debug entry points, and the chain through NemotronASR with encoder_dtype="bfloat16".  References are float64 torch with
.to(torch.bfloat16) at the contract's rounding points; the gate forms are test_gpu_parakeet_bf16.py's, derived there: a bf16 store is within
one rounding, (2^-8 + 2^-20) |ref| + 2^-126; a rounded operand 2 x rel(rounded reference, float64) + 2^-23; a block tap 4 x D_w + 2^-23 on
the device's own previous tap.  MIS_NEMOTRON_BF16_PARITY_LOG=<file> keeps every observed value (profiles/nemotron_bf16/parity_observed.jsonl)."""
import json
import os

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
from mlx_audio_swift_amd.generation import check
import nemotron_ref as N
import sortformer_ref as R
from test_gpu_parakeet_bf16 import ROWS, _bits, _ptr, _ragged, _rb, _rel, _rounded_matrices, _wide

pytestmark = pytest.mark.gpu
F64 = torch.float64
KEYS = (1, 13, 14, 15, 31, 33, 64, 65, 97, 230)
FRAMES = (1, 15, 17, 130)


def _gate(kind, value, tol):
    name = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].split("::")[-1]
    if os.environ.get("MIS_NEMOTRON_BF16_PARITY_LOG"):
        with open(os.environ["MIS_NEMOTRON_BF16_PARITY_LOG"], "a") as f:
            f.write(json.dumps(dict(test=name, kind=kind, value=float(value), tol=float(tol))) + "\n")
    print(f"{name} {kind}: {value:.3e} (tol {tol:.3e})")
    return value <= tol


def _attention_rounded(qkv, table, u, v, n, H, hd, Tcap, ctx):
    """the literal mask over the literal rel-shift scores in float64 with the contract's three roundings: q + u, q + v, the probabilities"""
    sp = lambda y: y.reshape(-1, H, hd).transpose(0, 1)
    q, k, val = (sp(qkv[:n, i * H * hd:(i + 1) * H * hd]) for i in range(3))
    idx = (torch.arange(n)[:, None] - torch.arange(n)[None, :] + Tcap - 1).expand(H, n, n)
    band = torch.gather(_rb(q + v[:, None]) @ sp(table).transpose(1, 2), 2, idx)                  # entry [i][j]: the row of distance i - j
    s = (_rb(q + u[:, None]) @ k.transpose(1, 2) + band) / hd ** 0.5 + torch.as_tensor(N.mask(n, *ctx))
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    return ((_rb(e) @ val) / e.sum(-1, keepdim=True)).transpose(0, 1).reshape(n, H * hd)


@pytest.mark.parametrize("ctx", [(56, 13), (4, 1), (0, 0), (-1, 3), (70, 0)])
@pytest.mark.parametrize("hd", [128, 72, 40])
def test_attention(hd, ctx):
    """one ragged launch, NaN behind every count AND in every table row outside the context's -(C - 1) .. L C + C - 1.  At (0, 0) a query
    sees itself alone: the output is V, bit for bit."""
    H, Tp, Tcap, B = 2, max(KEYS), 240, len(KEYS)
    g = torch.Generator().manual_seed(hd)
    w = H * hd
    qkv = torch.full((B, Tp, 3 * w), float("nan"), dtype=F64)
    for b, n in enumerate(KEYS):
        qkv[b, :n] = _rb(torch.randn(n, 3 * w, generator=g, dtype=F64))
    table = _rb(torch.randn(2 * Tcap - 1, w, generator=g, dtype=F64))
    Cs, L = N.context(*ctx)
    dev_table = torch.full_like(table, float("nan"))
    lo, hi = Tcap - 1 - (Cs - 1), Tcap - 1 + min(L * Cs + Cs - 1, Tcap - 1)
    dev_table[lo:hi + 1] = table[lo:hi + 1]
    u, v = ((torch.rand(H, hd, generator=g) - 0.5) for _ in range(2))
    qb, tb, un, vn, cnt = _bits(qkv), _bits(dev_table), u.numpy(), v.numpy(), np.asarray(KEYS, np.int32)
    out = np.zeros((B, Tp, w), np.uint16)
    check(mas._lib.lib().mis_debug_nemotron_attn_bf16(0, _ptr(qb), 3 * w, w, 2 * w, _ptr(cnt), B, Tp, H, hd, 1.0, float(np.sqrt(hd)), _ptr(un), _ptr(vn),
                                                      _ptr(tb), w, 2 * Tcap - 1, Tcap - 1, ctx[0], ctx[1], Tcap, w, _ptr(out), 0, None))
    dev, ok = _wide(out), True
    for b, n in enumerate(KEYS):
        r64 = torch.as_tensor(N.attention(qkv[b].numpy(), table.numpy(), un, vn, n, H, hd, Tcap, ctx, F64))
        rr = _rb(_attention_rounded(qkv[b], table, u.to(F64), v.to(F64), n, H, hd, Tcap, ctx))
        ok &= _gate(f"attn hd {hd} ctx {ctx} keys {n}", _rel(dev[b, :n], r64), 2 * _rel(rr, r64) + 2.0 ** -23)
        assert not out[b, n:].any()
        if ctx == (0, 0):
            assert np.array_equal(out[b, :n], qb[b, :n, 2 * w:])
    assert ok


@pytest.mark.parametrize("taps,pads", [(9, (8, 0)), (4, (3, 0)), (9, (5, 3))])
@pytest.mark.parametrize("C", [160, 72])
def test_glu_dwconv_ln(C, taps, pads):
    """Same-sign terms per channel (test_gpu_parakeet_bf16.test_glu_dwconv explains why): a = ta |.|, taps = ts ta |.|, bias = ts |.|.  The
    statistics are held as test_gpu_nemotron.py holds the f32 kernel's, applied to the float64 outputs: the device's (y - mean) rstd against
    float64 layer_norm(y) <= 4 x the float32 conv + layer_norm's own distance, + 2^-23."""
    g = torch.Generator().manual_seed(C + taps + pads[0])
    ta, ts = (torch.randint(0, 2, (C,), generator=g).to(F64) * 2 - 1 for _ in range(2))
    gated = lambda n, c: _rb(torch.cat([ta * torch.randn(n, C, generator=g, dtype=F64).abs(), torch.randn(n, C, generator=g, dtype=F64)], -1))
    B, Tp = len(FRAMES), max(FRAMES)
    pw = torch.full((B, Tp, 2 * C), float("nan"), dtype=F64)
    for b, n in enumerate(FRAMES):
        pw[b, :n] = gated(n, C)
    w = (ts * ta * torch.randn(taps, C, generator=g).abs() / taps ** 0.5).float().to(F64)
    bias = (0.1 * ts * torch.randn(C, generator=g).abs()).float().to(F64)
    pb, tn, bn, cnt = _bits(pw), w.float().numpy(), bias.float().numpy(), np.asarray(FRAMES, np.int32)
    out, st = np.zeros((B, Tp, C), np.uint16), np.zeros((B, Tp, 2), np.float32)
    check(mas._lib.lib().mis_debug_nemotron_dwconv_ln_bf16(0, _ptr(pb), _ptr(tn), _ptr(bn), _ptr(cnt), B, Tp, C, taps, pads[0], _ptr(out), _ptr(st)))
    dev, ok = _wide(out), True
    for b, n in enumerate(FRAMES):
        y = {}
        for dt in (F64, torch.float32):
            glu = torch.nn.functional.pad((pw[b, :n, :C].to(dt) * torch.sigmoid(pw[b, :n, C:].to(dt))).T[None], pads)
            y[dt] = torch.nn.functional.conv1d(glu, w.to(dt).T[:, None], bias.to(dt), groups=C)[0].T
        worst = float(((dev[b, :n] - y[F64]).abs() / ((2.0 ** -8 + 2.0 ** -20) * y[F64].abs() + 2.0 ** -126)).max())
        ok &= _gate(f"dwconv C {C} taps {taps} pads {pads} frames {n}: roundings", worst, 1.0)
        stats = torch.from_numpy(st[b, :n]).to(F64)
        own, own32 = (torch.nn.functional.layer_norm(y[dt], (C,), eps=1e-5) for dt in (F64, torch.float32))
        ok &= _gate(f"ln stats C {C} taps {taps} frames {n}", _rel((y[F64] - stats[:, :1]) * stats[:, 1:], own), 4 * _rel(own32, own) + 2.0 ** -23)
        assert not out[b, n:].any() and not st[b, n:].any()
    assert ok


@pytest.mark.parametrize("N_,K", [(8, 32), (72, 96), (160, 640)])
def test_ln_silu_load(N_, K):
    """the "ln load" gate of test_gpu_parakeet_bf16.test_contraction with SiLU behind the LayerNorm, through PKB_EPI_RES"""
    g = torch.Generator().manual_seed(N_ * 1000 + K)
    normal = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    live = torch.zeros(len(ROWS), max(ROWS), N_, dtype=torch.bool)
    for b, n in enumerate(ROWS):
        live[b, :n] = True
    x = _ragged(lambda n, k: _rb(1.5 * normal(n, k) + 0.3), K)
    w, bias, res = _rb(normal(N_, K) / K ** 0.5), normal(N_).float().to(F64), _ragged(normal, N_).float().to(F64)
    lnw, lnb = (1 + 0.1 * normal(K)).float().to(F64), (0.05 * normal(K)).float().to(F64)
    stats = torch.stack([x.mean(-1), 1 / torch.sqrt(x.var(-1, unbiased=False) + 1e-5)], -1).float().to(F64)
    act = torch.nn.functional.silu((x - stats[..., :1]) * stats[..., 1:] * lnw + lnb)
    f32 = lambda t: np.ascontiguousarray(t.to(torch.float32).numpy())
    keep = [_bits(x), f32(stats), f32(lnw), f32(lnb), _bits(w), f32(bias), f32(res), np.asarray(ROWS, np.int32)]
    out = np.zeros((len(ROWS), max(ROWS), N_), np.float32)
    check(mas._lib.lib().mis_debug_nemotron_gemm_bf16(0, 2, 2, 0, *(_ptr(a) for a in keep[:7]), 1.0, _ptr(keep[7]), len(ROWS), max(ROWS), K, N_, _ptr(out),
                                                      0, None))
    dev = torch.from_numpy(out).to(F64)
    exact, rounded = (res + act @ w.T + bias)[live], (res + _rb(act) @ w.T + bias)[live]
    assert _gate("ln silu load", _rel(dev[live], exact), 2 * _rel(rounded, exact) + 2.0 ** -23)
    assert not out[~live.numpy()].any()


def _waves():
    return [R.test_wave(40 + i, int(16000 * s) + 37 * i) for i, s in enumerate((0.3, 1.0, 2.5))]


@pytest.mark.parametrize("hidden", [256, 160])
def test_chain(hidden):
    cfg = N.case_config(hidden)
    W, waves, L = N.make_weights(cfg, 21), _waves(), cfg.num_hidden_layers
    m, f32 = mas.NemotronASR.from_weights(cfg, W, encoder_dtype="bfloat16"), mas.NemotronASR.from_weights(cfg, W)
    f32.decode_raw(waves)
    _, T = m.frames([len(w) for w in waves])
    ok = True
    for ctx in (None, (4, 1)):                                             # the default (56, 13), then the other listed context, per call
        used = ctx or cfg.default_context
        m.decode_raw(waves, att_context_size=ctx)
        assert m.launches == f32.launches == m.expected_launches["generate"]
        taps = [m.tap(s) for s in range(L + 1)]
        assert np.array_equal(taps[0].view(np.uint32), f32.tap(0).view(np.uint32))                # the stem is untouched
        # a block tap against the float64 specification holding the bf16-rounded matrices, on the device's own previous tap: <= 4 x D_w +
        # 2^-23, D_w that specification's distance to the float64 one with unrounded matrices (test_gpu_parakeet_bf16._block_taps_gate)
        exact, rounded = N.Encoder(cfg, W, F64, used), N.Encoder(cfg, _rounded_matrices(W, L), F64, used)
        for b in range(len(waves)):
            n = int(T[b])
            for s in range(1, L + 1):
                spec, plain = rounded.stage_after(s, taps[s - 1][b, :n]), exact.stage_after(s, taps[s - 1][b, :n])
                ok &= _gate(f"ctx {used} row {b} stage {s}", _rel(taps[s][b, :n], spec), 4 * _rel(spec, plain) + 2.0 ** -23)
                assert not taps[s][b, n:].any()
    assert ok
    batch = m.decode_raw(waves)
    enc, _ = m.encode(waves)
    junk, _ = m.encode(waves, junk=np.nan)
    assert np.array_equal(enc.view(np.uint32), junk.view(np.uint32))
    for b, w in enumerate(waves):                                          # a row alone: the same bits, the same decode
        alone, _ = m.encode([w])
        assert np.array_equal(alone[0].view(np.uint32), enc[b, :alone.shape[1]].view(np.uint32))
        one = m.decode_raw([w])[0]
        assert all(np.array_equal(one[k], batch[b][k]) for k in ("tokens", "frames"))


def test_refusals():
    with pytest.raises(mas.AudioGenerationError, match="hidden_size"):
        mas.NemotronASR.from_weights(N.case_config(144), {}, encoder_dtype="bfloat16")
    with pytest.raises(mas.AudioGenerationError, match="encoder_dtype"):
        mas.NemotronASR.from_weights(N.case_config(256), {}, encoder_dtype="float16")
    cfg = N.case_config(256)
    W = N.make_weights(cfg, 21)
    m = mas.NemotronASR.from_weights(cfg, W)
    with pytest.raises(mas.AudioGenerationError, match="after finalize"):
        m.set_encoder_dtype("bfloat16")
    out = m.decode_raw([_waves()[0]])                                      # still usable, and still the f32 engine
    assert len(out) == 1 and m.launches == m.expected_launches["generate"]
    m.make_stream_session(att_context_size=(4, 1)).close()
    with pytest.raises(mas.AudioGenerationError, match="encoder_dtype"):
        mas.NemotronASR.from_weights(cfg, W, encoder_dtype="bfloat16").make_stream_session(att_context_size=(4, 1))
