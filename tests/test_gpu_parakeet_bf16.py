"""-m gpu: the bf16 form of the Parakeet / Canary encoder (csrc/parakeet_encoder_bf16.h): its three kernels through the debug entry points
and the chain through ParakeetModel / CanaryModel with encoder_dtype="bfloat16".  References are float64 torch with .to(torch.bfloat16)
at the contract's rounding points.  Distances are relative rms, as in test_gpu_parakeet.py; the reasoning of each gate stands at the gate.
MIS_PARAKEET_BF16_PARITY_LOG=<file> keeps every observed value (profiles/parakeet_bf16/parity_observed.jsonl)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
from mlx_audio_swift_amd.generation import check
import canary_ref as CR
import parakeet_ref as P
import sortformer_ref as R

pytestmark = pytest.mark.gpu
F64, BF = torch.float64, torch.bfloat16
ROWS = (1, 63, 65, 130)
KEYS = (1, 15, 17, 31, 33, 64, 65, 97)
BLOCK_MATRICES = ("feed_forward1.linear1", "feed_forward1.linear2", "feed_forward2.linear1", "feed_forward2.linear2", "self_attn.q_proj",
                  "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "conv.pointwise_conv1", "conv.pointwise_conv2")


def _ptr(a):
    return a.ctypes.data


def _rb(t):
    return t.to(BF).to(F64)


def _bits(t):
    """float tensor of bf16-representable values -> its bf16 bits (numpy uint16)"""
    return t.to(BF).contiguous().view(torch.int16).numpy().view(np.uint16)


def _wide(bits):
    return torch.from_numpy(bits.view(np.int16).copy()).view(BF).to(F64)


def _rel(a, b):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    return float(torch.sqrt(torch.mean((a - b) ** 2)) / max(float(torch.sqrt(torch.mean(b ** 2))), 1e-30))


def _gate(kind, value, tol):
    name = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].split("::")[-1]
    if os.environ.get("MIS_PARAKEET_BF16_PARITY_LOG"):
        with open(os.environ["MIS_PARAKEET_BF16_PARITY_LOG"], "a") as f:
            f.write(json.dumps(dict(test=name, kind=kind, value=float(value), tol=None if tol is None else float(tol))) + "\n")
    print(f"{name} {kind}: {value:.3e} (tol {tol if tol is None else format(tol, '.3e')})")
    return tol is None or value <= tol


def _within_one_rounding(kind, dev, ref64):
    """bf16 store: one rounding plus f32 accumulation -> every element within (2^-8 + 2^-20) |ref| + 2^-126 of the float64 value"""
    worst = float(((dev - ref64).abs() / ((2.0 ** -8 + 2.0 ** -20) * ref64.abs() + 2.0 ** -126)).max())
    return _gate(kind, worst, 1.0)


def _ragged(gen, width, fill=float("nan")):
    """[len(ROWS), max(ROWS), width]: gen(n, width) in a row's first n frames, `fill` behind them"""
    x = torch.full((len(ROWS), max(ROWS), width), fill, dtype=F64)
    for b, n in enumerate(ROWS):
        x[b, :n] = gen(n, width)
    return x


def _gemm(load, epi, rule, x, w, bias, cnt, stats=None, lnw=None, lnb=None, R_=None, ra=0.0):
    B, Tp, K = x.shape
    N = w.shape[0]
    f32 = lambda t: None if t is None else np.ascontiguousarray(t.to(torch.float32).numpy())
    xa = f32(x) if load == 1 else _bits(x)
    keep = [f32(stats), f32(lnw), f32(lnb), _bits(w), f32(bias), f32(R_), np.asarray(cnt, np.int32)]
    out = np.zeros((B, Tp, N), np.float32 if epi == 2 else np.uint16)
    p = lambda a: None if a is None else _ptr(a)
    check(mas._lib.lib().mis_debug_parakeet_gemm_bf16(0, load, epi, rule, _ptr(xa), p(keep[0]), p(keep[1]), p(keep[2]), _ptr(keep[3]), p(keep[4]), p(keep[5]), ra,
                                                      _ptr(keep[6]), B, Tp, K, N, _ptr(out), 0, None))
    return torch.from_numpy(out).to(F64) if epi == 2 else _wide(out)


@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("N,K", [(n, k) for n in (8, 72, 160) for k in (32, 96, 640)])
def test_contraction(N, K, rule):
    g = torch.Generator().manual_seed(N * 1000 + K)
    normal = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    grid = lambda *s: torch.randint(-8, 9, s, generator=g).to(F64) / 8        # products and sums of K of them are exact in f32
    ok, live = True, torch.zeros(len(ROWS), max(ROWS), 1, dtype=torch.bool)
    for b, n in enumerate(ROWS):
        live[b, :n] = True
    # f32 store (bias + residual): the only device error is f32 accumulation -> <= 4 x the float32 reference's own distance, + 2^-23
    x, w, bias, res = _ragged(lambda n, k: _rb(normal(n, k)), K), _rb(normal(N, K) / K ** 0.5), normal(N).float().to(F64), _ragged(normal, N).float().to(F64)
    for ra in (0.5, 1.0):
        dev = _gemm(0, 2, rule, x, w, bias, ROWS, R_=res, ra=ra)
        r64 = res + ra * (x @ w.T + bias)
        r32 = (res.float() + ra * (x.float() @ w.float().T + bias.float())).to(F64)
        ok &= _gate(f"res ra {ra}", _rel(dev[live.expand_as(dev)], r64[live.expand_as(dev)]), 4 * _rel(r32[live.expand_as(dev)], r64[live.expand_as(dev)]) + 2.0 ** -23)
        assert not dev[~live.expand_as(dev)].any()
    # LayerNorm load of arbitrary f32 x: the device rounds the same LN(x) from f32, a flipped tie moves an error from -d to +d
    xf = _ragged(lambda n, k: 1.5 * normal(n, k) + 0.3, K).float().to(F64)
    lnw, lnb = (1 + 0.1 * normal(K)).float().to(F64), (0.05 * normal(K)).float().to(F64)
    stats = torch.stack([xf.mean(-1), 1 / torch.sqrt(xf.var(-1, unbiased=False) + 1e-5)], -1).float().to(F64)
    ln = (xf - stats[..., :1]) * stats[..., 1:] * lnw + lnb
    dev = _gemm(1, 0, rule, xf, w, bias, ROWS, stats=stats, lnw=lnw, lnb=lnb)
    exact, rounded = (ln @ w.T + bias)[live.expand_as(dev)], _rb(_rb(ln) @ w.T + bias)[live.expand_as(dev)]
    ok &= _gate("ln load", _rel(dev[live.expand_as(dev)], exact), 2 * _rel(rounded, exact) + 2.0 ** -23)
    assert not dev[~live.expand_as(dev)].any()
    # bf16 stores
    x, w, bias = _ragged(grid, K), grid(N, K), grid(N) / 8
    for epi, act in ((0, lambda v: v), (1, torch.nn.functional.silu)):
        dev = _gemm(0, epi, rule, x, w, bias, ROWS)
        ok &= _within_one_rounding(f"bf16 store epi {epi}", dev[live.expand_as(dev)], act(x @ w.T + bias)[live.expand_as(dev)])
        assert not dev[~live.expand_as(dev)].any()
    assert ok


def _attention_rounded(qkv, table, u, v, n, H, hd, Tcap):
    """the literal rel-shift in float64 with the contract's three roundings: q + u, q + v, the probabilities in front of P V"""
    sp = lambda y: y.reshape(n, H, hd).transpose(0, 1)
    q, k, val = (sp(qkv[:n, i * H * hd:(i + 1) * H * hd]) for i in range(3))
    idx = torch.arange(n)[:, None] - torch.arange(n)[None, :] + Tcap - 1                          # distance i - j
    s = (_rb(q + u[:, None]) @ k.transpose(1, 2) + torch.einsum("hid,ijhd->hij", _rb(q + v[:, None]), table[idx].reshape(n, n, H, hd))) / hd ** 0.5
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    return ((_rb(e) @ val) / e.sum(-1, keepdim=True)).transpose(0, 1).reshape(n, H * hd)


@pytest.mark.parametrize("hd", [128, 80, 40])
def test_attention(hd):
    H, Tp, Tcap, B = 2, max(KEYS), 100, len(KEYS)
    g = torch.Generator().manual_seed(hd)
    w = H * hd
    qkv = torch.full((B, Tp, 3 * w), float("nan"), dtype=F64)
    for b, n in enumerate(KEYS):
        qkv[b, :n] = _rb(torch.randn(n, 3 * w, generator=g, dtype=F64))
    table = _rb(torch.randn(2 * Tcap - 1, w, generator=g, dtype=F64))
    u, v = ((torch.rand(H, hd, generator=g) - 0.5) for _ in range(2))
    qb, tb, un, vn, cnt = _bits(qkv), _bits(table), u.numpy(), v.numpy(), np.asarray(KEYS, np.int32)
    out = np.zeros((B, Tp, w), np.uint16)
    check(mas._lib.lib().mis_debug_parakeet_attn_bf16(0, _ptr(qb), 3 * w, w, 2 * w, _ptr(cnt), B, Tp, H, hd, 1.0, float(np.sqrt(hd)), _ptr(un), _ptr(vn),
                                                      _ptr(tb), w, Tcap, w, _ptr(out), 0, None))
    dev, ok = _wide(out), True
    for b, n in enumerate(KEYS):
        r64 = torch.as_tensor(P.attention(qkv[b].numpy(), table.numpy(), un, vn, n, H, hd, Tcap, F64))
        rr = _rb(_attention_rounded(qkv[b], table, u.to(F64), v.to(F64), n, H, hd, Tcap))
        ok &= _gate(f"attn hd {hd} keys {n}", _rel(dev[b, :n], r64), 2 * _rel(rr, r64) + 2.0 ** -23)
        _gate(f"attn hd {hd} keys {n} to the rounded reference", _rel(dev[b, :n], rr), None)
        assert not dev[b, n:].any()
    assert ok


@pytest.mark.parametrize("k", [3, 9, 31])
@pytest.mark.parametrize("C", [72, 160])
def test_glu_dwconv(C, k):
    """The bound leaves 2^-20 for the f32 arithmetic, which a sum that cancels to nearly nothing does not keep relative to its result (with
    freely signed terms the worst element of these cases was 7.2 x the bound, at an output 1e-5 of its terms).  So every channel's terms
    share one sign: a = ta |.|, taps = ts ta |.|, shift = ts |.| with per-channel signs ta, ts - negative inputs, taps and outputs all occur."""
    g = torch.Generator().manual_seed(C + k)
    ta, ts = (torch.randint(0, 2, (C,), generator=g).to(F64) * 2 - 1 for _ in range(2))
    gated = lambda n, c: _rb(torch.cat([ta * torch.randn(n, C, generator=g, dtype=F64).abs(), torch.randn(n, C, generator=g, dtype=F64)], -1))
    pw = _ragged(gated, 2 * C)
    taps = (ts * ta * torch.randn(k, C, generator=g).abs() / k ** 0.5).to(F64)
    shift = (0.1 * ts * torch.randn(C, generator=g).abs()).to(F64)
    pb, tn, sn, cnt = _bits(pw), taps.float().numpy(), shift.float().numpy(), np.asarray(ROWS, np.int32)
    out = np.zeros((len(ROWS), max(ROWS), C), np.uint16)
    check(mas._lib.lib().mis_debug_parakeet_glu_dwconv_bf16(0, _ptr(pb), _ptr(tn), _ptr(sn), _ptr(cnt), len(ROWS), max(ROWS), C, k, _ptr(out)))
    dev, ok = _wide(out), True
    for b, n in enumerate(ROWS):
        glu = pw[b, :n, :C] * torch.sigmoid(pw[b, :n, C:])
        conv = torch.nn.functional.conv1d(glu.T[None], taps.T[:, None], shift, padding=(k - 1) // 2, groups=C)[0].T
        ok &= _within_one_rounding(f"glu C {C} k {k} T {n}", dev[b, :n], torch.nn.functional.silu(conv))
        assert not dev[b, n:].any()
    assert ok


@functools.lru_cache(maxsize=None)
def _waves():
    return tuple(R.test_wave(40 + i, int(16000 * s) + 37 * i) for i, s in enumerate((0.3, 1.0, 2.5)))


def _rounded_matrices(W, layers):
    Wr = dict(W)
    for i in range(layers):
        for n in BLOCK_MATRICES:
            key = f"encoder.layers.{i}.{n}.weight"
            Wr[key] = torch.as_tensor(W[key]).to(BF).float().numpy()
    return Wr


def _block_taps_gate(m, view, W, L, T, taps):
    """every block tap against the float64 specification holding the bf16-rounded matrices, run on the device's own previous tap:
    <= 4 x D_w + 2^-23, D_w that specification's distance to the float64 one with unrounded matrices (rounding ONE operand of every
    contraction; the device also rounds the other operand and three things inside attention)"""
    exact, rounded, ok = P.Encoder(view, W, F64), P.Encoder(view, _rounded_matrices(W, L), F64), True
    for b in range(len(T)):
        n = int(T[b])
        for s in range(1, L + 1):
            spec, plain = rounded.stage_after(s, taps[s - 1][b, :n]), exact.stage_after(s, taps[s - 1][b, :n])
            ok &= _gate(f"row {b} stage {s}", _rel(taps[s][b, :n], spec), 4 * _rel(spec, plain) + 2.0 ** -23)
            assert not taps[s][b, n:].any()
    return ok


@pytest.mark.parametrize("hidden", [256, 160])
def test_chain(hidden):
    cfg = P.case_config(hidden)
    W, waves, L = P.make_weights(cfg, 21), list(_waves()), cfg.num_hidden_layers
    m, f32 = mas.ParakeetModel.from_weights(cfg, W, encoder_dtype="bfloat16"), mas.ParakeetModel.from_weights(cfg, W)
    batch = m.decode_raw(waves)
    assert m.launches == 9 + 15 * L == m.expected_launches["generate"]
    taps = [m.tap(s) for s in range(L + 1)]
    f32.decode_raw(waves)
    assert np.array_equal(taps[0].view(np.uint32), f32.tap(0).view(np.uint32))                    # the stem is untouched
    _, T = m.frames([len(w) for w in waves])
    assert _block_taps_gate(m, cfg, W, L, T, taps)
    enc, _ = m.encode(waves)
    junk, _ = m.encode(waves, junk=np.nan)
    assert np.array_equal(enc.view(np.uint32), junk.view(np.uint32))
    for b, w in enumerate(waves):                                          # a row alone: the same bits, the same decode
        alone, _ = m.encode([w])
        assert np.array_equal(alone[0].view(np.uint32), enc[b, :alone.shape[1]].view(np.uint32))
        one = m.decode_raw([w])[0]
        assert all(np.array_equal(one[k], batch[b][k]) for k in ("tokens", "frames", "durations"))


def test_canary_chain():
    cfg = CR.case_config(256, 4)
    W, waves, L = CR.make_weights(cfg, 31), list(_waves()), cfg.encoder.n_layers
    m = mas.CanaryModel.from_weights(cfg, W, encoder_dtype="bfloat16")
    enc, T = m.encode(waves)
    taps = [m.tap(s) for s in range(L + 1)]
    assert _block_taps_gate(m, CR.encoder_view(cfg), W, L, T, taps)
    junk, _ = m.encode(waves, junk=np.nan)
    assert np.array_equal(enc.view(np.uint32), junk.view(np.uint32))
    for b, w in enumerate(waves):
        alone, _ = m.encode([w])
        assert np.array_equal(alone[0].view(np.uint32), enc[b, :alone.shape[1]].view(np.uint32))


def test_refusals():
    with pytest.raises(mas.AudioGenerationError, match="hidden_size"):
        mas.ParakeetModel.from_weights(P.case_config(144), {}, encoder_dtype="bfloat16")
    with pytest.raises(mas.AudioGenerationError, match="encoder_dtype"):
        mas.ParakeetModel.from_weights(P.case_config(256), {}, encoder_dtype="float16")
    cfg = P.case_config(256)
    m = mas.ParakeetModel.from_weights(cfg, P.make_weights(cfg, 21))
    with pytest.raises(mas.AudioGenerationError, match="after finalize"):
        m.set_encoder_dtype("bfloat16")
    out = m.decode_raw([_waves()[0]])                                      # still usable, and still the f32 engine
    assert len(out) == 1 and m.launches == 9 + 15 * cfg.num_hidden_layers
    raw = mas.ParakeetModel(P.case_config(144))
    with pytest.raises(mas.AudioGenerationError, match="hidden_size"):
        raw.set_encoder_dtype("bfloat16")
    raw.set_encoder_dtype("float32")                                       # the handle is still usable after the refusal
