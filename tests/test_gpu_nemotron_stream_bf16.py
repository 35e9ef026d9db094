"""-m gpu: the bf16 Nemotron stream session (csrc/nemotron_stream_bf16.h): its three kernels through the debug entry points and the chain through
NemotronStreamSession(encoder_dtype="bfloat16").  The yardstick is the offline bf16 engine of the same model, bit for bit; the float64 gates
are the ones derived in test_gpu_parakeet_bf16.py: a rounded operand 2 x rel(rounded float64 reference, float64) + 2^-23, a bf16 store one
rounding, an f32 store of unrounded operands 4 x the float32 reference's own distance + 2^-23.
MIS_NEMOTRON_STREAM_BF16_PARITY_LOG=<file> keeps every observed value (profiles/nemotron_stream_bf16/parity_observed.jsonl)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
from mlx_audio_swift_amd.generation import check
import nemotron_ref as N
from test_gpu_nemotron_bf16 import _attention_rounded
from test_gpu_nemotron_stream import CONTEXTS, LANGS, _feeds, _run, _waves, bits
from test_gpu_parakeet_bf16 import ROWS, _bits, _ptr, _rb, _rel, _wide

pytestmark = pytest.mark.gpu
F64 = torch.float64
NAN16 = 0x7FC0


def _gate(kind, value, tol):
    name = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].split("::")[-1]
    if os.environ.get("MIS_NEMOTRON_STREAM_BF16_PARITY_LOG"):
        with open(os.environ["MIS_NEMOTRON_STREAM_BF16_PARITY_LOG"], "a") as f:
            f.write(json.dumps(dict(test=name, kind=kind, value=float(value), tol=float(tol))) + "\n")
    print(f"{name} {kind}: {value:.3e} (tol {tol:.3e})")
    return value <= tol


@pytest.mark.parametrize("rows", [ROWS, (1,) * 64], ids=["ragged", "64x1"])
@pytest.mark.parametrize("load,epi", [(1, 1), (1, 0), (0, 2), (2, 2)])
@pytest.mark.parametrize("N_,K", [(8, 32), (72, 96), (160, 640)])
def test_contraction(N_, K, load, epi, rows):
    """the short-pass rules 2 / 3 / 4 (64 / 32 / 16 columns a block) on rows compacted across batch entries (a 16-row tile ends mid-entry),
    NaN behind every count: the live rows equal the 64 x 64 rule's bits, the rows behind a count stay unwritten.  Every load is held to the
    "rounded operand" gate; load 0 rounds nothing (x and w are bf16 values), so its rounded reference is the float64 one and the gate is
    2^-23 on the f32 accumulation alone."""
    g = torch.Generator().manual_seed(N_ * 1000 + K + load)
    normal = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    B, Tp = len(rows), max(rows) + 1
    live = torch.zeros(B, Tp, dtype=torch.bool)
    for b, n in enumerate(rows):
        live[b, :n] = True
    nanfill = lambda t: torch.where(live[..., None], t, torch.full_like(t, float("nan")))
    x = nanfill(1.5 * normal(B, Tp, K) + 0.3)
    x = x.float().to(F64) if load == 1 else _rb(x)
    w, bias, res = _rb(normal(N_, K) / K ** 0.5), normal(N_).float().to(F64), nanfill(normal(B, Tp, N_)).float().to(F64)
    lnw, lnb = (1 + 0.1 * normal(K)).float().to(F64), (0.05 * normal(K)).float().to(F64)
    xl = torch.where(live[..., None], x, torch.zeros_like(x))
    stats = nanfill(torch.stack([xl.mean(-1), 1 / torch.sqrt(xl.var(-1, unbiased=False) + 1e-5)], -1)).float().to(F64)
    ln = (x - stats[..., :1]) * stats[..., 1:] * lnw + lnb
    op = {0: x, 1: ln, 2: torch.nn.functional.silu(ln)}[load][live]
    f32 = lambda t: np.ascontiguousarray(t.to(torch.float32).numpy())
    keep = [f32(x) if load == 1 else _bits(x), f32(stats), f32(lnw), f32(lnb), _bits(w), f32(bias), f32(res), np.asarray(rows, np.int32)]

    def run(rule):
        out = np.zeros((B, Tp, N_), np.float32 if epi == 2 else np.uint16)
        check(mas._lib.lib().mis_debug_nemotron_gemm_bf16(0, load, epi, rule, *(_ptr(a) for a in keep[:7]), 0.5, _ptr(keep[7]), B, Tp, K, N_, _ptr(out), 0, None))
        return out

    tile64, short = run(0), run(2)
    for rule in (2, 3, 4):
        got = short if rule == 2 else run(rule)
        assert np.array_equal(got[live.numpy()], tile64[live.numpy()]), f"rule {rule} differs from the 64 x 64 rule"
        assert (got[~live.numpy()].view(np.uint8) == 0xFF).all(), f"rule {rule} wrote behind a count"
    dev = (torch.from_numpy(short).to(F64) if epi == 2 else _wide(short))[live]
    post = (lambda v: res[live] + 0.5 * v) if epi == 2 else (lambda v: _rb(torch.nn.functional.silu(v) if epi == 1 else v))
    exact = (lambda v: res[live] + 0.5 * v) if epi == 2 else (torch.nn.functional.silu if epi == 1 else (lambda v: v))
    r64, rr = exact(op @ w.T + bias), post(_rb(op) @ w.T + bias)
    if load == 0:                                                          # logged beside the gate, not asserted: the sibling's f32-store form
        r32 = (res[live].float() + 0.5 * (op.float() @ w.float().T + bias.float())).to(F64)
        _gate("rows load 0 epi 2 against 4 x the float32 reference", _rel(dev, r64), 4 * _rel(r32, r64) + 2.0 ** -23)
    assert _gate(f"rows load {load} epi {epi}", _rel(dev, r64), 2 * _rel(rr, r64) + 2.0 ** -23)


@pytest.mark.parametrize("ctx", [(56, 13), (4, 1), (0, 0), (70, 0)])
@pytest.mark.parametrize("hd", [128, 72, 40])
def test_attention(hd, ctx):
    """four streams behind two and more wraps of the smallest legal ring: a single query, a chunk, a full pass whose queries straddle a
    32-key tile boundary (every query in front of it walks a wholly hidden tile, every query behind it starts on one) and a full pass that
    straddles the wrap.  NaN in every ring row in front of the first visible key and in every table row outside the context.  Passes of
    5 and 8 frames launch 16 queries a block, 44 frames 32."""
    H, w, (left, right) = 2, 2 * hd, ctx
    Cs, L = right + 1, left // (right + 1)
    Tp = 3 * Cs + 2
    Rr = (left + Tp + 32 + 31) // 32 * 32
    sizes = [1, Cs, Tp, Tp]
    pos = [2 * Rr + 5, (3 * Rr + Cs) // Cs * Cs, 2 * Rr - 1, (4 * Rr - Tp // 2) // Cs * Cs]
    Tcap, S = max(p + n for p, n in zip(pos, sizes)), len(sizes)
    g = torch.Generator().manual_seed(hd + right)
    table = _rb(torch.randn(2 * Tcap - 1, w, generator=g, dtype=F64))
    dev_table = torch.full_like(table, float("nan"))
    lo, hi = Tcap - 1 - (Cs - 1), Tcap - 1 + L * Cs + Cs - 1
    dev_table[lo:hi + 1] = table[lo:hi + 1]
    u, v = ((torch.rand(H, hd, generator=g) - 0.5) for _ in range(2))
    full = torch.full((S, Tcap, 3 * w), float("nan"), dtype=F64)
    for b, (p, n) in enumerate(zip(pos, sizes)):
        full[b, :p + n] = _rb(torch.randn(p + n, 3 * w, generator=g, dtype=F64))
    fb, tb, un, vn = _bits(full), _bits(dev_table), u.numpy(), v.numpy()
    q, ring = np.full((S, Tp, w), NAN16, np.uint16), np.full((S, Rr, 2 * w), NAN16, np.uint16)
    for b, (p, n) in enumerate(zip(pos, sizes)):
        q[b, :n] = fb[b, p:p + n, :w]
        for key in range(max(p // Cs - L, 0) * Cs, p + n):
            ring[b, key % Rr] = fb[b, key, w:]
    cnt, ends, at = (np.asarray(a, np.int32) for a in (sizes, [p + n for p, n in zip(pos, sizes)], pos))
    out, off = np.zeros((S, Tp, w), np.uint16), np.zeros((S, Tcap, w), np.uint16)
    lib, sdk = mas._lib.lib(), float(np.sqrt(hd))
    check(lib.mis_debug_nemotron_attn_stream_bf16(0, _ptr(q), _ptr(ring), Rr, _ptr(cnt), _ptr(at), S, Tp, H, hd, 1.0, sdk, _ptr(un), _ptr(vn), _ptr(tb), w,
                                                  2 * Tcap - 1, Tcap - 1, left, right, _ptr(out), 0, None))
    check(lib.mis_debug_nemotron_attn_bf16(0, _ptr(fb), 3 * w, w, 2 * w, _ptr(ends), S, Tcap, H, hd, 1.0, sdk, _ptr(un), _ptr(vn), _ptr(tb), w, 2 * Tcap - 1,
                                           Tcap - 1, left, right, Tcap, w, _ptr(off), 0, None))
    dev, ok = _wide(out), True
    for b, (p, n) in enumerate(zip(pos, sizes)):
        assert np.array_equal(out[b, :n], off[b, p:p + n]), f"stream {b} differs from the offline kernel"
        assert not out[b, n:].any()
        r64 = torch.as_tensor(N.attention(full[b].numpy(), table.numpy(), un, vn, p + n, H, hd, Tcap, ctx, F64))[p:]
        rr = _rb(_attention_rounded(full[b], table, u.to(F64), v.to(F64), p + n, H, hd, Tcap, ctx))[p:]
        ok &= _gate(f"attn stream hd {hd} ctx {ctx} pos {p} frames {n}", _rel(dev[b, :n], r64), 2 * _rel(rr, r64) + 2.0 ** -23)
        if ctx == (0, 0):
            assert np.array_equal(out[b, :n], fb[b, p:p + n, 2 * w:])
    assert ok


@pytest.mark.parametrize("taps", [9, 4])
@pytest.mark.parametrize("C_", [160, 72])
def test_conv_module_carries_its_history(C_, taps):
    """two rows of 130 frames cut as (1, 15, 17, 97) and as (97, 17, 15, 1), history out -> history in from zeros: outputs, statistics and
    the carried rows equal the offline kernel's on the whole rows.  The first cut is also one rounding from the float64 conv (same-sign
    terms per channel, as test_gpu_nemotron_bf16.test_glu_dwconv_ln explains)."""
    g = torch.Generator().manual_seed(C_ + taps)
    ta, ts = (torch.randint(0, 2, (C_,), generator=g).to(F64) * 2 - 1 for _ in range(2))
    T, cuts, lib = 130, (1, 15, 17, 97), mas._lib.lib()
    pw = _rb(torch.cat([ta * torch.randn(2, T, C_, generator=g, dtype=F64).abs(), torch.randn(2, T, C_, generator=g, dtype=F64)], -1))
    wt = (ts * ta * torch.randn(taps, C_, generator=g).abs() / taps ** 0.5).float()
    bias = (0.1 * ts * torch.randn(C_, generator=g).abs()).float()
    pb, tn, bn = _bits(pw), wt.numpy(), bias.numpy()
    whole, wst = np.zeros((2, T, C_), np.uint16), np.zeros((2, T, 2), np.float32)
    check(lib.mis_debug_nemotron_dwconv_ln_bf16(0, _ptr(pb), _ptr(tn), _ptr(bn), _ptr(np.asarray([T, T], np.int32)), 2, T, C_, taps, taps - 1, _ptr(whole), _ptr(wst)))
    hist, at, Tp = np.zeros((2, taps - 1, 2 * C_), np.uint16), [0, 0], max(cuts)
    for i, pair in enumerate(zip(cuts, cuts[::-1])):
        x = np.full((2, Tp, 2 * C_), NAN16, np.uint16)
        for b, n in enumerate(pair):
            x[b, :n] = pb[b, at[b]:at[b] + n]
        nxt, out, st = np.zeros_like(hist), np.zeros((2, Tp, C_), np.uint16), np.zeros((2, Tp, 2), np.float32)
        check(lib.mis_debug_nemotron_dwconv_ln_stream_bf16(0, _ptr(x), _ptr(tn), _ptr(bn), _ptr(np.asarray(pair, np.int32)), 2, Tp, C_, taps, taps - 1, _ptr(hist),
                                                           _ptr(nxt), _ptr(out), _ptr(st)))
        for b, n in enumerate(pair):
            assert np.array_equal(out[b, :n], whole[b, at[b]:at[b] + n]) and np.array_equal(bits(st[b, :n]), bits(wst[b, at[b]:at[b] + n])), (i, b)
            assert not out[b, n:].any() and not st[b, n:].any()
            at[b] += n
            assert np.array_equal(nxt[b, max(taps - 1 - at[b], 0):], pb[b, max(at[b] - taps + 1, 0):at[b]])
            if i == 0:
                glu = torch.nn.functional.pad((pw[b, :n, :C_] * torch.sigmoid(pw[b, :n, C_:])).T[None], (taps - 1, 0))
                y = torch.nn.functional.conv1d(glu, wt.to(F64).T[:, None], bias.to(F64), groups=C_)[0].T
                worst = float(((_wide(out[b, :n]) - y).abs() / ((2.0 ** -8 + 2.0 ** -20) * y.abs() + 2.0 ** -126)).max())
                assert _gate(f"stream dwconv C {C_} taps {taps} first cut of {n}", worst, 1.0)
        hist = nxt


@functools.lru_cache(maxsize=None)
def _model(hidden):
    cfg = N.case_config(hidden, bias=hidden == 256, contexts=CONTEXTS, max_seconds=12)
    return cfg, mas.NemotronASR.from_weights(cfg, N.make_weights(cfg, 31), encoder_dtype="bfloat16")


@functools.lru_cache(maxsize=None)
def _offline(hidden, ctx):
    cfg, m = _model(hidden)
    raw = m.decode_raw(list(_waves()), LANGS, ctx)
    return raw, [m.tap(s) for s in range(cfg.num_hidden_layers + 3)], m.frames([len(w) for w in _waves()])[1]


@pytest.mark.parametrize("pattern", ["80ms", "ragged", "whole"])
@pytest.mark.parametrize("ctx", CONTEXTS)
@pytest.mark.parametrize("hidden", [256, 192])
def test_stream_equals_offline_bf16(hidden, ctx, pattern):
    """one bf16 model serves the bf16 session and the offline engine: every tap, the tokens and the frames; _run holds every feed's launches
    to passes x (9 + 16 L + 2 p)"""
    cfg, m = _model(hidden)
    L = cfg.num_hidden_layers
    raw, taps, T = _offline(hidden, ctx)
    sess = mas.NemotronStreamSession(m, 4, LANGS, att_context_size=ctx, max_pass_frames=None if pattern == "whole" else ctx[1] + 1, encoder_dtype="bfloat16")
    sess.enable_taps(int(T.max()) + 2)
    got = _run(sess, _feeds(pattern, _waves()), L + 3)
    for b in range(4):
        n = int(T[b])
        for s in range(L + 3):
            assert got[s][b].shape[0] == n and np.array_equal(bits(got[s][b]), bits(taps[s][b, :n])), f"stream {b} stage {s} differs from offline"
        mine = sess.raw(b)
        assert mine["tokens"].tolist() == raw[b]["tokens"].tolist() and mine["frames"].tolist() == raw[b]["frames"].tolist()
    sess.close()


def test_a_pass_of_many_rows_takes_the_64x64_rule():
    """24 streams of 25 frames in one pass are 38 tiles of 16 rows against 24 of 64: the pass goes through k_pk_gemm_bf16, and the bits stay"""
    cfg, m = _model(256)
    raw, taps, T = _offline(256, (56, 13))
    n, L = int(T[1]), cfg.num_hidden_layers
    sess = mas.NemotronStreamSession(m, 24, LANGS[1], att_context_size=(56, 13), encoder_dtype="bfloat16")
    sess.enable_taps(n + 2)
    sess.step_batch([_waves()[1]] * 24, [True] * 24)
    assert sess.launches == sess.expected_launches == sess.expected_launches_per_pass
    for s in range(L + 3):
        got = sess.tap(s)
        assert all(np.array_equal(bits(got[b]), bits(taps[s][1, :n])) for b in (0, 23)), f"stage {s} differs from offline"
    assert sess.raw(23)["tokens"].tolist() == raw[1]["tokens"].tolist()
    sess.close()


def _utterance(sess, slot, w, other=None, reset_at=None):
    """w through `slot` in feeds of 4000 samples (the other slots busy with `other`, slot 0 reset behind feed reset_at) -> tokens, taps L, L + 2"""
    L, taps = sess.model.config.num_hidden_layers, [[], []]
    for i, at in enumerate(list(range(0, len(w), 4000)) + [None]):
        chunks = [None if at is None or other is None else other[at:at + 4000]] * sess.streams
        chunks[slot] = None if at is None else w[at:at + 4000]
        sess.step_batch(chunks, [at is None and b == slot for b in range(sess.streams)])
        assert sess.launches == sess.expected_launches
        for k, stage in enumerate((L, L + 2)):
            taps[k].append(sess.tap(stage)[slot])
        if reset_at == i:
            sess.reset(0)
    return sess.raw(slot)["tokens"].tolist(), [np.concatenate(t) for t in taps]


def test_slots_and_refusals():
    cfg, m = _model(256)
    w, other = _waves()[1], _waves()[0][:40000]
    one = mas.NemotronStreamSession(m, 1, "de-DE", att_context_size=(4, 1), encoder_dtype="bfloat16")
    four = mas.NemotronStreamSession(m, 4, ["en-US", "en-US", "auto", "de-DE"], att_context_size=(4, 1), encoder_dtype="bfloat16")
    for s in (one, four):
        s.enable_taps(64)
    alone, busy = _utterance(one, 0, w), _utterance(four, 3, w, other, reset_at=2)
    assert len(alone[0]) > 0 and busy[0] == alone[0] and all(np.array_equal(bits(a), bits(b)) for a, b in zip(busy[1], alone[1]))
    one.close(); four.close()
    with pytest.raises(mas.AudioGenerationError, match="encoder_dtype"):
        m.make_stream_session(att_context_size=(4, 1))                         # the default session on a bf16 model
    f32 = mas.NemotronASR.from_weights(cfg, N.make_weights(cfg, 31))
    with pytest.raises(mas.AudioGenerationError, match="encoder_dtype"):
        f32.make_stream_session(att_context_size=(4, 1), encoder_dtype="bfloat16")
    old, new = (mas.NemotronStreamSession(f32, 1, "de-DE", att_context_size=(4, 1)) for _ in range(2))
    mas._lib.lib().mis_nemotron_stream_destroy(new._h)                       # the same f32 session, made by the new entry point
    check(mas._lib.lib().mis_nemotron_stream_create_dtype(f32._h, 1, 4, 1, 6, mas._lib.MIS_F32, C.byref(new._h)))
    new.reset(0, "de-DE")
    for s in (old, new):
        s.enable_taps(64)
    a, b = _utterance(old, 0, w), _utterance(new, 0, w)
    assert a[0] == b[0] and len(a[0]) > 0 and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a[1], b[1]))
    old.close(); new.close(); f32.close()
