"""-m gpu: Nemotron ASR (csrc/nemotron.hip) through the C ABI against tests/nemotron_ref.py, which test_nemotron_cpu.py holds to a hand-written
mask table, torch.nn.LSTM and the band form.

Gate of the float comparisons (test_gpu_parakeet._gate's): relative rms distance of the device to the float64 specification <= 4 x the
float32 specification's own distance to the float64 one, + 2^-23.  Every stage is compared with the specification run on the device's own
previous stage.  Decisions are compared for equality, no row exempt: test_nemotron_cpu's two decision-margin tests hold the margin that allows it.
MIS_NEMOTRON_PARITY_LOG=<file> keeps every observed value (profiles/nemotron/parity_observed.jsonl)."""
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
import sortformer_ref as R
from gpu_util import observe, rms

pytestmark = pytest.mark.gpu
KEYS = (1, 13, 14, 15, 64, 65, 97, 230)
SECONDS = (0.3, 1.0, 2.5)
LANGUAGES = ["de-DE", "en-US", "de-DE"]


def _gate(kind, dev, ref64, ref32):
    rel = lambda a, b: rms(a, np.asarray(b, np.float64)) / max(float(np.sqrt(np.mean(np.asarray(b, np.float64) ** 2))), 1e-30)
    value, tol = rel(dev, ref64), 4.0 * rel(ref32, ref64) + 2.0 ** -23
    name = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].split("::")[-1]
    if os.environ.get("MIS_NEMOTRON_PARITY_LOG"):
        with open(os.environ["MIS_NEMOTRON_PARITY_LOG"], "a") as f:
            f.write(json.dumps(dict(test=name, kind=kind, value=float(value), tol=float(tol))) + "\n")
    print(f"{name} {kind}: {value:.3e} (tol {tol:.3e})")
    return observe(kind, value, tol)


def _ptr(a):
    return a.ctypes.data


def _t(a, dt):
    return torch.as_tensor(np.asarray(a, np.float32)).to(dt)


@pytest.mark.parametrize("ctx", [(56, 13), (4, 1), (0, 0), (-1, 3), (70, 0)])
@pytest.mark.parametrize("hd", [128, 72])
def test_attention_kernel_against_the_literal_mask(hd, ctx):
    """one ragged launch, NaN behind every count AND in every table row outside -(C - 1) .. L C + C - 1; 230 keys under (56, 13) skip whole
    leading key tiles, (4, 1) skips them from the second query tile on"""
    H, Tp, Tcap, B = 2, max(KEYS), 240, len(KEYS)
    rng = np.random.default_rng(hd)
    w = H * hd
    qkv = np.full((B, Tp, 3 * w), np.nan, np.float32)
    for b, n in enumerate(KEYS):
        qkv[b, :n] = rng.standard_normal((n, 3 * w)).astype(np.float32)
    table = rng.standard_normal((2 * Tcap - 1, w)).astype(np.float32)
    Cs, L = N.context(*ctx)
    dev_table = np.full_like(table, np.nan)
    lo, hi = Tcap - 1 - (Cs - 1), Tcap - 1 + min(L * Cs + Cs - 1, Tcap - 1)
    dev_table[lo:hi + 1] = table[lo:hi + 1]
    u, v = (rng.uniform(-0.5, 0.5, (H, hd)).astype(np.float32) for _ in range(2))
    cnt, out = np.asarray(KEYS, np.int32), np.zeros((B, Tp, w), np.float32)
    check(mas._lib.lib().mis_debug_nemotron_attn(0, _ptr(qkv), 3 * w, w, 2 * w, _ptr(cnt), B, Tp, H, hd, 1.0, float(np.sqrt(hd)), _ptr(u), _ptr(v),
                                                 _ptr(dev_table), w, 2 * Tcap - 1, Tcap - 1, ctx[0], ctx[1], Tcap, w, _ptr(out), 0, None))
    ok = True
    for b, n in enumerate(KEYS):
        r64, r32 = (N.attention(qkv[b], table, u, v, n, H, hd, Tcap, ctx, dt) for dt in (torch.float64, torch.float32))
        ok &= _gate(f"attn hd {hd} ctx {ctx} keys {n}", out[b, :n], r64, r32)
        assert not out[b, n:].any()
    assert ok


FRAMES = (1, 8, 63, 64, 65, 130)


@pytest.mark.parametrize("d", [256, 144])
@pytest.mark.parametrize("taps,pads", [(9, (8, 0)), (4, (3, 0)), (9, (5, 3))])
def test_conv_module_kernel_and_its_layer_norm_statistics(taps, pads, d):
    Tp, B = max(FRAMES), len(FRAMES)
    rng = np.random.default_rng(taps + d)
    pw = np.full((B, Tp, 2 * d), np.nan, np.float32)
    for b, n in enumerate(FRAMES):
        pw[b, :n] = rng.standard_normal((n, 2 * d)).astype(np.float32)
    w, bias = rng.uniform(-0.5, 0.5, (d, taps, 1)).astype(np.float32), rng.uniform(-0.05, 0.05, d).astype(np.float32)
    tk = np.ascontiguousarray(w[:, :, 0].T)
    cnt, out, st = np.asarray(FRAMES, np.int32), np.zeros((B, Tp, d), np.float32), np.zeros((B, Tp, 2), np.float32)
    check(mas._lib.lib().mis_debug_nemotron_dwconv_ln(0, _ptr(pw), _ptr(tk), _ptr(bias), _ptr(cnt), B, Tp, d, taps, pads[0], _ptr(out), _ptr(st)))
    ok = True
    for b, n in enumerate(FRAMES):
        ref = {}
        for dt in (torch.float64, torch.float32):
            a, g = _t(pw[b, :n], dt).chunk(2, dim=-1)
            h = torch.nn.functional.pad((a * torch.sigmoid(g)).t()[None], pads)
            y = torch.nn.functional.conv1d(h, _t(w, dt).permute(0, 2, 1), _t(bias, dt), groups=d)[0].t()
            ref[dt] = (y, torch.nn.functional.layer_norm(y, (d,), eps=1e-5))
        ok &= _gate(f"dwconv taps {taps} pads {pads} frames {n}", out[b, :n], ref[torch.float64][0].numpy(), ref[torch.float32][0].numpy())
        normed = (out[b, :n].astype(np.float64) - st[b, :n, :1]) * st[b, :n, 1:]           # the statistics, applied to the device's own output
        own = torch.nn.functional.layer_norm(_t(out[b, :n], torch.float64), (d,), eps=1e-5).numpy()
        own32 = torch.nn.functional.layer_norm(_t(out[b, :n], torch.float32), (d,), eps=1e-5).numpy()
        ok &= _gate(f"ln stats taps {taps} frames {n}", normed, own, own32)
        assert not out[b, n:].any() and not st[b, n:].any()
    assert ok


STEM = (1, 2, 7, 8, 9, 65)


def test_causal_stem_kernels_and_lengths():
    """conv0, then the two depthwise + pointwise stages, each from the device's previous stage; lengths floor(n / 2) + 1 three times"""
    Cc, mels, B = 16, 16, len(STEM)
    rng = np.random.default_rng(5)
    u = lambda shape, amp: rng.uniform(-amp, amp, shape).astype(np.float32)
    x = np.full((B, max(STEM), mels), np.nan, np.float32)
    for b, n in enumerate(STEM):
        x[b, :n] = rng.standard_normal((n, mels)).astype(np.float32)
    cnt, Tin, Fin, ok = np.asarray(STEM, np.int32), max(STEM), mels, True
    for stage in range(3):
        w, bias, pw, pwb = u((Cc, 3, 3, 1), 0.6), u((Cc,), 0.05), u((Cc, 1, 1, Cc), 0.4), u((Cc,), 0.05)
        w9 = np.ascontiguousarray(w.reshape(Cc, 9).T)
        Tout, Fout = N.half(Tin), N.half(Fin)
        out = np.zeros((B, Tout, Fout, Cc), np.float32)
        check(mas._lib.lib().mis_debug_nemotron_stem(0, min(stage, 1), _ptr(x), _ptr(cnt), B, Tin, Fin, Cc, _ptr(w9), _ptr(bias), _ptr(pw[:, 0, 0]) if stage else None,
                                                     _ptr(pwb) if stage else None, _ptr(out)))
        for b in range(B):
            n, m = int(cnt[b]), N.half(int(cnt[b]))
            ref = []
            for dt in (torch.float64, torch.float32):
                xin = _t(x[b, :n], dt)[None, None] if stage == 0 else _t(x[b, :n], dt).permute(2, 0, 1)[None]
                y = N.causal_conv(xin, _t(w, dt), _t(bias, dt), groups=1 if stage == 0 else Cc)
                if stage:
                    y = torch.nn.functional.conv2d(y, _t(pw, dt).permute(0, 3, 1, 2), _t(pwb, dt))
                ref.append(torch.relu(y)[0].permute(1, 2, 0).numpy())
            assert ref[0].shape == (m, Fout, Cc)
            ok &= _gate(f"stem stage {stage} frames {n}", out[b, :m], ref[0], ref[1])
            assert not out[b, m:].any()
        x, cnt, Tin, Fin = out, np.asarray([N.half(int(c)) for c in cnt], np.int32), Tout, Fout
    assert cnt.tolist() == [N.frames(n) for n in STEM] and ok


def _run_rnnt(W, layers, encp, counts, max_symbols, cap):
    c, B = N.RNNT, len(counts)
    lstm = lambda n: (C.c_void_p * layers)(*[_ptr(W[f"decoder.prediction.dec_rnn.lstm.{n}_l{l}"]) for l in range(layers)])
    cnt = np.asarray(counts, np.int32)
    tok, frm = (np.zeros((B, cap), np.int32) for _ in range(2))
    n, flg, stp = (np.zeros(B, np.int32) for _ in range(3))
    e = np.ascontiguousarray(encp, np.float32)
    check(mas._lib.lib().mis_debug_nemotron_rnnt(0, _ptr(e), _ptr(cnt), B, e.shape[1], c["J"], c["P"], c["vocab"], layers, max_symbols or 0, cap,
                                                 _ptr(W["decoder.prediction.embed.weight"]), lstm("weight_ih"), lstm("weight_hh"), lstm("bias_ih"),
                                                 lstm("bias_hh"), _ptr(W["joint.pred.weight"]), _ptr(W["joint.pred.bias"]), _ptr(W["joint.joint_net.weight"]),
                                                 _ptr(W["joint.joint_net.bias"]), _ptr(tok), _ptr(frm), _ptr(n), _ptr(flg), _ptr(stp)))
    return tok, frm, n, flg, stp


@pytest.mark.parametrize("group", ["plain", "all_blank", "always_emit", "no_max_symbols_capacity"])
@pytest.mark.parametrize("layers", [1, 2])
def test_rnnt_kernel_equals_the_specification(layers, group):
    """plain: the four rows without a bias override in ONE ragged launch (T_b = 1, 7, 19, 24; NaN behind every count); always_emit: every step
    emits until max_symbols forces the advance; no_max_symbols_capacity: nothing but the capacity ends the row, flagged"""
    c = N.RNNT
    W, rows = N.rnnt_cases(layers)
    mine = [r for r in rows if (r[3] is None) == (group == "plain") and (group == "plain" or r[0] == group)]
    Wc = dict(W)
    if mine[0][3] is not None:
        Wc["joint.joint_net.bias"] = mine[0][3]
    ms = mine[0][4]
    tok, frm, n, flg, stp = _run_rnnt(Wc, layers, np.stack([r[1] for r in mine]), [r[2] for r in mine], ms, c["cap"])
    for b, (name, e, T, _, _) in enumerate(mine):
        ref = N.rnnt_decode(Wc, e[:T], c["vocab"], ms, c["cap"])
        k = len(ref["tokens"])
        assert (int(n[b]), int(flg[b]), int(stp[b])) == (k, ref["flag"], ref["steps"]), name
        assert (tok[b, :k].tolist(), frm[b, :k].tolist()) == (ref["tokens"], ref["frames"]), name
        assert (tok[b, k:] == -1).all(), name                              # nothing written behind the count
    if group == "always_emit":
        assert n[0] == 5 * c["max_symbols"] and not flg[0]
    if group == "no_max_symbols_capacity":
        assert n[0] == c["cap"] and flg[0] == 1 and frm[0].max() == 0


@functools.lru_cache(maxsize=None)
def _model(hidden):
    cfg = N.case_config(hidden, bias=hidden == 256)
    W = N.make_weights(cfg, 21)
    return cfg, W, mas.NemotronASR.from_weights(cfg, W)


@functools.lru_cache(maxsize=None)
def _waves():
    return tuple(R.test_wave(40 + i, int(16000 * s) + 37 * i) for i, s in enumerate(SECONDS))


@pytest.mark.parametrize("hidden", [256, 144])
def test_end_to_end_stages_batch_invariance_and_launches(hidden):
    cfg, W, m = _model(hidden)
    waves, L = _waves(), cfg.num_hidden_layers
    for ctx in (None, (4, 1)):                                             # the default (56, 13), then the other listed context
        used = ctx or cfg.default_context
        batch = m.decode_raw(list(waves), LANGUAGES, ctx)
        assert m.launches == 9 + 15 * L + 2 == m.expected_launches["generate"]
        taps = [m.tap(s) for s in range(L + 3)]
        F, T = m.frames([len(w) for w in waves])
        assert T.tolist() == [N.frames(int(f)) for f in F]
        r64, r32 = N.Encoder(cfg, W, torch.float64, used), N.Encoder(cfg, W, torch.float32, used)
        ok = True
        for b, w in enumerate(waves):
            n, idx = int(T[b]), N.LANGS[LANGUAGES[b]]
            ok &= _gate(f"row {b} stem", taps[0][b, :n], r64.pre_encode(r64.features(w)).numpy(), r32.pre_encode(r32.features(w)).numpy())
            for s in range(1, L + 3):
                ok &= _gate(f"ctx {used} row {b} stage {s}", taps[s][b, :n], r64.stage_after(s, taps[s - 1][b, :n], idx).numpy(),
                            r32.stage_after(s, taps[s - 1][b, :n], idx).numpy())
                assert not taps[s][b, n:].any()
            ref = N.rnnt_decode(W, taps[L + 2][b, :n], cfg.vocab_size, cfg.max_symbols, cfg.max_tokens)
            assert batch[b]["tokens"].tolist() == ref["tokens"] and batch[b]["frames"].tolist() == ref["frames"] and batch[b]["steps"] == ref["steps"]
        assert ok
    batch = m.decode_raw(list(waves), LANGUAGES)
    enc, _ = m.encode(list(waves))
    assert m.launches == 7 + 15 * L
    junk, _ = m.encode(list(waves), junk=np.nan)
    assert np.array_equal(enc.view(np.uint32), junk.view(np.uint32))
    for b, w in enumerate(waves):                                          # a row alone, and with junk behind the lengths: the same bits
        alone, _ = m.encode([w])
        assert np.array_equal(alone[0].view(np.uint32), enc[b, :alone.shape[1]].view(np.uint32))
        one = m.decode_raw([w], LANGUAGES[b])[0]
        assert all(np.array_equal(one[k], batch[b][k]) for k in ("tokens", "frames"))
    for a, b in zip(m.decode_raw(list(waves), LANGUAGES, junk=np.nan), batch):
        assert all(np.array_equal(a[k], b[k]) for k in ("tokens", "frames"))
    res = m.generate_batch(list(waves), LANGUAGES)
    specials = [sum(1 for t in b["tokens"] if t >= 38) for b in batch]     # pieces 38, 39 are special: dropped from the text, kept in the state
    assert [len(r.tokens) for r in res] == [len(b["tokens"]) - s for b, s in zip(batch, specials)]
    if res[2].tokens:
        t0 = res[2].tokens[0]
        first = next(f for t, f in zip(batch[2]["tokens"], batch[2]["frames"]) if t < 38)
        assert t0.start == first * 8 * 160 / 16000 and t0.duration == 8 * 160 / 16000


def test_published_widths_one_layer():
    cfg = mas.NemotronConfig(num_hidden_layers=1, max_batch=1, max_seconds=2, max_tokens=256, max_symbols=10, vocabulary=[])
    m = mas.NemotronASR.synthetic(cfg, seed=5)
    out = m.decode_raw([R.test_wave(3, 32000)])[0]
    T = N.frames(201)
    assert m.launches == 9 + 15 + 2 and 1 <= out["steps"] <= T * 11 and len(out["tokens"]) <= out["steps"]
    enc, Tn = m.encode([R.test_wave(3, 32000)])
    assert enc.shape == (1, T, 1024) and int(Tn[0]) == T and np.isfinite(enc).all() and float(np.abs(enc).max()) > 0
    m.close()


def test_long_row_at_small_width():
    """400 s, 2 layers, hidden 144.  The receptive field of an encoder frame is bounded: a block's attention reaches L C + C - 1 = 69
    frames back and C - 1 = 13 ahead at (56, 13), its causal conv 8 back; two blocks: (69 + 8) x 2 = 154 back, 26 ahead.  A window of 200
    stem embeddings that starts at the last chunk boundary (a multiple of C = 14, so the chunk indices inside it are the row's) at or before
    t - 160 holds t - 154 .. t + 26 and therefore reproduces frame t."""
    cfg = N.case_config(144, bias=False, prompt=False, max_batch=1, max_seconds=400, max_tokens=64)
    W = N.make_weights(cfg, 23)
    m = mas.NemotronASR.from_weights(cfg, W)
    wave = R.test_wave(9, 16000 * 400)
    res = m.generate(wave)
    assert res.truncated or len(res.tokens) >= 0
    emb, enc = m.tap(0)[0], m.tap(cfg.num_hidden_layers)[0]
    assert enc.shape[0] == N.frames(40001) and np.isfinite(enc).all()
    ok = True
    for t in (180, 2503, enc.shape[0] - 41):
        s = (t - 160) // 14 * 14
        outs = []
        for dt in (torch.float64, torch.float32):
            r = N.Encoder(cfg, W, dt)
            x = r.intake(_t(emb[s:s + 200], dt))
            for i in range(cfg.num_hidden_layers):
                x = r.fc_layer(i, x)
            outs.append(x[t - s].numpy())
        ok &= _gate(f"long row frame {t}", enc[t], outs[0], outs[1])
    assert ok
    m.close()


def test_refusals():
    with pytest.raises(mas.AudioGenerationError, match="head size"):
        mas.NemotronASR(N.case_config(64))
    with pytest.raises(mas.AudioGenerationError, match="add up"):
        mas.NemotronASR(N.case_config(256, conv=(5, 5)))
    cfg, W, m = _model(256)
    with pytest.raises(mas.AudioGenerationError, match="max_seconds"):
        m.decode_raw([np.zeros(16000 * cfg.max_seconds + 1, np.float32)])
    with pytest.raises(mas.AudioGenerationError, match="beam"):
        m.generate(_waves()[0], beam_size=4)
    with pytest.raises(mas.AudioGenerationError, match="listed contexts"):
        m.decode_raw([_waves()[0]], att_context_size=(4, 20))                # C 21: distances down to -20, the listed pairs reach -13
    with pytest.raises(mas.AudioGenerationError, match="stream session"):
        m.stream_session()
    assert len(m.decode_raw([_waves()[0]])) == 1                           # the handle is still usable
    raw = mas.NemotronASR(cfg)
    with pytest.raises(mas.AudioGenerationError, match="not finalized"):
        raw.decode_raw([_waves()[0]])
