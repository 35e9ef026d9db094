"""-m gpu: Parakeet TDT (csrc/parakeet.hip) through the C ABI against tests/parakeet_ref.py, which test_parakeet_cpu.py holds to
transformers, torch.nn.LSTM and a transliteration of the reference's decode loop.

Gate of the float comparisons: relative rms distance of the device to the float64 specification <= 4 x the float32 specification's own
distance to the float64 one, + 2^-23.  Every stage is compared with the specification run on the device's own previous stage.  Decisions
(tokens, frames, durations, counts, flags) are compared for equality, no row exempt: test_parakeet_cpu.test_decision_margin holds the margin
that allows it.  MIS_PARAKEET_PARITY_LOG=<file> keeps every observed value (profiles/parakeet/parity_observed.jsonl)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
from mlx_audio_swift_amd.generation import check
import parakeet_ref as P
import sortformer_ref as R
from gpu_util import observe, rms

pytestmark = pytest.mark.gpu
KEYS = (1, 31, 33, 64, 65, 97)
SECONDS = (0.3, 1.0, 2.5)


def _gate(kind, dev, ref64, ref32):
    rel = lambda a, b: rms(a, np.asarray(b, np.float64)) / max(float(np.sqrt(np.mean(np.asarray(b, np.float64) ** 2))), 1e-30)
    value, tol = rel(dev, ref64), 4.0 * rel(ref32, ref64) + 2.0 ** -23
    name = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].split("::")[-1]
    if os.environ.get("MIS_PARAKEET_PARITY_LOG"):
        with open(os.environ["MIS_PARAKEET_PARITY_LOG"], "a") as f:
            f.write(json.dumps(dict(test=name, kind=kind, value=float(value), tol=float(tol))) + "\n")
    print(f"{name} {kind}: {value:.3e} (tol {tol:.3e})")
    return observe(kind, value, tol)


def _ptr(a):
    return a.ctypes.data


@pytest.mark.parametrize("hd", [128, 72])
def test_attention_kernel_against_the_literal_rel_shift(hd):
    H, Tp, Tcap, B = 2, max(KEYS), 100, len(KEYS)
    rng = np.random.default_rng(hd)
    w = H * hd
    qkv = np.full((B, Tp, 3 * w), np.nan, np.float32)
    for b, n in enumerate(KEYS):
        qkv[b, :n] = rng.standard_normal((n, 3 * w)).astype(np.float32)
    table = rng.standard_normal((2 * Tcap - 1, w)).astype(np.float32)
    u, v = (rng.uniform(-0.5, 0.5, (H, hd)).astype(np.float32) for _ in range(2))
    cnt, out = np.asarray(KEYS, np.int32), np.zeros((B, Tp, w), np.float32)
    check(mas._lib.lib().mis_debug_parakeet_attn(0, _ptr(qkv), 3 * w, w, 2 * w, _ptr(cnt), B, Tp, H, hd, 1.0, float(np.sqrt(hd)), _ptr(u), _ptr(v),
                                                     _ptr(table), w, Tcap, w, _ptr(out)))
    ok = True
    for b, n in enumerate(KEYS):
        r64, r32 = (P.attention(qkv[b], table, u, v, n, H, hd, Tcap, dt) for dt in (torch.float64, torch.float32))
        ok &= _gate(f"attn hd {hd} keys {n}", out[b, :n], r64, r32)
        assert not out[b, n:].any()
    assert ok


def _run_tdt(W, encp, counts, cap):
    c, B = P.TDT, len(counts)
    lstm = lambda n: (C.c_void_p * 2)(*[_ptr(W[f"decoder.prediction.dec_rnn.lstm.{n}_l{l}"]) for l in range(2)])
    dur, cnt = np.asarray(P.DURATIONS, np.int32), np.asarray(counts, np.int32)
    tok, frm, drs = (np.zeros((B, cap), np.int32) for _ in range(3))
    n, flg, stp = (np.zeros(B, np.int32) for _ in range(3))
    e = np.ascontiguousarray(encp, np.float32)
    check(mas._lib.lib().mis_debug_parakeet_tdt(0, _ptr(e), _ptr(cnt), B, e.shape[1], c["J"], c["P"], c["vocab"], len(dur), _ptr(dur), c["max_symbols"], cap,
                                                    _ptr(W["decoder.prediction.embed.weight"]), lstm("weight_ih"), lstm("weight_hh"), lstm("bias_ih"),
                                                    lstm("bias_hh"), _ptr(W["joint.pred.weight"]), _ptr(W["joint.pred.bias"]), _ptr(W["joint.joint_net.weight"]),
                                                    _ptr(W["joint.joint_net.bias"]), _ptr(tok), _ptr(frm), _ptr(drs), _ptr(n), _ptr(flg), _ptr(stp)))
    return tok, frm, drs, n, flg, stp


@pytest.mark.parametrize("group", ["plain", "duration_0_always", "blank_duration_0", "jump_past_end", "all_blank", "capacity"])
def test_tdt_kernel_equals_the_specification(group):
    """plain: the four rows without a bias override in ONE ragged launch (T_b = 1, 7, 19, 24; NaN behind every count); every other case
    reaches its arg-max through its own joint_net bias, so it is its own launch."""
    c = P.TDT
    W, rows = P.tdt_cases()
    mine = [r for r in rows if (r[3] is None) == (group == "plain") and (group == "plain" or r[0] == group)]
    Wc = dict(W)
    if mine[0][3] is not None:
        Wc["joint.joint_net.bias"] = mine[0][3]
    tok, frm, drs, n, flg, stp = _run_tdt(Wc, np.stack([r[1] for r in mine]), [r[2] for r in mine], c["cap"])
    for b, (name, e, T, _) in enumerate(mine):
        ref = P.tdt_decode(Wc, e[:T], c["vocab"], P.DURATIONS, c["max_symbols"], c["cap"])
        k = len(ref["tokens"])
        assert (int(n[b]), int(flg[b]), int(stp[b])) == (k, ref["flag"], ref["steps"]), name
        assert (tok[b, :k].tolist(), frm[b, :k].tolist(), drs[b, :k].tolist()) == (ref["tokens"], ref["frames"], ref["durations"]), name
        assert (tok[b, k:] == -1).all(), name                              # nothing written behind the count


@functools.lru_cache(maxsize=None)
def _model(hidden):
    cfg = P.case_config(hidden)
    W = P.make_weights(cfg, 21)
    return cfg, W, mas.ParakeetModel.from_weights(cfg, W)


@functools.lru_cache(maxsize=None)
def _waves():
    return tuple(R.test_wave(40 + i, int(16000 * s) + 37 * i) for i, s in enumerate(SECONDS))


@pytest.mark.parametrize("hidden", [256, 144])
def test_end_to_end_stages_batch_invariance_and_launches(hidden):
    cfg, W, m = _model(hidden)
    waves, L = _waves(), cfg.num_hidden_layers
    batch = m.decode_raw(list(waves))
    assert m.launches == 9 + 15 * L == m.expected_launches["generate"]
    taps = [m.tap(s) for s in range(L + 2)]
    _, T = m.frames([len(w) for w in waves])
    r64, r32 = P.Encoder(cfg, W, torch.float64), P.Encoder(cfg, W, torch.float32)
    ok = True
    for b, w in enumerate(waves):
        n = int(T[b])
        ok &= _gate(f"row {b} stem", taps[0][b, :n], r64.pre_encode(r64.features(w)).numpy(), r32.pre_encode(r32.features(w)).numpy())
        for s in range(1, L + 2):
            ok &= _gate(f"row {b} stage {s}", taps[s][b, :n], r64.stage_after(s, taps[s - 1][b, :n]).numpy(), r32.stage_after(s, taps[s - 1][b, :n]).numpy())
            assert not taps[s][b, n:].any()
        # the decode of the device's own projected frames, by the specification
        ref = P.tdt_decode(W, taps[L + 1][b, :n], cfg.vocab_size, P.DURATIONS, cfg.max_symbols, cfg.max_tokens)
        assert batch[b]["tokens"].tolist() == ref["tokens"] and batch[b]["frames"].tolist() == ref["frames"] and batch[b]["steps"] == ref["steps"]
    assert ok
    enc, _ = m.encode(list(waves))
    assert m.launches == 7 + 15 * L
    junk, _ = m.encode(list(waves), junk=np.nan)
    assert np.array_equal(enc.view(np.uint32), junk.view(np.uint32))
    for b, w in enumerate(waves):                                          # a row alone, and with junk behind the lengths: the same bits
        alone, _ = m.encode([w])
        assert np.array_equal(alone[0].view(np.uint32), enc[b, :alone.shape[1]].view(np.uint32))
        one = m.decode_raw([w])[0]
        assert all(np.array_equal(one[k], batch[b][k]) for k in ("tokens", "frames", "durations"))
    for a, b in zip(m.decode_raw(list(waves), junk=np.nan), batch):
        assert all(np.array_equal(a[k], b[k]) for k in ("tokens", "frames", "durations"))
    res = m.generate_batch(list(waves))
    assert [len(r.tokens) for r in res] == [len(b["tokens"]) for b in batch]
    if res[2].tokens:
        t0 = res[2].tokens[0]
        assert t0.start == batch[2]["frames"][0] * 8 * 160 / 16000 and t0.duration == batch[2]["durations"][0] * 8 * 160 / 16000


def test_published_widths_one_layer():
    cfg = mas.ParakeetConfig(num_hidden_layers=1, max_batch=1, max_seconds=2, max_tokens=256, vocabulary=[])
    m = mas.ParakeetModel.synthetic(cfg, seed=5)
    out = m.decode_raw([R.test_wave(3, 32000)])[0]
    assert m.launches == 24 and 1 <= out["steps"] <= 26 * 11 and len(out["tokens"]) <= out["steps"]
    enc, T = m.encode([R.test_wave(3, 32000)])
    assert enc.shape == (1, 26, 1024) and np.isfinite(enc).all() and float(np.abs(enc).max()) > 0
    m.close()


def test_refusals():
    with pytest.raises(mas.AudioGenerationError, match="head size"):
        mas.ParakeetModel(P.case_config(258, heads=2))
    cfg, W, m = _model(256)
    with pytest.raises(mas.AudioGenerationError, match="max_seconds"):
        m.decode_raw([np.zeros(16000 * cfg.max_seconds + 1, np.float32)])
    with pytest.raises(mas.AudioGenerationError, match="beam"):
        m.generate(_waves()[0], beam_size=4)
    assert len(m.decode_raw([_waves()[0]])) == 1                           # the handle is still usable
    raw = mas.ParakeetModel(cfg)
    with pytest.raises(mas.AudioGenerationError, match="not finalized"):
        raw.decode_raw([_waves()[0]])
