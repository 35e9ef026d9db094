"""-m gpu: SenseVoice (csrc/sensevoice.hip) through the C ABI against tests/sensevoice_ref.py, which test_sensevoice_cpu.py holds to
torch.nn and numpy / scipy.

Gate of the comparisons: relative rms distance of the device to the float64 specification <= 4 x the float32 specification's own
distance to the float64 one at that stage, + 2^-23.  Every stage is compared with the specification run on the device's own previous
stage.  MIS_SENSEVOICE_PARITY_LOG=<file> keeps every observed value (profiles/sensevoice/parity_observed.jsonl)."""
import ctypes as C
import functools
import json
import os
import struct

import numpy as np
import pytest

import mlx_audio_swift_amd as mas
import sensevoice_ref as R
from gpu_util import observe, record, rms

pytestmark = pytest.mark.gpu

FLOOR_FACTOR = 4.0
SLACK = 2.0 ** -23


def _log(row):
    path = os.environ.get("MIS_SENSEVOICE_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(row) + "\n")


def _observe(kind, value, tol):
    name = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].split("::")[-1]
    _log(dict(test=name, kind=kind, value=float(value), tol=float(tol)))
    print(f"{name} {kind}: {float(value):.3e} (tol {float(tol):.3e})")
    return observe(kind, value, tol)


def _relrms(a, b):
    b = np.asarray(b, np.float64)
    return rms(a, b) / max(float(np.sqrt(np.mean(b ** 2))), 1e-30)


def _gate(kind, dev, ref64, ref32):
    return _observe(kind, _relrms(dev, ref64), FLOOR_FACTOR * _relrms(ref32, ref64) + SLACK)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _lengths(cfg):
    """Samples of the eight rows: 0, win - 1, win, F = 1 (mod lfr_n), and T_b = 32, 33, 64, 65 (the attention tile edges); the first two
    are the four query rows alone, shorter than kernel_size."""
    n = cfg.frontend_conf.lfr_n
    F = [None, None, 1, n + 1, (32 - 4 - 1) * n + 1, (33 - 4 - 1) * n + 1, (64 - 4) * n, (65 - 4 - 1) * n + 1]
    return [0, 399] + [R.samples_for_frames(f) for f in F[2:]]


@functools.lru_cache(maxsize=None)
def _rows(name):
    return tuple(R.tone_row(100 + i, n) for i, n in enumerate(_lengths(R.case_config(name))))


@functools.lru_cache(maxsize=None)
def _weights(name):
    cfg = R.case_config(name)
    return R.make_weights(cfg, R.DECISION_SEED), R.make_cmvn(cfg, R.DECISION_SEED)


@functools.lru_cache(maxsize=None)
def _model(name, **ws):
    cfg = R.case_config(name, **ws)
    W, cmvn = _weights(name)
    return cfg, mas.SenseVoiceModel.from_weights(cfg, W, cmvn)


@functools.lru_cache(maxsize=None)
def _refs(name):
    cfg = R.case_config(name)
    W, cmvn = _weights(name)
    return R.SenseVoiceRef(cfg, W, cmvn, np.float32), R.SenseVoiceRef(cfg, W, cmvn, np.float64)


def _check_taps(name, dev, rows):
    cfg = dev.config
    r32, r64 = _refs(name)
    n = cfg.frontend_conf.lfr_n
    F = [R.frames_of(len(r)) for r in rows]
    T = [R.rows_of(f, n) for f in F]
    logp, Tdev = dev.forward(rows)
    assert Tdev.tolist() == T
    NS = r64.stages
    taps = {s: dev.tap(s) for s in range(2 + NS)}
    B = len(rows)
    assert taps[0].shape == (B, max(max(F), 1), cfg.frontend_conf.n_mels) and taps[1].shape == (B, max(T), cfg.input_size)
    ok = {}
    live = [b for b in range(B) if F[b] > 0]
    cat = lambda f: np.concatenate([np.asarray(f(b)).ravel() for b in live])
    ok["fbank"] = _gate("fbank", cat(lambda b: taps[0][b, :F[b]]), cat(lambda b: R.fbank(rows[b], cfg, np.float64)),
                        cat(lambda b: R.fbank(rows[b], cfg, np.float32)))
    every = lambda f: np.concatenate([np.asarray(f(b)).ravel() for b in range(B)])
    ok["intake"] = _gate("intake", every(lambda b: taps[1][b, :T[b]]),
                         every(lambda b: r64.intake(r64.features_from_fbank(taps[0][b, :F[b]]))),
                         every(lambda b: r32.intake(r32.features_from_fbank(taps[0][b, :F[b]]))))
    for s in range(NS):
        ok[s] = _gate(f"stage{s}", every(lambda b: taps[2 + s][b, :T[b]]), every(lambda b: r64.step(s, taps[1 + s][b, :T[b]])),
                      every(lambda b: r32.step(s, taps[1 + s][b, :T[b]])))
    ok["head"] = _gate("head", every(lambda b: logp[b, :T[b]]), every(lambda b: r64.log_probs_from(taps[1 + NS][b, :T[b]])),
                       every(lambda b: r32.log_probs_from(taps[1 + NS][b, :T[b]])))
    ok["chain"] = _gate("chain", every(lambda b: logp[b, :T[b]]), every(lambda b: r64.log_probs(rows[b])), every(lambda b: r32.log_probs(rows[b])))
    assert all(ok.values()), ok
    for s in range(2 + NS):                                           # zeros behind a row's own rows
        for b in range(B):
            assert not _bits(taps[s][b, (F[b] if s == 0 else T[b]):]).any(), (s, b)
    for b in range(B):
        assert not _bits(logp[b, T[b]:]).any(), b
    return T


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", ["A", "B"])
def test_taps_of_a_ragged_batch(name):
    cfg, dev = _model(name)
    T = _check_taps(name, dev, _rows(name))
    assert T == [4, 4, 5, 6, 32, 33, 64, 65]


def test_taps_at_the_published_widths():
    cfg, dev = _model("P", max_batch=2, head_rows=128)
    rows = (R.tone_row(7, 48000), R.tone_row(8, 16000))
    assert _check_taps("P", dev, rows) == [54, 21]


# ---------------------------------------------------------------------------------------------- 2
def test_a_row_does_not_depend_on_its_batch():
    cfg, dev = _model("A")
    rows = _rows("A")
    feats, Rr = dev.features(rows)
    logp, T = dev.forward(rows)
    toks, rich = dev.generate_tokens(rows)
    for b, r in enumerate(rows):
        f1, R1 = dev.features([r])
        assert R1[0] == Rr[b] and np.array_equal(_bits(f1[0, :R1[0]]), _bits(feats[b, :Rr[b]])), b
        l1, T1 = dev.forward([r])
        assert np.array_equal(_bits(l1[0]), _bits(logp[b, :T[b]])), b
        t1, r1 = dev.generate_tokens([r])
        assert t1[0] == toks[b] and r1[0].tolist() == rich[b].tolist(), b
    for junk in (1e30, float("nan")):
        assert np.array_equal(_bits(dev.features(rows, junk=junk)[0]), _bits(feats)), junk
        assert np.array_equal(_bits(dev.forward(rows, junk=junk)[0]), _bits(logp)), junk
        t2, r2 = dev.generate_tokens(rows, junk=junk)
        assert t2 == toks and np.array_equal(r2, rich), junk
    # a row with peak <= 1 and the same row times 32768
    x = rows[5]
    assert np.abs(x).max() <= 1.0
    a, b = dev.forward([x])[0], dev.forward([x * np.float32(32768)])[0]
    assert np.array_equal(_bits(a), _bits(b))
    assert dev.generate_tokens([x])[0] == dev.generate_tokens([x * np.float32(32768)])[0]


def test_a_batch_of_64():
    cfg, dev = _model("F", max_batch=64, max_seconds=1)
    rows = [R.tone_row(300 + i, 400 + 97 * i) for i in range(64)]
    toks, rich = dev.generate_tokens(rows)
    assert len(toks) == 64 and rich.shape == (64, 3)
    for b in (0, 31, 63):
        t1, r1 = dev.generate_tokens([rows[b]])
        assert t1[0] == toks[b] and r1[0].tolist() == rich[b].tolist()


# ---------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("dk", [4, 16, 128])
def test_attention_one_launch(dk):
    H, cnt, Tp = 2, [1, 31, 32, 33, 65], 65
    D = H * dk
    g = np.random.default_rng(dk)
    qkv = g.standard_normal((len(cnt), Tp, 3 * D)).astype(np.float32)
    cn = np.asarray(cnt, np.int32)
    out = np.zeros((len(cnt), Tp, D), np.float32)
    mas.generation.check(mas._lib.lib().mis_debug_sensevoice_attn(0, qkv.ctypes.data, 3 * D, D, 2 * D, cn.ctypes.data, len(cnt), Tp, H, dk,
                                                                  C.c_float(1.0 / np.sqrt(dk)), D, out.ctypes.data))
    cfg = mas.SenseVoiceConfig(encoder_conf=mas.SenseVoiceEncoderConfig(output_size=D, attention_heads=H, num_blocks=1, tp_blocks=0),
                               vocab_size=4)
    got, w64, w32 = [], [], []
    for b, n in enumerate(cnt):
        for acc, dst in ((np.float64, w64), (np.float32, w32)):
            ref = R.SenseVoiceRef.__new__(R.SenseVoiceRef)
            ref.cfg, ref.acc = cfg, acc
            x = qkv[b, :n].astype(acc)
            dst.append(ref.attention(x[:, :D], x[:, D:2 * D], x[:, 2 * D:]).ravel())
        got.append(out[b, :n].ravel())
        assert not _bits(out[b, n:]).any(), b
    assert _gate(f"attn_dk{dk}", np.concatenate(got), np.concatenate(w64), np.concatenate(w32))


def _head_argmax(X, W, bias, cnt):
    B, Tp, K = X.shape
    N = W.shape[0]
    nt = -(-N // 64)
    pmax, pidx = np.zeros((B, Tp, nt), np.float32), np.zeros((B, Tp, nt), np.int32)
    pred, toks, ntok, rich = np.zeros((B, Tp), np.int32), np.zeros((B, Tp), np.int32), np.zeros(B, np.int32), np.zeros((B, 3), np.int32)
    cn = np.asarray(cnt, np.int32)
    mas.generation.check(mas._lib.lib().mis_debug_sensevoice_head_argmax(
        0, X.ctypes.data, W.ctypes.data, None if bias is None else bias.ctypes.data, cn.ctypes.data, B, Tp, K, N, pmax.ctypes.data,
        pidx.ctypes.data, pred.ctypes.data, toks.ctypes.data, ntok.ctypes.data, rich.ctypes.data))
    return pmax, pidx, pred, toks, ntok, rich


@pytest.mark.parametrize("V,K", [(6, 8), (300, 48), (25055, 512)])
def test_head_argmax_one_launch(V, K):
    g = np.random.default_rng(V)
    B, Tp, cnt = 2, 70, [70, 9]
    X = g.standard_normal((B, Tp, K)).astype(np.float32)
    W = (g.standard_normal((V, K)) / np.sqrt(K)).astype(np.float32)
    bias = (0.1 * g.standard_normal(V)).astype(np.float32)
    pmax, pidx, pred, toks, ntok, rich = _head_argmax(X, W, bias, cnt)
    exempt = frames = 0
    for b in range(B):
        x = X[b, :cnt[b]]
        z64 = x.astype(np.float64) @ W.astype(np.float64).T + bias
        z32 = x @ W.T + bias
        top = np.sort(z64, axis=1)
        margin = top[:, -1] - top[:, -2]
        sure = margin >= 8 * np.abs(z32 - z64).max(axis=1)
        assert np.array_equal(pred[b, :cnt[b]][sure], z64.argmax(axis=1)[sure]), b
        exempt += int((~sure).sum()); frames += len(sure)
        p = pred[b, :cnt[b]]
        assert toks[b, :ntok[b]].tolist() == R.greedy_ctc(p[4:].tolist()) and rich[b].tolist() == R.rich_ids(p)
        # the tiles' pairs: each maximum is attained at its index
        m = np.take_along_axis(z32, np.clip(pidx[b, :cnt[b]], 0, V - 1), axis=1)
        assert np.abs(m - pmax[b, :cnt[b]]).max() < 1e-3
    record("sensevoice_head_argmax", vocab=V, exempt=exempt, frames=frames)
    assert exempt <= 0.01 * frames + 1


def test_head_argmax_ties_go_to_the_lower_index():
    g = np.random.default_rng(5)
    B, Tp, K, V = 1, 40, 48, 300
    X = np.abs(g.standard_normal((B, Tp, K))).astype(np.float32)
    W = (0.01 * g.standard_normal((V, K))).astype(np.float32)
    W[74] = W[10] = 1.0                                              # two column tiles (10 and 64 + 10): the same sum, the same bits
    W[42 + 128] = W[10 + 128] = 0.5                                  # one tile, its two column waves
    pmax, pidx, pred, toks, ntok, rich = _head_argmax(X, W, None, [Tp])
    assert np.array_equal(_bits(pmax[0, :, 0]), _bits(pmax[0, :, 1])) and (pidx[0, :, 0] == 10).all() and (pidx[0, :, 1] == 74).all()
    assert (pidx[0, :, 2] == 138).all() and (pred[0] == 10).all()
    assert ntok[0] == 1 and toks[0, 0] == 10 and rich[0].tolist() == [10, 10, 10]


# ---------------------------------------------------------------------------------------------- 4
def test_decisions():
    cfg, dev = _model("A")
    r32, r64 = _refs("A")
    rows = [R.tone_row(500 + i, 32000 + 3000 * i) for i in range(8)]
    logp, T = dev.forward(rows)
    toks, rich = dev.generate_tokens(rows)
    exempt = frames = clean = 0
    for b, x in enumerate(rows):
        l64, l32 = r64.log_probs(x), r32.log_probs(x)
        top = np.sort(l64, axis=1)
        sure = (top[:, -1] - top[:, -2]) >= 8 * np.abs(l32 - l64).max(axis=1)
        want, got = l64.argmax(axis=1), logp[b, :T[b]].argmax(axis=1)
        assert np.array_equal(got[sure], want[sure]), b
        assert toks[b] == R.greedy_ctc(got[4:].tolist()) and rich[b].tolist() == R.rich_ids(got), b
        if sure.all():
            clean += 1
            assert toks[b] == R.greedy_ctc(want[4:].tolist()) and rich[b].tolist() == R.rich_ids(want), b
        exempt += int((~sure).sum()); frames += len(sure)
    record("sensevoice_decisions", exempt=exempt, frames=frames, clean_rows=clean)
    assert exempt <= 0.01 * frames
    # a head bias favouring blank
    W, cmvn = _weights("A")
    Wb = dict(W)
    Wb["ctc_lo.bias"] = W["ctc_lo.bias"].copy()
    Wb["ctc_lo.bias"][0] += np.float32(100.0)
    m = mas.SenseVoiceModel.from_weights(cfg, Wb, cmvn)
    assert m.generate_tokens(rows[:2])[0] == [[], []]
    m.close()


# ---------------------------------------------------------------------------------------------- 5
def test_forward_chunking_is_exact():
    rows = _rows("A")[3:]
    _, whole = _model("A")
    _, small = _model("A", head_rows=16)
    a, b = whole.forward(rows)[0], small.forward(rows)[0]
    assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b))
    L = whole.config.num_layers
    assert whole.launches == 5 + 5 * L + 2 and small.launches == 5 + 5 * L + 2 * len(rows) * -(-65 // 16)


# ---------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("name", ["A", "B", "F"])
def test_launch_count(name):
    cfg, dev = _model(name)
    rows = _rows(name)
    dev.generate_tokens(rows[4:5])
    one = dev.launches
    dev.generate_tokens(rows)
    record("sensevoice_launches", shape=name, launches=dev.launches)
    assert one == dev.launches == 7 + 5 * cfg.num_layers
    dev.features(rows)
    assert dev.launches == 3


# ---------------------------------------------------------------------------------------------- 7
def test_errors():
    cfg, dev = _model("A")
    rows = _rows("A")
    with pytest.raises(mas.AudioGenerationError) as e:
        dev.generate_tokens([np.zeros(4 * 16000 + 1, np.float32)])
    assert "max_seconds" in str(e.value)
    assert dev.generate_tokens([rows[4]])[1].shape == (1, 3)          # a rejected call leaves the handle usable
    with pytest.raises(mas.AudioGenerationError):
        dev.generate_tokens([])
    with pytest.raises(mas.AudioGenerationError) as e:
        dev.generate_tokens([rows[2]] * 65)
    assert "batch" in str(e.value)
    import copy
    bad = copy.deepcopy(cfg)
    bad.frontend_conf.frame_length = 40                               # 640 samples: the next power of two is 1024
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.SenseVoiceModel(bad)
    assert "window" in str(e.value)
    W, cmvn = _weights("A")
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.SenseVoiceModel.from_weights(cfg, {**W, "encoder.extra.weight": W["ctc_lo.bias"]})
    assert "encoder.extra.weight" in str(e.value)
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.SenseVoiceModel.from_weights(cfg, {k: v for k, v in W.items() if k != "encoder.tp_norm.bias"})
    assert "encoder.tp_norm.bias" in str(e.value)
    m = mas.SenseVoiceModel(cfg)
    for k, v in W.items():
        if k != "ctc_lo.bias":
            m.set_tensor(k, v)
    with pytest.raises(mas.AudioGenerationError) as e:
        m.finalize()
    assert "ctc_lo.bias" in str(e.value)
    m.close()


# ---------------------------------------------------------------------------------------------- 8
def _toy_model_bytes():
    def varint(v):
        out = b""
        while True:
            b, v = v & 0x7F, v >> 7
            out += bytes([b | (0x80 if v else 0)])
            if not v:
                return out

    def piece(text, score, kind):
        t = text.encode("utf-8")
        body = b"\x0a" + varint(len(t)) + t + b"\x15" + struct.pack("<f", score) + b"\x18" + varint(kind)
        return b"\x0a" + varint(len(body)) + body

    return b"".join(piece(t, s, k) for t, s, k in (("<unk>", 0.0, 2), ("<s>", 0.0, 3), ("</s>", 0.0, 3), ("▁hello", -1.0, 1),
                                                   ("▁world", -2.0, 1)))


def test_model_directory(tmp_path):
    import torch
    from safetensors.torch import save_file
    cfg = R.case_config("F")
    W = R.make_weights(cfg, 3)
    raw = {}
    for k, v in W.items():
        t = torch.from_numpy(v)
        if k.endswith("fsmn_block.weight"):
            t = t.permute(0, 2, 1).contiguous()                       # torch's [channels, 1, kernel]
        raw[k.replace("ctc_lo.", "ctc.ctc_lo.")] = t.contiguous()
    e, f = cfg.encoder_conf, cfg.frontend_conf
    (tmp_path / "config.json").write_text(json.dumps({
        "model_type": "sensevoice", "vocab_size": cfg.vocab_size, "input_size": cfg.input_size,
        "encoder_conf": {"output_size": e.output_size, "attention_heads": e.attention_heads, "linear_units": e.linear_units,
                         "num_blocks": e.num_blocks, "tp_blocks": e.tp_blocks, "kernel_size": e.kernel_size, "sanm_shfit": 0},
        "frontend_conf": {"fs": f.fs, "window": f.window, "n_mels": f.n_mels, "lfr_m": f.lfr_m, "lfr_n": f.lfr_n}}))
    fmt = lambda a: " ".join(repr(float(v)) for v in a)
    (tmp_path / "am.mvn").write_text(f"<Nnet>\n<AddShift> 560 560\n<LearnRateCoef> 0 [ {fmt(np.zeros(560))} ]\n<Rescale> 560 560\n"
                                     f"<LearnRateCoef> 0 [ {fmt(np.ones(560))} ]\n</Nnet>\n")
    (tmp_path / "toy.model").write_bytes(_toy_model_bytes())
    save_file(raw, str(tmp_path / "model.safetensors"))
    m = mas.SenseVoiceModel.from_pretrained(str(tmp_path), max_batch=2, max_seconds=2)
    assert m.has_cmvn and m.tokenizer is not None and m.tokenizer.decode([3, 4]) == "hello world"
    out = m.generate(np.zeros(16000, np.float32))
    assert len(out.segments) == 1 and set(out.segments[0]) == {"text", "language", "emotion", "event"} and out.language == "unknown"
    assert out.segments[0]["emotion"].startswith("token_") and out.text == out.segments[0]["text"]
    plain = mas.SenseVoiceModel.from_weights(R.case_config("F", max_batch=2, max_seconds=2), W, (np.zeros(560, np.float32), np.ones(560, np.float32)))
    x = R.tone_row(1, 16000)
    assert np.array_equal(_bits(m.forward([x])[0]), _bits(plain.forward([x])[0]))
    assert [k for k, _ in m.generate_stream(x)] == ["result"]
    m.close(); plain.close()
