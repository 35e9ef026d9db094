"""-m gpu: the Moonshine engine (csrc/moonshine.hip) through the C ABI against tests/moonshine_ref.py, which test_moonshine_cpu.py holds
to transformers' implementation.

Gate of every numeric comparison (the idiom of test_gpu_fulldepth.py, same numbers): relative rms distance of the device to the
reference with bf16 rounding points <= FLOOR_FACTOR x the distance of the reference's own float64-accumulation realisation to it, + 2e-3.
Two exact realisations of one specification differ because summation order flips bf16 roundings; the device has to sit at that floor.
The distance to the reference WITHOUT bf16 rounding (what running an f32 checkpoint in bf16 costs) is recorded, not gated."""
import json
import os
import wave

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
import moonshine_ref as mr
from gpu_util import observe, record, rms

pytestmark = pytest.mark.gpu

FLOOR_FACTOR = 2.0
SLACK = 2e-3
HERE = os.path.dirname(os.path.abspath(__file__))

HD36 = dict(vocab_size=2048, hidden_size=288, intermediate_size=1152, encoder_num_hidden_layers=2, decoder_num_hidden_layers=2)
HD52 = dict(vocab_size=2048, hidden_size=416, intermediate_size=1664, encoder_num_hidden_layers=2, decoder_num_hidden_layers=2)
HD64 = dict(vocab_size=2048, hidden_size=512, intermediate_size=640, encoder_num_hidden_layers=2, decoder_num_hidden_layers=2,
            attention_bias=True, tie_word_embeddings=False, encoder_num_key_value_heads=4, decoder_num_key_value_heads=2)
TINY_DEPTH = dict(HD36, encoder_num_hidden_layers=6, decoder_num_hidden_layers=6)
BASE_DEPTH = dict(HD52, encoder_num_hidden_layers=8, decoder_num_hidden_layers=8)
T_DEC = 6


def _wave(n, seed):
    g = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return (0.15 * np.sin(2 * np.pi * (180 + 40 * seed) * t) + 0.1 * g.standard_normal(n)).astype(np.float32)


def _intention():
    with wave.open(os.path.join(HERE, "golden", "intention.wav"), "rb") as w:
        return np.frombuffer(w.readframes(w.getnframes()), "<i2").astype(np.float32) / 32768.0


RAGGED = [960, 320000, 16000, 5000, 48000, 1663]                 # 0.06 s .. 20 s
ROWS32 = [960 + 733 * i for i in range(32)]                     # 0.06 s .. 1.5 s


def _rows(kind):
    if kind == "b1":
        return [_wave(24000, 1)]
    if kind == "intention":
        return [_intention()[:64000]]
    if kind == "ragged":
        return [_wave(n, i) for i, n in enumerate(RAGGED)]
    return [_wave(n, i) for i, n in enumerate(ROWS32)]


def _pair(shape, seed=11):
    cfg = mas.MoonshineConfig(**shape)
    W = mr.make_weights(cfg, seed=seed)
    return cfg, W, mas.MoonshineModel.from_weights(cfg, W)


def _relrms(a, b):
    b = np.asarray(b, np.float64)
    return rms(a, b) / max(float(np.sqrt(np.mean(b ** 2))), 1e-30)


def _gate(kind, dev, ref, floor):
    d, f = _relrms(dev, ref), _relrms(floor, ref)
    return observe(kind, d, FLOOR_FACTOR * f + SLACK)


def test_stem_taps_against_the_reference():
    cfg, W, dev = _pair(HD36)
    rows = [_wave(n, i) for i, n in enumerate([960, 40000, 7000])]
    r32, r64 = mr.MoonshineRef(cfg, W, round="bf16"), mr.MoonshineRef(cfg, W, round="bf16", acc=torch.float64)
    refs = [(r32.stem(r), r64.stem(r)) for r in rows]
    ok = True
    for stage in range(4):
        got = dev.stem_tap(rows, stage)
        for b in range(len(rows)):
            assert got[b].shape == tuple(refs[b][0][stage].shape), (stage, b)
        cat = lambda xs: np.concatenate([np.asarray(x).reshape(-1) for x in xs])
        ok &= _gate(f"stem_stage{stage}", cat(got), cat([r[0][stage] for r in refs]), cat([r[1][stage] for r in refs]))
    dev.close()
    assert ok


@pytest.mark.parametrize("shape,kind", [
    pytest.param(HD36, "ragged", id="hd36-ragged6"), pytest.param(HD52, "ragged", id="hd52-ragged6"),
    pytest.param(HD64, "ragged", id="hd64-gqa-bias-untied-ragged6"), pytest.param(HD52, "b1", id="hd52-b1"),
    pytest.param(HD36, "rows32", id="hd36-32rows"), pytest.param(HD52, "rows32", id="hd52-32rows"),
    pytest.param(TINY_DEPTH, "intention", id="tiny-depth-6+6-intention-wav"),
    pytest.param(TINY_DEPTH, "ragged", id="tiny-depth-6+6-ragged6"),
    pytest.param(BASE_DEPTH, "ragged", id="base-depth-8+8-ragged6", marks=pytest.mark.slow)])
def test_encoder_and_teacher_forced_logits(shape, kind):
    cfg, W, dev = _pair(shape)
    rows = _rows(kind)
    B = len(rows)
    toks = np.random.default_rng(5).integers(0, cfg.vocab_size, (B, T_DEC))
    toks[:, 0] = cfg.decoder_start_token_id
    enc = dev.encode(rows)
    dev.decoder_reset()
    lg = np.stack([dev.decoder_forward(toks[:, t]) for t in range(T_DEC)], 1)                # [B, T, V]
    assert dev.frames([len(r) for r in rows]).tolist() == [e.shape[0] for e in enc]
    r32, r64, rf = (mr.MoonshineRef(cfg, W, round="bf16"), mr.MoonshineRef(cfg, W, round="bf16", acc=torch.float64),
                    mr.MoonshineRef(cfg, W, round=None))
    # the CPU reference walks a subset of a 32-row batch (every 4th row and both ends); every row of the smaller batches
    check = list(range(B)) if B <= 8 else sorted(set(list(range(0, B, 4)) + [B - 1]))
    E, L = {k: [] for k in "dfu"}, {k: [] for k in "dfu"}
    for b in check:
        a = torch.from_numpy(rows[b])
        for key, ref in (("d", r32), ("f", r64), ("u", rf)):
            e = ref.encode(a)
            E[key].append(e.numpy().reshape(-1))
            L[key].append(ref.decode_all(toks[b], e).numpy().reshape(-1))
    cat = np.concatenate
    dev_e, dev_l = cat([enc[b].reshape(-1) for b in check]), cat([lg[b].reshape(-1) for b in check])
    record("moonshine_unrounded_distance", shape=f"{cfg.hidden_size}/{cfg.encoder_num_hidden_layers}", kind=kind,
           enc=_relrms(dev_e, cat(E["u"])), logits=_relrms(dev_l, cat(L["u"])))
    ok = _gate("encoder", dev_e, cat(E["d"]), cat(E["f"]))
    ok &= _gate("logits", dev_l, cat(L["d"]), cat(L["f"]))
    # a row inside the batch means what the row alone means
    if B > 1:
        b = check[len(check) // 2]
        alone = dev.encode([rows[b]])[0]
        dev.decoder_reset()
        lg1 = np.stack([dev.decoder_forward(toks[b:b + 1, t])[0] for t in range(T_DEC)])
        i = check.index(b)
        ok &= observe("row_alone_vs_in_batch_encoder", _relrms(alone, enc[b]), FLOOR_FACTOR * _relrms(E["f"][i], E["d"][i]) + SLACK)
        ok &= observe("row_alone_vs_in_batch_logits", _relrms(lg1, lg[b]), FLOOR_FACTOR * _relrms(L["f"][i], L["d"][i]) + SLACK)
    dev.close()
    assert ok


def test_padding_is_inert():
    """Samples behind lens[b] overwritten with large finite junk: same batch shape, same kernels -> bit-identical results."""
    cfg, W, dev = _pair(dict(HD36, eos_token_id=2047))
    rows = [_wave(n, i) for i, n in enumerate([960, 30000, 4001, 12345, 20000])]
    gp = mas.STTGenerateParameters(max_tokens=10, temperature=0.0)
    out = {}
    for junk in (None, 3.0e4):
        enc = dev.encode(rows, junk=junk)
        dev.decoder_reset()
        lg = [dev.decoder_forward(np.full(len(rows), t + 1, np.int32)) for t in range(3)]
        out[junk] = (enc, lg, dev.generate_ids(rows, gp, junk=junk), [dev.stem_tap(rows, s, junk=junk) for s in range(4)])
    a, b = out[None], out[3.0e4]
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(x, y)
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(x, y)
    assert a[2] == b[2] and all(len(t) == 10 for t in a[2])
    for sa, sb in zip(a[3], b[3]):
        for x, y in zip(sa, sb):
            assert np.array_equal(x, y)
    dev.close()


def test_generate_choices_eos_rule_and_counts():
    """The reference is fed the engine's own tokens: at every step the reference logit of the engine's choice must lie within a bound
    of the reference's maximum - no step is left out.  Bound: both logits (the chosen one and the maximum) may be off by the engine's
    logit error, which the floor gate of this file limits to FLOOR_FACTOR x the reference's own float64-accumulation distance + SLACK of
    the largest logit; so 2 x (FLOOR_FACTOR x max|float64 ref - ref| + SLACK x max|ref|), computed per row from the reference alone.
    Then the EOS rule, max_tokens and the token counts."""
    shape = dict(HD36, eos_token_id=2047, tie_word_embeddings=False)   # (untied: with random tied weights greedy decoding repeats one id)
    cfg, W, dev = _pair(shape)
    rows = [_wave(n, i + 3) for i, n in enumerate([9000, 960, 33000, 16000])]
    K = 12
    gp = mas.STTGenerateParameters(max_tokens=K, temperature=0.0)
    ids = dev.generate_ids(rows, gp)
    assert all(len(t) == K for t in ids) and all(2047 not in t for t in ids), ids            # 2047 is unreachable with these weights
    ref, ref64 = mr.MoonshineRef(cfg, W, round="bf16"), mr.MoonshineRef(cfg, W, round="bf16", acc=torch.float64)
    worst = 0.0
    for b, r in enumerate(rows):
        fed = [cfg.decoder_start_token_id] + ids[b][:-1]
        lg = ref.decode_all(fed, ref.encode(torch.from_numpy(r))).numpy()                    # [K, V]
        lg64 = ref64.decode_all(fed, ref64.encode(torch.from_numpy(r))).numpy()
        bound = 2 * (FLOOR_FACTOR * float(np.abs(lg64 - lg).max()) + SLACK * float(np.abs(lg).max()))
        for t in range(K):
            gap = float(lg[t].max() - lg[t][ids[b][t]])
            worst = max(worst, gap / bound)
            assert observe("generate_choice_gap", gap, bound), (b, t)
    record("moonshine_generate_choice_gap_over_bound", worst=worst)
    # generation_tokens / total_tokens as the reference counts them (:406-407), one waveform and a ragged list
    one = dev.generate(rows[0], gp)
    assert (one.generation_tokens, one.total_tokens, one.token_ids) == (K, K + 1, ids[0])
    assert one.text == dev.decode(ids[0]).strip() and one.segments == [{"text": one.text, "start": 0.0, "end": 0.0}]
    stereo = np.stack([rows[0] * 2, np.zeros_like(rows[0])], -1)                             # averaged over the last axis (:376)
    assert dev.generate(stereo, gp).token_ids == ids[0]
    ev = list(dev.generate_stream(rows[0], gp))
    assert [e[0] for e in ev] == ["token", "result"] and ev[0][1] == one.text and ev[1][1].token_ids == ids[0]
    short = dev.generate_ids(rows, mas.STTGenerateParameters(max_tokens=5, temperature=0.0))
    assert short == [t[:5] for t in ids]                                                     # max_tokens honoured, same prefix
    dev.close()
    # EOS = the token row 0 produced at step k: row 0 returns exactly k tokens, the others stop at their own first occurrence
    k = max(t for t in range(K) if ids[0][t] not in ids[0][:t])                             # the last step at which row 0 said something new
    eos = ids[0][k]
    assert k >= 1, ids[0]
    dev2 = mas.MoonshineModel.from_weights(mas.MoonshineConfig(**dict(shape, eos_token_id=eos)), W)
    got = dev2.generate_ids(rows, gp)
    for b in range(len(rows)):
        want = ids[b][: ids[b].index(eos)] if eos in ids[b] else ids[b]
        assert got[b] == want and eos not in got[b], b
    assert len(got[0]) == k
    outs = dev2.generate(rows, gp)
    assert [o.generation_tokens for o in outs] == [len(t) for t in got] and [o.total_tokens for o in outs] == [len(t) + 1 for t in got]
    dev2.close()


def test_errors_leave_the_handle_usable():
    cfg, W, dev = _pair(HD36)
    good = _wave(4000, 1)
    gp = mas.STTGenerateParameters(max_tokens=4, temperature=0.0)
    before = dev.generate_ids([good], gp)
    for rows, params, word in (([good, _wave(894, 2)], gp, "895"), ([_wave(480001, 3)], gp, "cap"),
                               ([good], mas.STTGenerateParameters(max_tokens=4, temperature=0.7), "temperature")):
        with pytest.raises(mas.AudioGenerationError) as e:
            dev.generate_ids(rows, params)
        assert e.value.case == "invalidInput" and word in str(e.value), str(e.value)
        assert dev.generate_ids([good], gp) == before
    with pytest.raises(mas.AudioGenerationError) as e:
        dev.encode([_wave(894, 2)])
    assert e.value.case == "invalidInput"
    assert len(dev.generate_ids([_wave(480000, 4)], gp)[0]) == 4                             # the cap itself is served
    dev.close()


def test_loader_gives_the_same_tokens_and_decodes_text(tmp_path):
    from safetensors.torch import save_file
    shape = dict(HD36, vocab_size=300, eos_token_id=299)
    cfg = mas.MoonshineConfig(**shape)
    W = mr.make_weights(cfg, seed=21)
    (tmp_path / "config.json").write_text(json.dumps(dict(shape, model_type="moonshine")))
    save_file({k: v.contiguous() for k, v in W.items()}, os.path.join(tmp_path, "model.safetensors"))
    vocab = {f"▁w{i}": i for i in range(300)}
    (tmp_path / "tokenizer.json").write_text(json.dumps({"model": {"vocab": vocab}, "added_tokens": [{"id": 1, "special": True}]}), encoding="utf-8")
    rows = [_wave(9000, 1), _wave(2000, 2)]
    gp = mas.STTGenerateParameters(max_tokens=6, temperature=0.0)
    a = mas.MoonshineModel.from_weights(cfg, W)
    b = mas.MoonshineModel.from_pretrained(str(tmp_path))
    ia, ib = a.generate_ids(rows, gp), b.generate_ids(rows, gp)
    assert ia == ib and b.tokenizer is not None and b.config.vocab_size == 300
    out = b.generate(rows[0], gp)
    assert out.text == " ".join(f"w{i}" for i in ia[0] if i != 1) and out.token_ids == ia[0]
    assert b.launches_per_step == 8 * 2 + 2
    a.close(); b.close()
