"""-m gpu: Silero VAD (csrc/silero_vad.hip) through the C ABI against tests/silero_vad_ref.py, which test_silero_vad_cpu.py holds to
torch.nn.Conv1d / torch.nn.LSTM and the literal index lists.

Gate of the comparisons (the f32 family's, as test_gpu_fsmn_vad.py): relative rms distance of the device to the float64 reference
<= FLOOR_FACTOR x the float32 reference's own distance to the float64 reference, + SLACK.  Every stage is compared with the reference
run on the device's own previous stage.  MIS_SILERO_VAD_PARITY_LOG=<file> keeps every observed value
(profiles/silero_vad/parity_observed.jsonl)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
import silero_vad_ref as R
from gpu_util import observe, record, rms

pytestmark = pytest.mark.gpu

FLOOR_FACTOR = 2.0
SLACK = 1e-5
LAUNCHES = 7                                                          # STFT, conv1..conv4, Wx, the recurrence - a pass
NAMES = ["16k", "8k", "S"]


def _observe(kind, value, tol):
    name = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].split("::")[-1]
    path = os.environ.get("MIS_SILERO_VAD_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(test=name, kind=kind, value=float(value), tol=float(tol))) + "\n")
    print(f"{name} {kind}: {float(value):.3e} (tol {float(tol):.3e})")
    return observe(kind, value, tol)


def _relrms(a, b):
    b = np.asarray(b, np.float64)
    return rms(a, b) / max(float(np.sqrt(np.mean(b ** 2))), 1e-30)


def _gate(kind, dev, ref64, ref32):
    return _observe(kind, _relrms(dev, ref64), FLOOR_FACTOR * _relrms(ref32, ref64) + SLACK)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _weights(name):
    return R.make_weights(R.case_config(name), R.DECISION_SEED)


@functools.lru_cache(maxsize=None)
def _model(name, max_chunks=1024):
    cfg = R.case_config(name, max_chunks=max_chunks)
    return cfg, mas.SileroVAD.from_weights(cfg, _weights(name))


@functools.lru_cache(maxsize=None)
def _refs(name):
    return R.case_ref(name, _weights(name), torch.float32), R.case_ref(name, _weights(name), torch.float64)


@functools.lru_cache(maxsize=None)
def _rows(name):
    return tuple(R.case_rows(R.case_config(name).branch(R.case_rate(name)).chunk_size))


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", NAMES)
def test_taps_of_a_ragged_batch(name):
    cfg, dev = _model(name)
    rate, rows = R.case_rate(name), _rows(name)
    r32, r64 = _refs(name)
    probs = dev.predict_proba_batch(rows, rate)
    nc = [len(p) for p in probs]
    assert nc == [1, 1, 1, 2, 6] == dev.chunks([len(r) for r in rows], rate).tolist() and dev.launches == LAUNCHES
    taps = [dev.tap(s) for s in range(7)]
    frames, widths = [r64.F, r64.F, r64.F2, r64.S, r64.S, r64.S], [r64.b.cutoff, 128, 64, 64, 128, 512]
    for s in range(6):
        assert taps[s].shape == (5, 6, frames[s], widths[s]), (s, taps[s].shape)
    assert taps[6].shape == (5, 6) and all(_same(taps[6][b, : nc[b]], probs[b]) for b in range(5))
    assert dev.tap("gates").shape == taps[5].shape
    ok = {}
    for s in range(6):
        prev = [r64.windows(rows[b]) if s == 0 else torch.from_numpy(taps[s - 1][b, : nc[b]]) for b in range(5)]
        got = np.concatenate([taps[s][b, : nc[b]].ravel() for b in range(5)])
        w32 = np.concatenate([r32.step(s, p).numpy().ravel() for p in prev])
        w64 = np.concatenate([r64.step(s, p).numpy().ravel() for p in prev])
        ok[s] = _gate(f"stage{s}", got, w64, w32)
    # the recurrence on the device's own gate pre-activations, from the zero state
    got = np.concatenate(probs)
    w32 = np.concatenate([r32.recur(torch.from_numpy(taps[5][b, : nc[b]]))[0].numpy() for b in range(5)])
    w64 = np.concatenate([r64.recur(torch.from_numpy(taps[5][b, : nc[b]]))[0].numpy() for b in range(5)])
    ok[6] = _gate("stage6", got, w64, w32)
    assert all(ok.values()), ok
    e2e = np.concatenate([probs[b] - r64.predict(rows[b])[0].numpy() for b in range(5)])
    record("silero_vad_probs_end_to_end", shape=name, max_abs=float(np.abs(e2e).max()))
    for s in range(7):                                                # zeros behind a row's own chunks
        for b in range(5):
            assert not _bits(taps[s][b, nc[b]:]).any(), (s, b)


# ---------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("name", NAMES)
def test_bit_identity(name):
    cfg, dev = _model(name)
    rate = R.case_rate(name)
    b = cfg.branch(rate)
    g = torch.Generator().manual_seed(17)
    row = R._noise(g, 6 * b.chunk_size + 17, 0.1)                     # 7 chunks
    (alone,), st_alone = dev.predict_proba_batch([row], rate, return_state=True)
    assert len(alone) == 7
    # in a batch of 8 with junk beyond every length
    others = [R._noise(g, n, 0.1) for n in (1, b.chunk_size, 3 * b.chunk_size + 5, 9 * b.chunk_size, 40, 2 * b.chunk_size - 1, 5 * b.chunk_size)]
    for junk in (1e30, float("nan")):
        for at in (0, 5):
            batch = others[:at] + [row] + others[at:]
            out, st = dev.predict_proba_batch(batch, rate, junk=junk, return_state=True)
            assert _same(out[at], alone) and _same(st[:, at], st_alone[:, 0]), (junk, at)
    # three passes of max_chunks = 3
    _, small = _model(name, 3)
    (split,), st_split = small.predict_proba_batch([row], rate, return_state=True)
    assert _same(split, alone) and _same(st_split, st_alone) and small.launches == 3 * LAUNCHES
    # chunk by chunk through feed
    padded = np.concatenate([row, np.zeros(7 * b.chunk_size - len(row), np.float32)])
    state, fed = None, []
    for j in range(7):
        p, state = dev.feed(padded[j * b.chunk_size: (j + 1) * b.chunk_size], state, rate)
        assert p.shape == (1, 1) and dev.launches == LAUNCHES
        fed.append(p[0, 0])
    assert _same(np.asarray(fed, np.float32), alone) and _same(state.lstm_state, st_alone)
    assert state.sample_rate == rate and np.array_equal(state.context[0], padded[-b.context_size:])
    # state=None against an explicit zero state
    (zero,), st_zero = dev.predict_proba_batch([row], rate, state=np.zeros((2, 1, 128), np.float32), return_state=True)
    assert _same(zero, alone) and _same(st_zero, st_alone)
    w = np.concatenate([np.zeros(b.context_size, np.float32), row[: b.chunk_size]])
    p0, s0 = dev(w, None, rate)
    p1, s1 = dev(w[None], np.zeros((2, 1, 128), np.float32), rate)
    assert _same(p0, p1) and _same(s0, s1) and _same(p0[0], alone[:1])
    # two half-rows chained through the state: the second half's first window starts with the first half's last `context` samples, so
    # the second half is fed from a streaming state that carries them (the next test chains two predict calls)
    (first,), st_first = dev.predict_proba_batch([row[: 3 * b.chunk_size]], rate, return_state=True)
    state, rest = mas.SileroVADStreamingState(st_first, row[None, 3 * b.chunk_size - b.context_size: 3 * b.chunk_size], rate), []
    for j in range(3, 7):
        p, state = dev.feed(padded[j * b.chunk_size: (j + 1) * b.chunk_size], state, rate)
        rest.append(p[0, 0])
    assert _same(np.concatenate([first, np.asarray(rest, np.float32)]), alone) and _same(state.lstm_state, st_alone)


def test_two_half_rows_through_state_when_the_context_is_silent():
    """predict(state=...) continues a row exactly where the cut leaves `context` zeros in front of the second half."""
    cfg, dev = _model("16k")
    b = cfg.branch16k
    g = torch.Generator().manual_seed(23)
    row = R._noise(g, 7 * b.chunk_size - 100, 0.1)
    row[3 * b.chunk_size - b.context_size: 3 * b.chunk_size] = 0.0
    (whole,), st_whole = dev.predict_proba_batch([row], 16000, return_state=True)
    (first,), st_first = dev.predict_proba_batch([row[: 3 * b.chunk_size]], 16000, return_state=True)
    (second,), st_second = dev.predict_proba_batch([row[3 * b.chunk_size:]], 16000, state=st_first, return_state=True)
    assert _same(np.concatenate([first, second]), whole) and _same(st_second, st_whole)


# ---------------------------------------------------------------------------------------------- 3
def test_long_row():
    cfg, dev = _model("16k")
    r32, r64 = _refs("16k")
    g = torch.Generator().manual_seed(21)
    row = R.burst_row(g, 2000 * 512 / 16000.0, [(1.0, 9.0), (12.0, 12.2), (20.0, 41.5), (50.0, 63.0)])
    assert len(row) == 2000 * 512
    probs = dev.predict_proba(row)
    assert probs.shape == (2000,) and dev.launches == 2 * LAUNCHES    # two passes of 1024
    assert _gate("long_row_probs", probs, r64.predict(row)[0].numpy(), r32.predict(row)[0].numpy())
    _, one = _model("16k", 2048)
    assert _same(one.predict_proba(row), probs) and one.launches == LAUNCHES


# ---------------------------------------------------------------------------------------------- 4
def test_decisions():
    cfg, dev = _model("16k")
    r32, r64 = _refs("16k")
    rows = R.decision_rows()
    probs = dev.predict_proba_batch(rows)
    seg_cfg = mas.SpeechSegmentConfig()
    exempt = chunks = clean = 0
    worst = 0.0
    for b, x in enumerate(rows):
        p64, p32 = r64.predict(x)[0].numpy(), r32.predict(x)[0].numpy()
        e = R.exempt_chunks(p64, p32)
        exempt += int(e.sum()); chunks += len(e)
        worst = max(worst, float(np.abs(probs[b] - p64).max()))
        for t in (np.float32(0.5), max(np.float32(0.5) - np.float32(0.15), np.float32(0.01))):
            assert np.array_equal((probs[b] >= t)[~e], (p64 >= float(t))[~e]), (b, t)
        if not e.any():
            clean += 1
            want = R.swift_probs_to_timestamps(p32, len(x), 16000, cfg.threshold, cfg.min_speech_duration_ms, cfg.min_silence_duration_ms,
                                               cfg.speech_pad_ms)
            assert dev.get_speech_timestamps(x) == want, b
            got = mas.segment_speech(x, 16000, dev, seg_cfg)
            ref = R.swift_segment_speech(x, p32, 16000, seg_cfg)
            assert len(got) == len(ref) and all(off == o and np.array_equal(seg, x[s:e_]) for (seg, off), (s, e_, o) in zip(got, ref)), b
    record("silero_vad_decisions", exempt=exempt, chunks=chunks, clean_rows=clean, probs_max_abs=worst)
    assert exempt <= 0.02 * chunks and clean >= 4
    assert dev.get_speech_timestamps(rows[1]) == [] and len(mas.segment_speech(rows[1], 16000, dev)) == 1
    assert len(dev.get_speech_timestamps(rows[3])) == 3


# ---------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("name", NAMES)
def test_launch_count(name):
    cfg, dev = _model(name)
    rate, rows = R.case_rate(name), _rows(name)
    dev.predict_proba_batch(rows[4:], rate)
    one = dev.launches
    dev.predict_proba_batch(rows, rate)
    record("silero_vad_launches", shape=name, launches=dev.launches)
    assert one == dev.launches == LAUNCHES
    dev(np.zeros(cfg.branch(rate).window, np.float32), None, rate)
    assert dev.launches == LAUNCHES
    fe, rec = dev.timing()
    assert fe > 0.0 and rec > 0.0


# ---------------------------------------------------------------------------------------------- 6
def test_errors_leave_the_handle_usable():
    cfg, dev = _model("16k")
    rows = _rows("16k")
    want = dev.predict_proba(rows[4])

    def usable():
        assert _same(dev.predict_proba(rows[4]), want)

    for call in (lambda: dev.predict_proba(rows[4], sample_rate=22050), lambda: dev.initial_state(1, 22050),
                 lambda: dev(np.zeros(576, np.float32), None, 22050), lambda: dev.feed(np.zeros(512, np.float32), None, 22050)):
        with pytest.raises(mas.SileroVADError) as e:
            call()
        assert e.value.kind == "unsupportedSampleRate"
        usable()
    with pytest.raises(mas.SileroVADError) as e:
        dev.feed(np.zeros((1, 256), np.float32), sample_rate=16000)
    assert e.value.kind == "unexpectedChunkSize" and "Expected 512 samples per chunk, got 256" in str(e.value)
    usable()
    st = dev.initial_state(1, 8000)
    assert st.context.shape == (1, 32) and st.lstm_state is None and st.sample_rate == 8000 and dev.initial_state().context.shape == (1, 64)
    with pytest.raises(mas.SileroVADError) as e:
        dev.feed(np.zeros(512, np.float32), st, 16000)
    assert e.value.kind == "stateSampleRateMismatch"
    usable()
    with pytest.raises(mas.AudioGenerationError) as e:
        dev.predict_proba_batch([rows[2]] * 9)
    assert "batch" in str(e.value)
    usable()
    for n in (64, 10):
        with pytest.raises(mas.SileroVADError) as e:
            dev(np.zeros(n, np.float32))
        assert e.value.kind == "insufficientReflectPadInput"
    usable()
    with pytest.raises(mas.AudioGenerationError):
        dev(np.zeros(500, np.float32))                                # longer than pad, but no window of the engine
    with pytest.raises(mas.AudioGenerationError):
        dev(np.zeros(576, np.float32), np.zeros((2, 2, 128), np.float32))
    usable()
    # an empty row returns an empty result
    assert dev.predict_proba(np.zeros(0, np.float32)).shape == (0,) and dev.predict_proba(np.zeros((3, 0), np.float32)).shape == (3, 0)
    out = dev.predict_proba_batch([np.zeros(0, np.float32), rows[4], np.zeros(0, np.float32)])
    assert [len(p) for p in out] == [0, 6, 0] and _same(out[1], want)
    out, st = dev.predict_proba_batch([np.zeros(0, np.float32)], state=np.ones((2, 1, 128), np.float32), return_state=True)
    assert len(out[0]) == 0 and dev.launches == 0 and np.all(st == 1.0)
    assert dev.get_speech_timestamps(np.zeros(0, np.float32)) == []
    # the C side judges a configuration and a tensor by itself
    bad = mas.SileroVADConfig(branch16k=mas.SileroVADBranchConfig(pad=600))
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.SileroVAD(bad)
    assert "Reflect padding of 600 requires more than 600 samples (got 576)" in str(e.value)
    W = _weights("16k")
    m = mas.SileroVAD(cfg)
    with pytest.raises(mas.AudioGenerationError) as e:
        m.predict_proba(rows[4])
    assert "finalized" in str(e.value)
    for k, v in W.items():
        if k != "branch8k.lstm.Wh":
            m.set_tensor(k, v)
    with pytest.raises(mas.AudioGenerationError) as e:
        m.set_tensor("branch16k.lstm.Wh", W["branch16k.lstm.Wh"])
    assert "set twice" in str(e.value)
    with pytest.raises(mas.AudioGenerationError) as e:
        m.set_tensor("branch8k.lstm.Wh", W["branch8k.lstm.Wh"].t().contiguous()[:, :100])
    assert "wrong shape" in str(e.value)
    with pytest.raises(mas.AudioGenerationError) as e:
        m.set_tensor("branch16k.conv5.weight", W["branch16k.conv4.weight"])
    assert "unexpected tensor" in str(e.value)
    with pytest.raises(mas.AudioGenerationError) as e:
        m.finalize()
    assert "branch8k.lstm.Wh" in str(e.value)
    m.set_tensor("branch8k.lstm.Wh", W["branch8k.lstm.Wh"])
    m.finalize()                                                      # a rejected finalize can be repeated
    assert _same(m.predict_proba(rows[4]), want)
    m.close()
    usable()


# ---------------------------------------------------------------------------------------------- 7
def test_model_directory_loads_like_from_weights(tmp_path):
    from safetensors.torch import save_file
    cfg, dev = _model("S")
    W = _weights("S")
    rows = _rows("S")
    want16, want8 = dev.predict_proba_batch(rows, 16000), dev.predict_proba_batch(rows, 8000)
    raw = {k.replace("branch16k.", "vad_16k.").replace("branch8k.", "vad_8k."): v.contiguous() for k, v in W.items()}
    names = sorted(raw)
    body = {"branch_16k": R.SMALL, "threshold": 0.5}

    def write(d, tensors):
        d.mkdir()
        (d / "config.json").write_text(json.dumps(body))
        half = len(tensors) // 2
        keys = sorted(tensors)
        save_file({k: tensors[k] for k in keys[:half]}, str(d / "model-00001.safetensors"))
        save_file({**{k: tensors[k] for k in keys[half:]}, "val_loss": torch.zeros(1), "val_acc": torch.ones(1)}, str(d / "model-00002.safetensors"))
        return str(d)

    m = mas.SileroVAD.from_pretrained(write(tmp_path / "good", raw), max_batch=8)
    assert m.config.branch16k.chunk_size == 224
    assert all(_same(a, b) for a, b in zip(m.predict_proba_batch(rows, 16000), want16))
    assert all(_same(a, b) for a, b in zip(m.predict_proba_batch(rows, 8000), want8))
    m.close()
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.SileroVAD.from_model_directory(write(tmp_path / "missing", {k: v for k, v in raw.items() if k != names[3]}))
    assert "missing keys" in str(e.value)
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.SileroVAD.from_model_directory(write(tmp_path / "misshapen", {**raw, "vad_8k.lstm.bias": torch.zeros(511)}))
    assert "vad_8k" not in str(e.value) and "branch8k.lstm.bias has shape" in str(e.value)


def test_synthetic_runs():
    m = mas.SileroVAD.synthetic(mas.SileroVADConfig(max_batch=2, max_chunks=16))
    p = m.predict_proba(np.zeros((2, 1000), np.float32), 8000)
    assert p.shape == (2, 4) and np.all((p > 0) & (p < 1)) and _same(p[0], p[1])
    m.close()
