"""-m gpu: the language-identification engine (csrc/ecapa_lid.hip) through the C ABI against tests/ecapa_lid_ref.py, which
test_ecapa_lid_cpu.py holds to numpy / scipy and torch.nn.

Gate of the model comparisons: relative rms distance of the device to the float64 reference <= FLOOR_FACTOR x the float32 reference's
own distance to the float64 reference, + SLACK (the slack of the f32 kernel family, TOL in test_gpu_q3_reference.py).  The stages are
held one after the other: stage 0 against the float64 front end over the valid frames (test_gpu_mel.py's bounds, times 10 for
10 log10; the float32 reference stays inside them on the case rows, test_ecapa_lid_cpu.py), stage 1 against the reference's
normalisation of the device's own stage 0, stages 2-9 against the reference run on the device's own stage 1.
MIS_ECAPA_LID_PARITY_LOG=<file> keeps every observed value (profiles/ecapa_lid/parity_observed.jsonl)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
import ecapa_lid_ref as er
from gpu_util import observe, record, rms
from mlx_audio_swift_amd import _lib

pytestmark = pytest.mark.gpu

FLOOR_FACTOR = 2.0
SLACK = 1e-5
LAUNCHES = 49                                                         # the seven-launch Res2Net form, published depth


def _log(row):
    path = os.environ.get("MIS_ECAPA_LID_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(row) + "\n")


def _observe(kind, value, tol):
    name = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].split("::")[-1]
    _log(dict(test=name, kind=kind, value=float(value), tol=float(tol)))
    print(f"{name} {kind}: {float(value):.3e} (tol {float(tol):.3e})")
    return observe(kind, value, tol)


def _record(name, **kw):
    _log(dict(test=name, **{k: (float(v) if isinstance(v, (int, float, np.floating, np.integer)) else v) for k, v in kw.items()}))
    record(name, **kw)


def _relrms(a, b):
    b = np.asarray(b, np.float64)
    return rms(a, b) / max(float(np.sqrt(np.mean(b ** 2))), 1e-30)


def _gate(kind, dev, ref64, ref32):
    return _observe(kind, _relrms(dev, ref64), FLOOR_FACTOR * _relrms(ref32, ref64) + SLACK)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _rows():
    return tuple(er.case_rows())


@functools.lru_cache(maxsize=None)
def _weights(name):
    return er.make_weights(er.case_config(name), er.DECISION_SEED)


@functools.lru_cache(maxsize=None)
def _model(name):
    cfg = er.case_config(name)
    return cfg, mas.EcapaTdnnLID.from_weights(cfg, _weights(name))


def _refs(name):
    cfg = er.case_config(name)
    return er.EcapaLidRef(cfg, _weights(name), torch.float32), er.EcapaLidRef(cfg, _weights(name), torch.float64)


def _stage_gates(name, dev, taps, frames, stages):
    """stages of the device against the references run on the device's own stage 1, every row's valid frames side by side"""
    r32, r64 = _refs(name)
    got = {s: [] for s in stages}
    want32, want64 = {s: [] for s in stages}, {s: [] for s in stages}
    for b, T in enumerate(frames):
        feat = torch.from_numpy(taps[1][b, :T])
        s32, s64 = r32.stages(feat), r64.stages(feat)
        for s in stages:
            got[s].append((taps[s][b, :T] if s <= 6 else taps[s][b]).ravel())
            want32[s].append(s32[s].numpy().ravel()); want64[s].append(s64[s].numpy().ravel())
    ok = {s: _gate(f"stage{s}", np.concatenate(got[s]), np.concatenate(want64[s]), np.concatenate(want32[s])) for s in stages}
    assert all(ok.values()), ok                                       # (every stage is measured before the first one fails)


@pytest.mark.parametrize("name", ["S64", "S128"])
def test_taps_of_a_ragged_batch(name):
    cfg, dev = _model(name)
    rows = _rows()
    frames = [er.frames_of(len(r)) for r in rows]
    logp = dev.predict_raw(rows)[0]
    taps = {s: dev.tap(s) for s in range(10)}
    assert np.array_equal(taps[9], logp) and taps[0].shape == (8, max(frames), 60) and taps[6].shape == (8, max(frames), 3 * cfg.channels)
    # stage 0 over the valid frames
    d = np.concatenate([(taps[0][b, :T].astype(np.float64) - er.mel_db(rows[b], 60, torch.float64).numpy()).ravel() for b, T in enumerate(frames)])
    ok = [_observe("mel_max_db", np.abs(d).max(), 2e-2), _observe("mel_share_beyond_1e-3_db", np.mean(np.abs(d) > 1e-3), 1e-3),
          _observe("mel_rms_db", np.sqrt(np.mean(d ** 2)), 2e-4)]
    # stage 1: the reference's normalisation of the device's own stage 0
    n64 = np.concatenate([er.sentence_mean_normalize(torch.from_numpy(taps[0][b, :T]).double()).numpy().ravel() for b, T in enumerate(frames)])
    n32 = np.concatenate([er.sentence_mean_normalize(torch.from_numpy(taps[0][b, :T])).numpy().ravel() for b, T in enumerate(frames)])
    ok.append(_gate("stage1", np.concatenate([taps[1][b, :T].ravel() for b, T in enumerate(frames)]), n64, n32))
    assert all(ok), ok
    assert not taps[1][7].any() and not taps[1][0].any()              # silence, and a single frame minus itself: exactly 0
    _stage_gates(name, dev, taps, frames, range(2, 10))
    for s in range(7):                                                # masks
        for b, T in enumerate(frames):
            assert not _bits(taps[s][b, T:]).any(), (s, b)


def test_a_row_does_not_depend_on_its_batch():
    cfg, dev = _model("S64")
    rows = _rows()
    together = _bits(dev.predict_raw(rows)[0])
    for b, r in enumerate(rows):
        assert np.array_equal(_bits(dev.predict_raw([r])[0][0]), together[b]), b
    for junk in (1e30, float("nan")):
        assert np.array_equal(_bits(dev.predict_raw(rows, junk=junk)[0]), together), junk


def test_forward_features_equals_predict():
    cfg, dev = _model("S64")
    rows = _rows()
    logp, emb, idx, prob = dev.predict_raw(rows, top_k=3)
    mel = dev.tap(0)
    frames = np.asarray([er.frames_of(len(r)) for r in rows], np.int32)
    l2, e2, i2, p2 = dev.forward_features(mel, frames, top_k=3)
    assert np.array_equal(_bits(l2), _bits(logp)) and np.array_equal(_bits(e2), _bits(emb))
    assert np.array_equal(i2, idx) and np.array_equal(_bits(p2), _bits(prob))
    assert np.array_equal(_bits(dev(mel, frames)), _bits(logp))


def test_decisions():
    cfg, dev = _model("S128")
    rows = _rows()
    r32, r64 = _refs("S128")
    out = dev.predict_batch(rows)
    logp, _, idx, prob = dev.predict_raw(rows, top_k=5)
    p64, p32 = [], []
    for b, r in enumerate(rows):
        want_idx, want_p = er.top_k(r32.log_probs(r), 5)
        assert idx[b].tolist() == want_idx.tolist(), (b, idx[b], want_idx)
        assert np.all(np.diff(prob[b]) <= 0)
        assert [t.language for t in out[b].top_languages] == [f"l{i:03d}" for i in want_idx] and out[b].language == f"l{want_idx[0]:03d}"
        assert out[b].confidence == float(prob[b, 0])
        p32.append(want_p)
        p64.append(torch.exp(r64.log_probs(r))[torch.from_numpy(want_idx)].numpy())
        assert np.allclose(prob[b], np.exp(logp[b, idx[b]]), rtol=1e-6, atol=0)
    assert _gate("top5_prob", prob.ravel(), np.concatenate(p64), np.concatenate(p32))
    _, _, i500, p500 = dev.predict_raw(rows[3:4], top_k=500)
    assert i500.shape == (1, 107) and sorted(i500[0].tolist()) == list(range(107)) and np.all(np.diff(p500[0]) <= 0)
    assert dev.predict(rows[3], top_k=500).top_languages[0].language == out[3].language and len(dev.predict(rows[3], top_k=500).top_languages) == 107
    assert dev.embed(rows[3:5]).shape == (2, cfg.embedding_dim)


def test_published_shape():
    cfg, dev = _model("PUB")
    rows = [_rows()[6], _rows()[4]]                                   # 16000 and 7999 samples
    frames = [er.frames_of(len(r)) for r in rows]
    dev.predict_raw(rows)
    taps = {s: dev.tap(s) for s in (1, 6, 7, 8, 9)}
    _stage_gates("PUB", dev, taps, frames, (6, 7, 8, 9))
    _record("ecapa_lid_launches", shape="PUB", launches=dev.launches)
    assert dev.launches == LAUNCHES


def test_errors_leave_the_handle_usable():
    cfg, dev = _model("S64")
    L = _lib.lib()
    pcm = np.zeros((9, 16001), np.float32)
    out = np.zeros((9, cfg.num_classes), np.float32)

    def lens(*v):
        a = np.asarray(v, np.int64)
        return a, a.ctypes.data

    def rejected(status, word):
        assert status == 3 and word in _lib.last_error(), (status, _lib.last_error())

    k1, p1 = lens(4000, 0)
    rejected(L.mis_ecapa_lid_predict(dev._h, pcm.ctypes.data, p1, 2, 16001, 5, out.ctypes.data, None, None, None), "empty")
    rejected(L.mis_ecapa_lid_predict(dev._h, pcm.ctypes.data, None, 0, 4000, 5, out.ctypes.data, None, None, None), "batch")
    rejected(L.mis_ecapa_lid_predict(dev._h, pcm.ctypes.data, None, 9, 4000, 5, out.ctypes.data, None, None, None), "batch")
    k2, p2 = lens(16001)
    rejected(L.mis_ecapa_lid_predict(dev._h, pcm.ctypes.data, p2, 1, 16001, 5, out.ctypes.data, None, None, None), "max_samples")
    rejected(L.mis_ecapa_lid_predict(dev._h, None, None, 1, 4000, 5, out.ctypes.data, None, None, None), "null")
    m = mas.EcapaTdnnLID(cfg)
    W = _weights("S64")
    for k, v in W.items():
        if k != "embedding_model.block2.se_block.conv2.bias":
            m.set_tensor(k, v)
    with pytest.raises(mas.AudioGenerationError) as e:
        m.finalize()
    assert e.value.case == "invalidInput" and "embedding_model.block2.se_block.conv2.bias" in str(e.value)
    rejected(L.mis_ecapa_lid_predict(m._h, pcm.ctypes.data, None, 1, 4000, 5, out.ctypes.data, None, None, None), "finalized")
    m.set_tensor("embedding_model.block2.se_block.conv2.bias", W["embedding_model.block2.se_block.conv2.bias"])
    m.finalize()                                                      # a rejected finalize can be repeated
    row = _rows()[3]
    assert np.array_equal(_bits(m.predict_raw([row])[0]), _bits(dev.predict_raw([row])[0]))
    m.close()


def test_model_directory_loads_like_from_weights(tmp_path):
    from safetensors.torch import save_file
    cfg, dev = _model("S64")
    body = {k: getattr(cfg, k) for k in ("n_mels", "channels", "kernel_sizes", "dilations", "attention_channels", "res2net_scale",
                                         "se_channels", "embedding_dim", "classifier_hidden_dim", "id2label")}
    (tmp_path / "config.json").write_text(json.dumps(body))
    save_file({k: v.contiguous() for k, v in er.raw_checkpoint(_weights("S64")).items()}, str(tmp_path / "model.safetensors"))
    m = mas.EcapaTdnnLID.from_model_directory(str(tmp_path), max_batch=8, max_samples=16000)
    rows = _rows()
    assert m.config.num_classes == 10 and m.id2label[3] == "l003"
    assert np.array_equal(_bits(m.predict_raw(rows)[0]), _bits(dev.predict_raw(rows)[0]))
    m.close()
