"""-m gpu: the Smart Turn engine (csrc/smartturn.hip) through the C ABI against tests/smartturn_ref.py, which test_smartturn_cpu.py holds
to transformers' WhisperEncoder and WhisperFeatureExtractor.

Gate of the encoder, pool and logit comparisons (the idiom and numbers of test_gpu_moonshine.py): relative rms distance of the device to
the reference with bf16 rounding points <= FLOOR_FACTOR x the distance of the reference's own float64-accumulation realisation to it,
+ 2e-3.  The distance to the reference WITHOUT bf16 rounding is recorded, not gated.  The stages are held one after the other: stage 0
against the float64 statistics, stage 1 against the reference's features of the device's own stage 0, the encoder and the head against
the reference run on the device's own stage 1; the decisions test holds the whole chain against the reference's own.
MIS_SMARTTURN_PARITY_LOG=<file> keeps every observed value (profiles/smartturn/parity_observed.jsonl)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
import smartturn_ref as sr
from gpu_util import observe, record, rms
from mlx_audio_swift_amd import _lib

pytestmark = pytest.mark.gpu

FLOOR_FACTOR = 2.0
SLACK = 2e-3


def _log(row):
    path = os.environ.get("MIS_SMARTTURN_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(row) + "\n")


def _observe(kind, value, tol):
    name = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].split("::")[-1]
    _log(dict(test=name, kind=kind, value=float(value), tol=float(tol)))
    return observe(kind, value, tol)


def _record(name, **kw):
    _log(dict(test=name, **{k: (float(v) if isinstance(v, (int, float, np.floating, np.integer)) else v) for k, v in kw.items()}))
    record(name, **kw)


def _relrms(a, b):
    b = np.asarray(b, np.float64)
    return rms(a, b) / max(float(np.sqrt(np.mean(b ** 2))), 1e-30)


def _gate(kind, dev, ref, floor):
    return _observe(kind, _relrms(dev, ref), FLOOR_FACTOR * _relrms(floor, ref) + SLACK)


@functools.lru_cache(maxsize=None)
def _weights(name, seed=sr.DECISION_SEED):
    return sr.make_weights(sr.case_config(name), seed=seed)


def _model(name, seed=sr.DECISION_SEED):
    cfg = sr.case_config(name)
    return cfg, mas.SmartTurnModel.from_weights(cfg, _weights(name, seed))


def _mel_close(got, ref):                                            # the tolerance of test_gpu_mel.py
    d = np.abs(got - ref)
    assert d.max() < 2e-3, d.max()
    assert np.mean(d > 1e-4) < 1e-3, np.mean(d > 1e-4)
    assert float(np.sqrt(np.mean(d.astype(np.float64) ** 2))) < 2e-5


def _encoder_and_head_gates(cfg, W, rows_idx, feats, dev_enc, dev_pooled, dev_logit, tag):
    """The three references on the device's own features; returns the conjunction of the floor gates."""
    r32, r64, ru = (sr.SmartTurnRef(cfg, W, round="bf16"), sr.SmartTurnRef(cfg, W, round="bf16", acc=torch.float64),
                    sr.SmartTurnRef(cfg, W, round=None))
    out = {k: [r.forward_features(feats[b]) for b in rows_idx] for k, r in (("d", r32), ("f", r64), ("u", ru))}
    cat = lambda key, what: np.concatenate([np.asarray(o[what], np.float64).reshape(-1) for o in out[key]])
    de, dp, dl = (np.concatenate([dev_enc[b].reshape(-1) for b in rows_idx]), np.concatenate([dev_pooled[b].reshape(-1) for b in rows_idx]),
                  np.asarray([dev_logit[b] for b in rows_idx]))
    _record("smartturn_unrounded_distance", shape=tag, enc=_relrms(de, cat("u", "enc")), pooled=_relrms(dp, cat("u", "pooled")),
            logits=_relrms(dl, cat("u", "logit")))
    ok = _gate("stage2_encoder", de, cat("d", "enc"), cat("f", "enc"))
    ok &= _gate("stage3_pooled", dp, cat("d", "pooled"), cat("f", "pooled"))
    ok &= _gate("logits", dl, cat("d", "logit"), cat("f", "logit"))
    return ok


@pytest.mark.parametrize("name", ["S64", "S128"])
def test_taps_against_the_reference(name):
    cfg, dev = _model(name)
    pc, rows = cfg.processor_config, sr.case_rows(cfg)
    prob, logit, pred = dev.predict_raw(rows)
    t0, t1, t2, t3 = (dev.tap(s) for s in range(4))
    dev.close()
    assert t0.shape == (8, cfg.window_samples) and t1.shape == (8, cfg.frames, 80) and t2.shape == (8, cfg.positions, cfg.encoder_config.d_model)
    # stage 0: the float64 statistics; the bound is what the reference's own sequential float32 sums miss them by
    p64 = np.stack([sr.prepare(r, pc, "f64") for r in rows]); pseq = np.stack([sr.prepare(r, pc, "f32seq") for r in rows])
    ok = _observe("stage0_prepared", _relrms(t0, p64), 2.0 * _relrms(pseq, p64) + 1e-6)
    assert np.array_equal(t0[6], np.zeros_like(t0[6]))                                       # an all-zero row stays all zeros
    assert np.all(t0[3, : cfg.window_samples - 1600] == t0[3, 0]) and np.abs(t1[6] + 1.5).max() < 1e-6
    for b in range(8):                                                                       # stage 1 on the device's own stage 0
        _mel_close(t1[b], sr.features(t0[b], pc))
    ok &= _encoder_and_head_gates(cfg, _weights(name), list(range(8)), t1, t2, t3, logit, name)
    assert ok


def test_published_shape():
    cfg, dev = _model("PUB")
    rows = sr.case_rows(cfg)
    rows = [rows[i] for i in (0, 1, 2, 4, 6, 7)]                                             # 6 rows: the CPU reference stays in seconds
    prob, logit, pred = dev.predict_raw(rows)
    n1 = dev.launches
    t1, t2, t3 = dev.tap(1), dev.tap(2), dev.tap(3)
    dev.predict_raw([r[: max(1, len(r) // 2)] for r in rows])
    n2 = dev.launches
    dev.close()
    assert n1 == n2 == 4 + 8 * 4 + 3, (n1, n2)
    assert _encoder_and_head_gates(cfg, _weights("PUB"), list(range(6)), t1, t2, t3, logit, "PUB")


def test_decisions_follow_the_reference_outside_the_margin():
    """The rows and weights of test_smartturn_cpu.py::test_decision_margins_leave_most_rows_decidable, the whole chain end to end."""
    name = sr.DECISION_SHAPE
    cfg, dev = _model(name)
    rows, W = sr.case_rows(cfg), _weights(name)
    r32, r64 = sr.SmartTurnRef(cfg, W, round="bf16"), sr.SmartTurnRef(cfg, W, round="bf16", acc=torch.float64)
    l32 = np.asarray([r32.forward(r)["logit"] for r in rows]); l64 = np.asarray([r64.forward(r)["logit"] for r in rows])
    m = FLOOR_FACTOR * np.abs(l64 - l32) + SLACK
    prob, logit, pred = dev.predict_raw(rows)
    for thr in (None, 0.25, 0.8):
        t = cfg.processor_config.threshold if thr is None else thr
        p_t, _, pred_t = dev.predict_raw(rows, threshold=thr)
        assert np.array_equal(p_t, prob)
        sure = np.abs(l32 - sr.threshold_logit(t)) > m
        assert (~sure).sum() <= len(rows) // 4, (t, l32, m)
        assert np.array_equal(pred_t[sure], (l32 > sr.threshold_logit(t)).astype(np.int32)[sure]), (t, pred_t, l32)
        assert np.array_equal(pred_t, (prob > np.float32(t)).astype(np.int32))               # the explicit threshold is the one applied
        _record("smartturn_decisions", threshold=t, exempt=int((~sure).sum()), worst_logit_gap=float(np.abs(logit - l32).max()))
    sig = 1.0 / (1.0 + np.exp(-logit.astype(np.float64)))
    assert np.abs(prob - sig).max() <= 2 * np.finfo(np.float32).eps, np.abs(prob - sig).max()     # probability == sigmoid(logit) to f32 rounding
    one = dev.predict_endpoint(rows[0])
    assert (one.prediction, np.float32(one.probability)) == (int(pred[0]), prob[0])
    many = dev.predict_endpoints(rows[:3], threshold=0.8)
    assert [o.prediction for o in many] == [int(p > np.float32(0.8)) for p in prob[:3]]
    dev.close()


def test_rows_do_not_depend_on_their_batch():
    cfg, dev = _model("S64")
    rows = sr.case_rows(cfg)[:7]
    prob, logit, _ = dev.predict_raw(rows)
    pj, lj, _ = dev.predict_raw(rows, junk=3.0e4)                                            # junk behind lens[b] inside the stride
    assert np.array_equal(prob, pj) and np.array_equal(logit, lj)
    for b, r in enumerate(rows):
        p1, l1, _ = dev.predict_raw([r])
        assert p1[0] == prob[b] and l1[0] == logit[b], b
    rows33 = [sr.wave(1600 + 977 * i, i) for i in range(33)]
    p33, l33, _ = dev.predict_raw(rows33)
    p32, l32, _ = dev.predict_raw(rows33[:32]); p1, l1, _ = dev.predict_raw(rows33[32:])
    assert np.array_equal(p33, np.concatenate([p32, p1])) and np.array_equal(l33, np.concatenate([l32, l1]))
    n_graph = dev.launches
    old = os.environ.get("MIS_NO_GRAPH")
    os.environ["MIS_NO_GRAPH"] = "1"                                                         # read at every call
    try:
        pn, ln, _ = dev.predict_raw(rows)
        n_plain = dev.launches
    finally:
        if old is None:
            os.environ.pop("MIS_NO_GRAPH", None)
        else:
            os.environ["MIS_NO_GRAPH"] = old
    assert np.array_equal(pn, prob) and np.array_equal(ln, logit) and n_plain == n_graph == 4 + 8 * 2 + 3
    dev.close()


def test_forward_features_reproduces_predict():
    cfg, dev = _model("S64")
    rows = sr.case_rows(cfg)[:4]
    prob, logit, _ = dev.predict_raw(rows)
    feats = dev.tap(1).transpose(0, 2, 1)                                                    # HF layout [B, n_mels, F]
    assert np.array_equal(dev(feats, return_logits=True)[:, 0], logit) and np.array_equal(dev(feats)[:, 0], prob)
    assert np.array_equal(dev(feats[1], return_logits=True)[0, 0], logit[1])
    f = dev.prepare_input_features(rows[2])
    assert f.shape == (80, cfg.frames) and np.array_equal(f, feats[2])
    dev.close()


def test_errors_leave_the_handle_usable(tmp_path):
    cfg, dev = _model("S64")
    L, W = _lib.lib(), _weights("S64")
    good = sr.wave(9000, 3)
    before = dev.predict_raw([good])
    n0 = dev.launches
    pcm = np.zeros((2, 4000), np.float32)
    out = np.zeros(65, np.float32)

    def rejected(status):
        assert status == 3 and _lib.last_error(), (status, _lib.last_error())
        assert dev.launches == n0                                                            # handle state unchanged (the count moves only with a chain that ran)
        after = dev.predict_raw([good])
        assert all(np.array_equal(a, b) for a, b in zip(before, after))

    lens = lambda *v: np.asarray(v, np.int64).ctypes.data
    rejected(L.mis_smartturn_predict(dev._h, pcm.ctypes.data, None, 0, 4000, -1.0, out.ctypes.data, None, None))
    rejected(L.mis_smartturn_predict(dev._h, pcm.ctypes.data, None, 65, 4000, -1.0, out.ctypes.data, None, None))
    rejected(L.mis_smartturn_predict(dev._h, pcm.ctypes.data, lens(4000, 0), 2, 4000, -1.0, out.ctypes.data, None, None))
    rejected(L.mis_smartturn_predict(dev._h, pcm.ctypes.data, lens(4001, 10), 2, 4000, -1.0, out.ctypes.data, None, None))
    rejected(L.mis_smartturn_predict(dev._h, None, None, 1, 4000, -1.0, out.ctypes.data, None, None))
    rejected(L.mis_smartturn_forward_features(dev._h, None, 1, out.ctypes.data, None))
    for thr in (float("nan"), 1.5):                                                          # a threshold that is no number, or above 1
        rejected(L.mis_smartturn_predict(dev._h, pcm.ctypes.data, None, 1, 4000, thr, out.ctypes.data, None, None))
    # configurations the engine does not take
    for bad in (dict(max_source_positions=99), dict(encoder_attention_heads=0), dict(d_model=96, encoder_attention_heads=2)):
        enc = mas.SmartTurnEncoderConfig(**{**cfg.encoder_config.__dict__, **bad})
        with pytest.raises(mas.AudioGenerationError) as e:
            mas.SmartTurnModel(mas.SmartTurnConfig(encoder_config=enc, max_audio_seconds=2))
        assert e.value.case == "invalidInput" and str(e.value), bad
    # predict before finalize, a missing weight, a weight of the wrong shape: the same handle then loads and predicts
    m = mas.SmartTurnModel(cfg)
    missing = "encoder.layers.1.fc2.bias"
    for k, v in W.items():
        if k != missing:
            m.set_tensor(k, v)
    assert L.mis_smartturn_predict(m._h, pcm.ctypes.data, None, 1, 4000, -1.0, out.ctypes.data, None, None) == 3 and "finalized" in _lib.last_error()
    with pytest.raises(mas.AudioGenerationError) as e:
        m.finalize()
    assert e.value.case == "invalidInput" and missing in str(e.value)
    m.set_tensor(missing, torch.zeros(7))
    with pytest.raises(mas.AudioGenerationError) as e:
        m.finalize()
    assert e.value.case == "invalidInput" and missing in str(e.value) and "shape" in str(e.value)
    m.set_tensor(missing, W[missing])
    m.finalize()
    assert all(np.array_equal(a, b) for a, b in zip(before, m.predict_raw([good])))
    m.close()
    with pytest.raises(mas.AudioGenerationError):
        dev.predict_raw([good], sample_rate=8000)                                            # no resampler in the package
    assert all(np.array_equal(a, b) for a, b in zip(before, dev.predict_raw([good])))
    dev.close()


def test_loader_reads_an_unsanitized_checkpoint(tmp_path):
    from safetensors.torch import save_file
    name = "S64"
    cfg, a = _model(name)
    e, p = cfg.encoder_config, cfg.processor_config
    (tmp_path / "config.json").write_text(json.dumps(dict(model_type="smart_turn", encoder_config=dict(e.__dict__), max_audio_seconds=p.max_audio_seconds)))
    save_file(sr.raw_checkpoint(_weights(name)), os.path.join(tmp_path, "model.safetensors"))
    b = mas.SmartTurnModel.from_pretrained(str(tmp_path))
    rows = sr.case_rows(cfg)[:3]
    ra, rb = a.predict_raw(rows), b.predict_raw(rows)
    assert all(np.array_equal(x, y) for x, y in zip(ra, rb)) and b.config.processor_config.max_audio_seconds == 2
    a.close(); b.close()
