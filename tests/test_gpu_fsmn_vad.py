"""-m gpu: the voice activity detector (csrc/fsmn_vad.hip) through the C ABI against tests/fsmn_vad_ref.py, which test_fsmn_vad_cpu.py
holds to numpy / scipy and torch.nn.

Gate of the comparisons (the f32 family's, as test_gpu_ecapa_lid.py): relative rms distance of the device to the float64 reference
<= FLOOR_FACTOR x the float32 reference's own distance to the float64 reference, + SLACK.  Every stage is compared with the reference
run on the device's own previous stage.  MIS_FSMN_VAD_PARITY_LOG=<file> keeps every observed value
(profiles/fsmn_vad/parity_observed.jsonl)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
import fsmn_vad_ref as R
from gpu_util import observe, record, rms

pytestmark = pytest.mark.gpu

FLOOR_FACTOR = 2.0
SLACK = 1e-5
LAUNCHES = 13                                                         # 5 + 2 fsmn_layers a chunk, published depth


def _log(row):
    path = os.environ.get("MIS_FSMN_VAD_PARITY_LOG")
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


@functools.lru_cache(maxsize=None)
def _rows():
    return tuple(R.case_rows())


@functools.lru_cache(maxsize=None)
def _drows():
    return tuple(R.decision_rows())


@functools.lru_cache(maxsize=None)
def _weights(name):
    cfg = R.case_config(name)
    return R.make_weights(cfg, R.DECISION_SEED), R.make_cmvn(cfg, R.DECISION_SEED)


@functools.lru_cache(maxsize=None)
def _model(name, chunk_frames=3000):
    cfg = R.case_config(name, chunk_frames=chunk_frames)
    W, cmvn = _weights(name)
    return cfg, mas.FSMNVAD.from_weights(cfg, W, cmvn)


@functools.lru_cache(maxsize=None)
def _refs(name):
    cfg = R.case_config(name)
    W, cmvn = _weights(name)
    return R.FsmnVadRef(cfg, W, cmvn, torch.float32), R.FsmnVadRef(cfg, W, cmvn, torch.float64)


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", ["S", "P"])
def test_taps_of_a_ragged_batch(name):
    cfg, dev = _model(name)
    rows = _rows()
    T = [R.frames_of(len(r)) for r in rows]
    Rr = [R.rows_of(t) for t in T]
    NL = cfg.encoder.fsmn_layers
    scores, Rdev = dev.scores_raw(rows)
    assert Rdev.tolist() == Rr and T[:5] == [0, 1, 2, 98, 109] and Rr[:5] == [0, 3, 4, 100, 111]
    taps = {s: dev.tap(s) for s in range(8 + 2 * NL)}
    assert taps[0].shape == (8, max(T), 80) and taps[2].shape == (8, max(Rr), 400) and np.array_equal(_bits(taps[6 + 2 * NL]), _bits(scores))
    # fbank and decibel against the float64 front end over the valid frames
    live = [b for b in range(8) if T[b] > 0]
    fb64 = np.concatenate([R.fbank(rows[b], 80, torch.float64).numpy().ravel() for b in live])
    fb32 = np.concatenate([R.fbank(rows[b], 80, torch.float32).numpy().ravel() for b in live])
    db64 = np.concatenate([R.decibel(rows[b], torch.float64).numpy() for b in live])
    db32 = np.concatenate([R.decibel(rows[b], torch.float32).numpy() for b in live])
    fbd = np.concatenate([taps[0][b, :T[b]].ravel() for b in live])
    dbd = np.concatenate([taps[1][b, :T[b]] for b in live])
    ok = [_gate("fbank_rms", fbd, fb64, fb32), _gate("decibel_rms", dbd, db64, db32),
          _observe("fbank_max_abs", np.abs(fbd - fb64).max(), 10 * np.abs(fb32 - fb64).max()),
          _observe("decibel_max_abs", np.abs(dbd - db64).max(), 10 * np.abs(db32 - db64).max())]
    assert all(ok), ok
    # silence: exactly log(1e-8) and -60 dB
    assert np.all(taps[0][6, :T[6]] == np.float32(np.log(np.float64(np.float32(1e-8))))) and np.all(taps[1][6, :T[6]] == np.float32(-60.0))
    # LFR + CMVN: numpy float32 on the device's own fbank, bit for bit
    cmvn = _weights(name)[1]
    for b in live:
        assert np.array_equal(_bits(taps[2][b, :Rr[b]]), _bits(R.lfr_cmvn_numpy(taps[0][b, :T[b]], cmvn))), b
    feats, Rf = dev.features_raw(rows)
    assert np.array_equal(_bits(feats), _bits(taps[2])) and Rf.tolist() == Rr
    # every encoder stage on the device's own previous stage
    r32, r64 = _refs(name)
    ok = {}
    for s in range(3, 8 + 2 * NL):
        prev = 5 + 2 * NL if s == 7 + 2 * NL else s - 1
        got = np.concatenate([taps[s][b, :Rr[b]].ravel() for b in live])
        w32 = np.concatenate([r32.step(s, torch.from_numpy(taps[prev][b, :Rr[b]])).numpy().ravel() for b in live])
        w64 = np.concatenate([r64.step(s, torch.from_numpy(taps[prev][b, :Rr[b]])).numpy().ravel() for b in live])
        ok[s] = _gate(f"stage{s}", got, w64, w32)
    assert all(ok.values()), ok
    # end to end: the scores against the float64 reference on the waveform (recorded, not gated: the fbank's log amplifies the f32 front end)
    e2e = np.concatenate([(scores[b, :Rr[b]] - r64.scores(rows[b]).numpy()).ravel() for b in live])
    record("fsmn_vad_scores_end_to_end", shape=name, max_abs=float(np.abs(e2e).max()))
    # masks
    for s in range(8 + 2 * NL):
        for b in range(8):
            n = T[b] if s <= 1 else Rr[b]
            assert not _bits(taps[s][b, n:]).any(), (s, b)


# ---------------------------------------------------------------------------------------------- 2
def test_a_row_does_not_depend_on_its_batch():
    cfg, dev = _model("S")
    rows = _rows()
    sil, dec, Rr, T = dev.detect_raw(rows)
    scores = dev.scores_raw(rows)[0]
    for b, r in enumerate(rows):
        s1, d1, R1, T1 = dev.detect_raw([r])
        assert np.array_equal(_bits(s1[0]), _bits(sil[b, :Rr[b]])) and np.array_equal(_bits(d1[0]), _bits(dec[b, :T[b]])), b
        assert np.array_equal(_bits(dev.scores_raw([r])[0][0]), _bits(scores[b, :Rr[b]])), b
    for junk in (1e30, float("nan")):
        s2, d2, _, _ = dev.detect_raw(rows, junk=junk)
        assert np.array_equal(_bits(s2), _bits(sil)) and np.array_equal(_bits(d2), _bits(dec)), junk
        assert np.array_equal(_bits(dev.scores_raw(rows, junk=junk)[0]), _bits(scores)), junk


# ---------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("name", ["S", "P"])
def test_chunking_is_exact(name):
    row = _rows()[5]                                                  # 3.01 s: 299 frames, 301 LFR rows
    others = [_rows()[3]]
    _, whole = _model(name, 512)
    want = (whole.scores_raw([row] + others)[0],) + whole.detect_raw([row] + others)[:2]
    assert whole.launches == 5 + 2 * whole.config.encoder.fsmn_layers
    for chunk in (32, 64):
        _, dev = _model(name, chunk)
        got = (dev.scores_raw([row] + others)[0],) + dev.detect_raw([row] + others)[:2]
        for a, b in zip(got, want):
            assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), chunk
        assert dev.launches == (5 + 2 * dev.config.encoder.fsmn_layers) * -(-301 // chunk)


# ---------------------------------------------------------------------------------------------- 4
def test_decisions():
    cfg, dev = _model("P")
    rows = _drows()
    r32, _ = _refs("P")
    NL = cfg.encoder.fsmn_layers
    sil, dec, Rr, T = dev.detect_raw(rows)
    feats = dev.features_raw(rows)[0]
    segs = dev.detect_batch(rows)
    thr = np.float32(cfg.speech_noise_thres)
    ref_sil = [r32.stages(torch.from_numpy(feats[b, :Rr[b]]))[7 + 2 * NL].numpy() for b in range(8)]
    e = max(float(np.abs(sil[b, :Rr[b]] - ref_sil[b]).max()) for b in range(8))
    _observe("silence_max_abs", e, 1e-4)
    exempt, frames, clean_rows = 0, 0, 0
    for b in range(8):
        s, d = sil[b, :Rr[b]], dec[b, :T[b]]
        unsure = np.abs(1.0 - 2.0 * ref_sil[b].astype(np.float64) - float(thr)) < 4 * e + 1e-6
        got, want = R.speech_flags(s, d, thr), R.speech_flags(ref_sil[b], d, thr)
        sure = ~unsure[: len(got)]
        assert np.array_equal(got[sure], want[sure]), b
        if not unsure.any():
            clean_rows += 1
            assert segs[b] == mas.fsmn_vad_postprocess(ref_sil[b], d, len(rows[b]), cfg), b
        assert segs[b] == R.swift_segments(cfg, s, d, len(rows[b])), b
        exempt += int(unsure.sum()); frames += len(unsure)
    record("fsmn_vad_decisions", exempt=exempt, frames=frames, clean_rows=clean_rows, silence_max_abs=e)
    assert exempt <= 0.01 * frames and clean_rows >= 4
    assert len(segs[0]) == 2 and segs[1] == [] and segs[2][-1][1] == Rr[2] * 10
    assert dev.detect(rows[0]) == segs[0]


# ---------------------------------------------------------------------------------------------- 5
def test_call_on_the_reference_fixture():
    cfg, dev = _model("P")
    r32, r64 = _refs("P")
    NL = cfg.encoder.fsmn_layers
    feats = ((np.arange(6 * 400) % 101 - 50) / 50.0).astype(np.float32).reshape(1, 6, 400)
    out = dev(feats)
    assert out.shape == (1, 6, 248) and np.abs(out.sum(-1) - 1.0).max() < 1e-5
    w32, w64 = r32.stages(torch.from_numpy(feats[0]))[6 + 2 * NL].numpy(), r64.stages(torch.from_numpy(feats[0]))[6 + 2 * NL].numpy()
    assert _gate("call_scores", out[0], w64, w32)
    assert dev.launches == LAUNCHES - 1                               # no front end
    two = dev(np.concatenate([feats, feats[:, ::-1]], 0), counts=[6, 4])
    assert np.array_equal(_bits(two[0]), _bits(out[0])) and not two[1, 4:].any()


# ---------------------------------------------------------------------------------------------- 6
def test_launch_count():
    cfg, dev = _model("P")
    rows = _rows()
    dev.detect_raw(rows[3:4])
    one = dev.launches
    dev.detect_raw(rows)
    record("fsmn_vad_launches", shape="P", launches=dev.launches)
    assert one == dev.launches == LAUNCHES == 5 + 2 * cfg.encoder.fsmn_layers


# ---------------------------------------------------------------------------------------------- 7
def test_errors_and_empty_input():
    cfg, dev = _model("S")
    rows = _rows()
    with pytest.raises(mas.AudioGenerationError) as e:
        dev.detect(rows[3], sample_rate=8000)
    assert "resample" in str(e.value)
    with pytest.raises(mas.AudioGenerationError) as e:
        dev.detect_raw([rows[1]] * 9)
    assert "batch" in str(e.value)
    W, cmvn = _weights("S")
    m = mas.FSMNVAD(cfg)
    with pytest.raises(mas.AudioGenerationError) as e:
        m.detect_raw([rows[3]])
    assert "finalized" in str(e.value)
    for k, v in W.items():
        if k != "fsmn.1.affine.bias":
            m.set_tensor(k, v)
    with pytest.raises(mas.AudioGenerationError) as e:
        m.finalize()
    assert "fsmn.1.affine.bias" in str(e.value)
    m.set_tensor("fsmn.1.affine.bias", W["fsmn.1.affine.bias"])
    m.finalize()                                                      # a rejected finalize can be repeated; no CMVN on this handle
    assert m.detect_raw([rows[3]])[0].shape == (1, 100)
    m.close()
    with pytest.raises(mas.AudioGenerationError):
        mas.FSMNVAD.from_weights(cfg, {k: v for k, v in W.items() if k != "in_linear1.bias"})
    import copy
    bad = copy.deepcopy(cfg)
    bad.encoder.lstride = 2
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.FSMNVAD(bad)
    assert "lstride" in str(e.value)
    assert dev.detect_batch([rows[0], np.zeros(0, np.float32), rows[0][:100]]) == [[], [], []] and dev.launches == 0
    assert dev.extract_features(rows[0]).shape == (0, 400) and dev.detect(rows[0]) == []


# ---------------------------------------------------------------------------------------------- 8
def test_model_directory_loads_like_from_weights(tmp_path):
    from dataclasses import asdict
    from safetensors.torch import save_file
    cfg, dev = _model("S")
    W, cmvn = _weights("S")
    body = {k: v for k, v in asdict(cfg).items() if k not in ("max_batch", "chunk_frames")}
    rows = _rows()
    want = dev.scores_raw(rows)[0]
    for kind in ("am.mvn", "cmvn.json"):
        d = tmp_path / kind.replace(".", "_")
        d.mkdir()
        (d / "config.json").write_text(json.dumps(body))
        save_file({"encoder." + k: v.contiguous() for k, v in W.items()}, str(d / "model.safetensors"))
        if kind == "am.mvn":
            fmt = lambda a: " ".join(repr(float(v)) for v in a)
            (d / kind).write_text(f"<Nnet>\n<AddShift> 400 400\n<LearnRateCoef> 0 [ {fmt(cmvn[0])} ]\n<Rescale> 400 400\n"
                                  f"<LearnRateCoef> 0 [ {fmt(cmvn[1])} ]\n</Nnet>\n")
        else:
            (d / kind).write_text(json.dumps({"shift": [float(v) for v in cmvn[0]], "scale": [float(v) for v in cmvn[1]]}))
            (d / "am.mvn").write_text("<AddShift> [ 1 2 ] <Rescale> [ 3 4 ]")       # cmvn.json wins
        m = mas.FSMNVAD.from_pretrained(str(d), max_batch=8)
        assert m.config.encoder.lorder == 3 and np.array_equal(_bits(m.scores_raw(rows)[0]), _bits(want)), kind
        m.close()


# ---------------------------------------------------------------------------------------------- 9
def test_long_row():
    cfg, dev = _model("P")
    r32, r64 = _refs("P")
    NL = cfg.encoder.fsmn_layers
    g = torch.Generator().manual_seed(21)
    row = R.burst_row(g, 60.0, [(1.0, 9.0), (12.0, 12.2), (20.0, 41.5), (50.0, 60.0)])
    sil, dec, Rr, T = dev.detect_raw([row])
    assert Rr[0] == 6000 and dev.launches == 2 * LAUNCHES             # two chunks of 3000
    feats = torch.from_numpy(dev.features_raw([row])[0][0])
    assert _gate("long_row_silence", sil[0], r64.stages(feats)[7 + 2 * NL].numpy(), r32.stages(feats)[7 + 2 * NL].numpy())
    segs = dev.detect(row)
    assert segs == R.swift_segments(cfg, sil[0], dec[0], len(row)) and len(segs) >= 3
