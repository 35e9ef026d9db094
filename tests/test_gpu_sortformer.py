"""Sortformer on the device (csrc/sortformer.hip) against tests/sortformer_ref.py.  The engine is exact f32, so every stage is gated as
tests/test_gpu_mossformer2.py gates its f32 stages: relative rms against the float64 reference <= FLOOR_FACTOR x the float32
reference's own distance to the float64 reference, + SLACK.  Every stage is compared with the reference run on the device's own
previous stage.  MIS_SORTFORMER_PARITY_LOG=<file> keeps every observed value (profiles/sortformer/parity_observed.jsonl)."""
import functools
import json
import os
from dataclasses import asdict

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
import sortformer_ref as R
from gpu_util import observe, rms

pytestmark = pytest.mark.gpu

FLOOR_FACTOR = 2.0                 # the constants of tests/test_gpu_mossformer2.py
SLACK = 1e-5


def launches(cfg, call="forward"):
    """include/mi_speech.h: 15 launches a Conformer block, 7 a BART layer; 11 around them from samples, 8 from features, 4 from embeddings."""
    return {"forward": 11, "forward_features": 8, "encode_embeddings": 4}[call] + 15 * cfg.fc_encoder_config.num_hidden_layers \
        + 7 * cfg.tf_encoder_config.encoder_layers


def _observe(kind, value, tol):
    name = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].split("::")[-1]
    path = os.environ.get("MIS_SORTFORMER_PARITY_LOG")
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


def _cat(parts):
    return np.concatenate([np.asarray(p, np.float64).ravel() for p in parts])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_OPEN = []


@functools.lru_cache(maxsize=None)
def _model(name, **modules):
    cfg = R.case_config(name, **modules)
    W = R.synthetic_weights(cfg, 5, R.HEAD_GAIN)
    _OPEN.append(mas.SortformerModel.from_weights(cfg, W))
    return cfg, _OPEN[-1], R.Ref(cfg, W, torch.float32), R.Ref(cfg, W, torch.float64), W


@pytest.fixture(scope="module", autouse=True)
def _release_handles():
    yield
    while _OPEN:
        _OPEN.pop().close()
    _model.cache_clear()


def _chain_ok(tag, dev, r32, r64, T, stages):
    """every stage >= 1 of `stages` against the references run on the device's previous stage, the rows' own frames only"""
    taps = {s: dev.tap(s) for s in sorted(set(stages) | {s - 1 for s in stages})}
    ok = []
    for s in stages:
        both = [[r.stage_after(s, taps[s - 1][b, :T[b]]).numpy() for b in range(len(T))] for r in (r64, r32)]
        ok.append(_gate(f"{tag}stage{s}_rms", _cat(taps[s][b, :T[b]] for b in range(len(T))), _cat(both[0]), _cat(both[1])))
        assert all(not taps[s][b, T[b]:].any() for b in range(len(T))), f"stage {s}: rows behind a row's count are not zero"
    return ok, taps


def _n_for_T(T):
    """a sample count whose row has exactly T diarization frames without frame padding: F = 8 T - 3"""
    return (8 * T - 4) * 160 + 7


def test_features_of_a_ragged_batch():
    cfg, dev, r32, r64, _ = _model("A")
    rows = [R.test_wave(s, n) for s, n in ((1, 16000), (2, 5000), (3, 24321))]
    mels = cfg.fc_encoder_config.num_mel_bins
    ok = []
    for peak, norm, pad in ((True, True, 16), (False, False, 0), (True, True, 0)):
        got = dev.features(rows, peak_normalize=peak, normalize=norm, pad_to=pad)
        F, _ = dev.frames([len(r) for r in rows], pad)
        assert dev.launches == 3 and got.shape == (3, int(F.max()), mels)
        ref = [[R.features(r, mels, dt, peak, norm, pad).numpy() for r in rows] for dt in (torch.float64, torch.float32)]
        assert [len(x) for x in ref[0]] == F.tolist()
        ok.append(_gate(f"features_{int(peak)}{int(norm)}{pad}_rms", _cat(got[b, :F[b]] for b in range(3)), _cat(ref[0]), _cat(ref[1])))
        assert all(not got[b, F[b]:].any() for b in range(3))
    assert all(ok)


@pytest.mark.parametrize("name", ["A", "B"])
def test_taps_of_a_ragged_batch(name):
    cfg, dev, r32, r64, _ = _model(name)
    rows = [R.test_wave(20 + i, int(16000 * s)) for i, s in enumerate((1.0, 2.3, 3.7, 5.1, 6.5))]
    feats = dev.features(rows)
    probs = dev.forward(rows)
    F, T = dev.frames([len(r) for r in rows])
    assert dev.launches == launches(cfg) and probs.shape == (5, int(T.max()), 4)
    L, Lt = cfg.fc_encoder_config.num_hidden_layers, cfg.tf_encoder_config.encoder_layers
    stem = [[r.pre_encode(torch.as_tensor(feats[b, :F[b]]).to(r.dtype)).numpy() for b in range(5)] for r in (r64, r32)]
    ok, taps = _chain_ok("", dev, r32, r64, T, list(range(1, L + Lt + 3)))
    ok.append(_gate("stem_rms", _cat(taps[0][b, :T[b]] for b in range(5)), _cat(stem[0]), _cat(stem[1])))
    assert np.array_equal(_bits(taps[L + Lt + 2]), _bits(probs))
    assert all(ok)


@pytest.mark.parametrize("name,Ts", [("A", (1, 2, 31, 32, 33, 63, 64, 65, 97)), ("B", (1, 2, 31, 32, 33, 63, 64, 65, 97)),
                                     ("A", (3, 8, 9, 10, 4, 5, 6)), ("B", (2, 4, 5, 6, 3))])
def test_attention_and_depthwise_edges(name, Ts):
    """T_b around the 32-key tile, the 64-query block, the tap count and the 64-frame tile of the depthwise conv"""
    cfg, dev, r32, r64, _ = _model(name)
    rows = [R.test_wave(40 + T, _n_for_T(T)) for T in Ts]
    probs = dev.forward(rows, pad_to=0)
    _, T = dev.frames([len(r) for r in rows], 0)
    assert T.tolist() == list(Ts)
    L, Lt = cfg.fc_encoder_config.num_hidden_layers, cfg.tf_encoder_config.encoder_layers
    ok, taps = _chain_ok("edge_", dev, r32, r64, T, [1, 2, L + 2, L + Lt + 2])
    assert np.array_equal(_bits(taps[L + Lt + 2]), _bits(probs)) and all(ok)


@pytest.mark.parametrize("name", ["A", "B"])
def test_stem_edges(name):
    """F_b 16 / 32 / 48 and lengths whose halves are odd"""
    cfg, dev, r32, r64, _ = _model(name)
    Fs = [16, 32, 48, 21, 37, 1, 2, 47]
    rng = np.random.default_rng(7)
    feats = rng.standard_normal((len(Fs), 48, cfg.fc_encoder_config.num_mel_bins)).astype(np.float32)      # junk behind a row's frames
    emb = dev.pre_encode(feats, Fs)
    assert dev.launches == 4
    T = [R.diar_frames(F) for F in Fs]
    ref = [[r.pre_encode(torch.as_tensor(feats[b, :Fs[b]]).to(r.dtype)).numpy() for b in range(len(Fs))] for r in (r64, r32)]
    assert [len(x) for x in ref[0]] == T
    assert _gate("stem_edges_rms", _cat(emb[b, :T[b]] for b in range(len(Fs))), _cat(ref[0]), _cat(ref[1]))
    assert all(not emb[b, T[b]:].any() for b in range(len(Fs)))
    alone = [dev.pre_encode(feats[b:b + 1, :Fs[b]])[0] for b in range(len(Fs))]
    assert all(np.array_equal(_bits(alone[b]), _bits(emb[b, :T[b]])) for b in range(len(Fs)))


@pytest.mark.parametrize("name", ["A", "B"])
def test_padding_is_inert_and_the_entry_points_agree(name):
    cfg, dev, *_ = _model(name)
    short, long_ = R.test_wave(60, 23000), R.test_wave(61, 70011)
    alone = dev.forward([short])
    T = alone.shape[1]
    batch = dev.forward([long_, short, long_[:31000]])
    junk = dev.forward([long_, short], junk=7.5e3)
    assert np.array_equal(_bits(alone[0]), _bits(batch[1, :T])) and np.array_equal(_bits(alone[0]), _bits(junk[1, :T]))
    assert not batch[1, T:].any()
    # forward_features after features equals forward; pre_encode + encode_embeddings equals forward_features
    rows = [long_, short]
    feats = dev.features(rows)
    F, Td = dev.frames([len(r) for r in rows])
    via = dev(feats, F)
    assert dev.launches == launches(cfg, "forward_features") and np.array_equal(_bits(via), _bits(batch[:2]))
    emb = dev.pre_encode(feats, F)
    two = dev.encode_embeddings(emb, Td)
    assert dev.launches == launches(cfg, "encode_embeddings") and np.array_equal(_bits(two), _bits(via))
    noisy = emb.copy()
    noisy[1, Td[1]:] = 3.0e4
    assert np.array_equal(_bits(dev.encode_embeddings(noisy, Td)), _bits(two))


def test_decisions():
    cfg, dev, r32, r64, _ = _model("A")
    rows = [R.decision_row(s) for s in R.DECISION_SEEDS]
    probs = dev.forward(rows)
    _, T = dev.frames([len(r) for r in rows])
    mels = cfg.fc_encoder_config.num_mel_bins
    for b, row in enumerate(rows):
        p64, p32 = (r.forward_features(R.features(row, mels, r.dtype)).numpy() for r in (r64, r32))
        got = probs[b, :T[b]]
        for thr in R.DECISION_THRESHOLDS:
            ex = R.exempt_mask(p64, p32, thr)
            assert ex.mean() <= 0.02
            assert np.array_equal((got > np.float32(thr))[~ex], (p64 > thr)[~ex]), (b, thr)
            if not ex.any():
                assert mas.preds_to_segments(got, dev.frame_duration, thr) == mas.preds_to_segments(p64.astype(np.float32), dev.frame_duration, thr)


@pytest.mark.parametrize("aosc", [False, True])
def test_streaming(aosc):
    """generate_stream on the device against R.generate_stream: at every step both references run from the device run's state from
    before the step and on the device's features.  The chunk probabilities and the cache / FIFO probabilities the step writes back are
    held to the stage gate; the lengths behind the step and behind the compression and frames_processed to equality."""
    mod = dict(spkcache_len=16, spkcache_sil_frames_per_spk=1, use_aosc=aosc, chunk_left_context=1, chunk_right_context=1, spkcache_update_period=16)
    cfg, dev, r32, r64, _ = _model("A", **mod)
    m = cfg.modules_config
    wave = R.test_wave(70, 96000)
    outs = list(dev.generate_stream(wave, chunk_duration=0.64, spkcache_max=16, fifo_max=16))
    befores = [dev.init_streaming_state()] + [mas.maybe_compress_state(o.state, 16, 16, m) for o in outs[:-1]]
    trimmed, _ = (wave, 0) if aosc else R.literal_trim_silence(wave)
    feats = dev.features([trimmed], peak_normalize=not aosc, normalize=not aosc, pad_to=0 if aosc else 16)[0]
    steps = [list(R.generate_stream(r, wave, 0.64, 16, 16, states=iter(befores), feats=feats)) for r in (r64, r32)]
    assert len(outs) == len(steps[0]) == len(steps[1]) >= 9
    ok, fired = [], 0
    for i, out in enumerate(outs):
        (_, _, _, before, p64, new64, _), (_, _, _, _, p32, new32, _) = steps[0][i], steps[1][i]
        got = out.state
        ok.append(_gate(f"stream{int(aosc)}_step{i}_rms", out.speaker_probs, p64, p32))
        assert (got.spkcache_len, got.fifo_len, got.frames_processed) == (new64.spkcache.shape[1], new64.fifo.shape[1], new64.frames_processed)
        assert got.spkcache_preds.shape == new64.spkcache_preds.shape and got.fifo_preds.shape == new64.fifo_preds.shape
        nf = before.fifo.shape[1]
        if nf + before.spkcache.shape[1] > 0:                              # what the step wrote back over the state's probabilities
            back = lambda s: np.concatenate([np.asarray(s.spkcache_preds), np.asarray(s.fifo_preds)[:, :nf]], axis=1)
            ok.append(_gate(f"stream{int(aosc)}_step{i}_state_preds_rms", back(got), back(new64), back(new32)))
        assert np.array_equal(_bits(got.fifo_preds[0, nf:]), _bits(out.speaker_probs))
        after = mas.maybe_compress_state(got, 16, 16, m)
        assert (after.spkcache_len, after.fifo_len) == R.expected_lengths(got.spkcache_len, got.fifo_len, 16, 16, m)
        assert after.frames_processed == got.frames_processed and after.spkcache_preds.shape[1] == after.spkcache_len
        fired += after.spkcache_len < got.spkcache_len + (got.fifo_len - after.fifo_len)
    assert outs[-1].state.frames_processed == R.diar_frames(feats.shape[0]) and fired >= 3 and all(ok)


def test_published_widths():
    cfg, dev, r32, r64, _ = _model("P")
    row = R.test_wave(80, _n_for_T(100))
    feats = dev.features([row], pad_to=0)
    probs = dev.forward([row], pad_to=0)
    assert probs.shape == (1, 100, 4) and dev.launches == launches(cfg)
    stem = [r.pre_encode(torch.as_tensor(feats[0]).to(r.dtype)).numpy() for r in (r64, r32)]
    ok, taps = _chain_ok("published_", dev, r32, r64, [100], [1, 2, 3, 4, 5, 6])
    ok.append(_gate("published_stem_rms", taps[0][0], stem[0], stem[1]))
    assert all(ok)


def test_errors_leave_the_handle_usable():
    cfg, dev, *_ = _model("A")
    row = R.test_wave(90, 16000)
    want = dev.forward([row])
    for bad in (lambda: dev.forward([row] * 10), lambda: dev.forward([np.zeros(16000 * 11, np.float32)]), lambda: dev.forward([row], pad_to=5),
                lambda: dev(np.zeros((1, 32, 32), np.float32), [40]), lambda: dev.encode_embeddings(np.zeros((1, 8, 128), np.float32), [0]),
                lambda: dev.tap(99)):
        with pytest.raises(mas.AudioGenerationError):
            bad()
        assert np.array_equal(_bits(dev.forward([row])), _bits(want))
    # a tap needs a call that left embeddings; the timing a timed forward; frames applies the calls' own rules
    dev.features([row])
    with pytest.raises(mas.AudioGenerationError, match="no call to tap"):
        dev.tap(0)
    assert np.array_equal(_bits(dev.forward([row])), _bits(want)) and dev.tap(0).shape == (1, want.shape[1], 128)
    dev.enable_timing()
    dev.forward([row])
    assert len(dev.timing()) == 4
    dev(dev.features([row]))
    with pytest.raises(mas.AudioGenerationError, match="no timed forward"):
        dev.timing()
    for lens, pad in (([16000], 5), ([16000 * 10 + 1], 16), ([-1], 0)):
        with pytest.raises(mas.AudioGenerationError):
            dev.frames(lens, pad)
    launches_before = dev.launches
    with pytest.raises(mas.AudioGenerationError):
        dev.encode_embeddings(np.zeros((1, 8, 128), np.float32), [9])
    assert dev.launches == launches_before                               # a rejected call leaves the last call's state
    with pytest.raises(mas.AudioGenerationError, match="conv_kernel_size"):
        c = R.case_config("A")
        c.fc_encoder_config.conv_kernel_size = 8
        mas.SortformerModel(c)


def test_loader_both_key_layouts(tmp_path):
    from safetensors.numpy import save_file
    cfg, dev, _, _, W = _model("A")
    row = R.test_wave(91, 20000)
    want = dev.forward([row])
    body = {k: v for k, v in asdict(cfg).items() if k not in ("max_batch", "max_seconds")}
    raw = {}
    for k, v in W.items():
        if "subsampling.layers_" in k:
            k = k.replace("layers_", "layers.")
            v = v.transpose(0, 3, 1, 2) if v.ndim == 4 else v
        elif v.ndim == 3:
            v = v.transpose(0, 2, 1)
        raw[k] = np.ascontiguousarray(v)
    raw["fc_encoder.layers.0.conv.norm.num_batches_tracked"] = np.zeros(1, np.float32)
    for name, weights in (("raw", raw), ("converted", W)):
        d = tmp_path / name
        d.mkdir()
        (d / "config.json").write_text(json.dumps(body))
        save_file({k: np.ascontiguousarray(v) for k, v in weights.items()}, str(d / "model.safetensors"))
        m = mas.SortformerModel.from_pretrained(str(d), max_batch=1, max_seconds=4)
        assert np.array_equal(_bits(m.forward([row])), _bits(want))
        m.close()
    save_file({**W, "extra.weight": np.zeros(1, np.float32)}, str(tmp_path / "converted" / "model.safetensors"))
    with pytest.raises(mas.AudioGenerationError, match="unused"):
        mas.SortformerModel.from_model_directory(str(tmp_path / "converted"))
