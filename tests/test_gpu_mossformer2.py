"""-m gpu: MossFormer2-SE speech enhancement (csrc/mossformer2.hip) through the C ABI against tests/mossformer2_ref.py, which
test_mossformer2_cpu.py holds to numpy / scipy and torch.nn.

Gate of the comparisons (the f32 family's, as test_gpu_fsmn_vad.py): relative rms distance of the device to the float64 reference
<= FLOOR_FACTOR x the float32 reference's own distance to the float64 reference, + SLACK.  Every stage is compared with the reference
run on the device's own previous stage(s).  MIS_MOSSFORMER2_PARITY_LOG=<file> keeps every observed value
(profiles/mossformer2/parity_observed.jsonl)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
import mossformer2_ref as R
from gpu_util import observe, record, rms

pytestmark = pytest.mark.gpu

FLOOR_FACTOR = 2.0
SLACK = 1e-5


def launches(num_blocks, call="enhance"):
    """18 launches a block; 11 around them for enhance, 8 for mask, 6 for mask_features."""
    return {"enhance": 11, "mask": 8, "mask_features": 6}[call] + 18 * num_blocks


def _log(row):
    path = os.environ.get("MIS_MOSSFORMER2_PARITY_LOG")
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
def _rows(name):
    return tuple(R.case_rows(R.case_config(name)))


@functools.lru_cache(maxsize=None)
def _weights(name, nb=2):
    return R.make_weights(R.case_config(name, nb))


_OPEN = []


@functools.lru_cache(maxsize=None)
def _model(name, nb=2):
    cfg = R.case_config(name, nb)
    _OPEN.append(mas.MossFormer2SE.from_weights(cfg, _weights(name, nb)))
    return cfg, _OPEN[-1]


@pytest.fixture(scope="module", autouse=True)
def _release_handles():
    """The shared handles, their streams and workspaces go when the module is done: the tests that follow in a whole-suite run (the
    diagnostics that hold compute units from a second stream among them) find the device as they would without this file."""
    yield
    while _OPEN:
        _OPEN.pop().close()
    for cached in (_model, _refs, _weights, _rows):
        cached.cache_clear()


@functools.lru_cache(maxsize=None)
def _refs(name, nb=2):
    cfg = R.case_config(name, nb)
    return R.MossFormer2Ref(cfg, _weights(name, nb), torch.float32), R.MossFormer2Ref(cfg, _weights(name, nb), torch.float64)


def _cat(parts):
    return np.concatenate([np.asarray(p, np.float64).ravel() for p in parts])


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", ["S", "P"])
def test_taps_of_a_ragged_batch(name):
    cfg, dev = _model(name)
    rows = _rows(name)
    r32, r64 = _refs(name)
    T = [R.frames_of(cfg, len(r)) for r in rows]
    assert T == list(R.ROW_FRAMES)
    mask, Tdev = dev.mask_raw(rows)
    assert Tdev.tolist() == T and dev.launches == launches(2, "mask") and mask.shape == (8, 600, cfg.out_channels_final)
    base = r64.base
    stages = list(range(base + 4)) + list(range(base + 7, base + 7 + R.INNER_STAGES))
    taps = {s: dev.tap(s) for s in stages}
    assert np.array_equal(_bits(taps[base + 3]), _bits(mask)) and taps[0].shape == (8, 600, cfg.num_mels)
    live = [b for b in range(8) if T[b] > 0]
    # the front end against the float64 reference on the waveform
    ok = [_gate("fbank_rms", _cat(taps[0][b, :T[b]] for b in live), _cat(r64.fbank(rows[b]) for b in live), _cat(r32.fbank(rows[b]) for b in live)),
          _gate("features_rms", _cat(taps[1][b, :T[b]] for b in live), _cat(r64.features(rows[b]) for b in live),
                _cat(r32.features(rows[b]) for b in live))]
    assert all(ok), ok
    # the silent row: log(1e-10) | 0 | 0 exactly, and a mask like any other row's
    nm = cfg.num_mels
    assert np.all(taps[1][7, :T[7], :nm] == np.float32(np.log(np.float64(np.float32(1e-10))))) and not _bits(taps[1][7, :, nm:]).any()
    feats, Tf = dev.features_raw(rows)
    assert np.array_equal(_bits(feats), _bits(taps[1])) and Tf.tolist() == T and dev.launches == 2
    # every network stage on the device's own previous stage(s)
    ok = {}
    for s in stages[2:]:
        w32 = _cat(r32.step(s, lambda k, b=b: torch.from_numpy(taps[k][b, :T[b]])) for b in live)
        w64 = _cat(r64.step(s, lambda k, b=b: torch.from_numpy(taps[k][b, :T[b]]).double()) for b in live)
        ok[s] = _gate(f"stage{s if s < base else 'B+' + str(s - base)}", _cat(taps[s][b, :T[b]] for b in live), w64, w32)
    assert all(ok.values()), ok
    # exact zeros behind every row's own frames, in every stage
    for s in stages:
        for b in range(8):
            assert not _bits(taps[s][b, T[b]:]).any(), (s, b)
    assert 0.1 < float((mask[6] == 0).mean()) < 0.9


# ---------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("name", ["S", "P"])
def test_synthesis(name):
    cfg, dev = _model(name)
    rows = _rows(name)
    r32, r64 = _refs(name)
    T = list(R.ROW_FRAMES)
    base, F = r64.base, cfg.out_channels_final
    assert cfg.fft_len == (320 if name == "S" else 1920)
    waves = dev.enhance_batch(rows)
    assert dev.launches == launches(2) and [len(w) for w in waves] == [R.out_len(cfg, t) for t in T]
    mask, spec, fr, wav = dev.tap(base + 3), dev.tap(base + 4), dev.tap(base + 5), dev.tap(base + 6)
    live = [b for b in range(8) if T[b] > 0]
    for b in range(8):
        assert np.array_equal(_bits(wav[b, : len(waves[b])]), _bits(waves[b])) and not _bits(wav[b, len(waves[b]):]).any(), b
    assert not _bits(waves[7]).any() and len(waves[0]) == 0           # the silent row gives exact zeros, the short row nothing
    m = lambda b, dt: torch.from_numpy(mask[b, :T[b]]).to(dt)
    s = lambda b, dt: torch.from_numpy(spec[b, :T[b]]).to(dt)
    f = lambda b, dt: torch.from_numpy(fr[b, :T[b]]).to(dt)
    d32, d64 = torch.float32, torch.float64
    ok = [_gate("stft", _cat(spec[b, :T[b]] for b in live), _cat(r64.stft(rows[b]) for b in live), _cat(r32.stft(rows[b]) for b in live)),
          _gate("istft_frames", _cat(fr[b, :T[b]] for b in live), _cat(r64.istft_frames(s(b, d64), m(b, d64)) for b in live),
                _cat(r32.istft_frames(s(b, d32), m(b, d32)) for b in live)),
          _gate("overlap_add", _cat(waves[b] for b in live), _cat(r64.overlap_add(f(b, d64)) for b in live),
                _cat(r32.overlap_add(f(b, d32)) for b in live)),
          _gate("synthesis", _cat(waves[b] for b in live), _cat(r64.synthesize(rows[b], m(b, d64)) for b in live),
                _cat(r32.synthesize(rows[b], m(b, d32)) for b in live))]
    assert all(ok), ok
    # an all-ones mask reproduces the covered samples of the input
    ones = dev.synthesize_batch(rows, np.ones((8, 600, F), np.float32))
    assert dev.launches == 3
    noisy = [b for b in live if b != 7]
    assert _gate("ones_mask_round_trip", _cat(ones[b] for b in noisy), _cat(rows[b][: len(ones[b])] for b in noisy),
                 _cat(r32.synthesize(rows[b], torch.ones(T[b], F)) for b in noisy))
    assert not _bits(ones[7]).any()


# ---------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("name", ["S", "P"])
def test_chained(name):
    cfg, dev = _model(name)
    rows = [_rows(name)[b] for b in (2, 5)]
    r32, r64 = _refs(name)
    waves = dev.enhance_batch(rows)
    base = r64.base
    feats, mask = dev.tap(1), dev.tap(base + 3)
    T = [R.frames_of(cfg, len(r)) for r in rows]
    w64 = [r64.enhance_from(rows[b], torch.from_numpy(feats[b, :T[b]]).double()) for b in range(2)]
    w32 = [r32.enhance_from(rows[b], torch.from_numpy(feats[b, :T[b]])) for b in range(2)]
    ok = [_gate("chained_mask", _cat(mask[b, :T[b]] for b in range(2)), _cat(w[0] for w in w64), _cat(w[0] for w in w32)),
          _gate("chained_waveform", _cat(waves), _cat(w[1] for w in w64), _cat(w[1] for w in w32))]
    assert all(ok), ok
    one = dev.enhance(rows[0], cfg.sample_rate)
    assert np.array_equal(_bits(one), _bits(waves[0]))
    called = dev(feats[0, :T[0]])                                     # callAsFunction on features
    assert called.shape == (1, T[0], cfg.out_channels_final) and np.array_equal(_bits(called[0]), _bits(mask[0, :T[0]]))
    assert dev.launches == launches(2, "mask_features")


# ---------------------------------------------------------------------------------------------- 4
def test_a_row_does_not_depend_on_its_batch():
    cfg, dev = _model("S")
    rows = _rows("S")
    waves = dev.enhance_batch(rows)
    mask = dev.mask_raw(rows)[0]
    T = list(R.ROW_FRAMES)
    for b in (1, 2, 4, 5, 6):
        assert np.array_equal(_bits(dev.enhance_batch([rows[b]])[0]), _bits(waves[b])), b
        assert np.array_equal(_bits(dev.mask_raw([rows[b]])[0][0]), _bits(mask[b, :T[b]])), b
    for junk in (1e30, float("nan")):
        again = dev.enhance_batch(rows, junk=junk)
        assert all(np.array_equal(_bits(a), _bits(w)) for a, w in zip(again, waves)), junk
        assert np.array_equal(_bits(dev.mask_raw(rows, junk=junk)[0]), _bits(mask)), junk
    feats = dev.features_raw(rows)[0]
    junked = feats.copy()
    for b in range(8):
        junked[b, T[b]:] = np.nan
    assert np.array_equal(_bits(dev(junked, counts=T)), _bits(mask))


# ---------------------------------------------------------------------------------------------- 5
def test_published_depth_once():
    cfg = R.case_config("P", 24, max_batch=1, max_seconds=2.5)
    W = R.make_weights(cfg)
    dev = mas.MossFormer2SE.from_weights(cfg, W)
    row = (0.05 * torch.randn(116736, generator=torch.Generator().manual_seed(9))).numpy()
    wave = dev.enhance(row)
    assert dev.launches == launches(24) == 443 and len(wave) == 299 * 384 + 1920
    r32, r64 = R.MossFormer2Ref(cfg, W, torch.float32), R.MossFormer2Ref(cfg, W, torch.float64)
    feats, mask = dev.tap(1)[0], dev.tap(r64.base + 3)[0]
    assert feats.shape == (300, 180)
    m64, w64 = r64.enhance_from(row, torch.from_numpy(feats).double())
    m32, w32 = r32.enhance_from(row, torch.from_numpy(feats))
    ok = [_gate("depth24_mask", mask, m64.numpy(), m32.numpy()), _gate("depth24_waveform", wave, w64.numpy(), w32.numpy())]
    record("mossformer2_depth24", launches=dev.launches)
    dev.close()
    assert all(ok), ok


# ---------------------------------------------------------------------------------------------- 6
def test_errors_empty_input_and_loader(tmp_path):
    from dataclasses import asdict
    from safetensors.torch import save_file
    cfg, dev = _model("S")
    rows = _rows("S")
    W = _weights("S")
    with pytest.raises(mas.MossFormer2SEError) as e:
        dev.enhance(np.zeros((2, 400), np.float32))
    assert e.value.sts_case == "invalidAudioShape" and "Expected a 1D waveform" in str(e.value)
    with pytest.raises(mas.AudioGenerationError) as e:
        dev.enhance(rows[2], dither=1.0)
    assert "dither" in str(e.value)
    with pytest.raises(mas.AudioGenerationError) as e:
        dev.enhance(rows[2], sample_rate=48000)
    assert "resample" in str(e.value)
    with pytest.raises(mas.AudioGenerationError) as e:
        dev.enhance(np.zeros(cfg.max_samples + 1, np.float32), cfg.sample_rate)
    assert "max_seconds" in str(e.value)
    with pytest.raises(mas.AudioGenerationError) as e:
        dev.enhance_batch([rows[1]] * 9)
    assert "batch" in str(e.value)
    import copy
    bad = copy.deepcopy(cfg)
    bad.fft_len = 322
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.MossFormer2SE(bad)
    assert "out_channels_final" in str(e.value)
    m = mas.MossFormer2SE(cfg)
    with pytest.raises(mas.AudioGenerationError) as e:
        m.enhance(rows[2], cfg.sample_rate)
    assert "finalized" in str(e.value)
    m.close()
    with pytest.raises(mas.AudioGenerationError):
        mas.MossFormer2SE.from_weights(cfg, {k: v for k, v in W.items() if not k.endswith("conv1d_out.bias")})
    # empty input: nothing launched, empty results
    out = dev.enhance_batch([rows[0], np.zeros(0, np.float32)])
    assert [len(o) for o in out] == [0, 0] and dev.launches == 0 and dev.enhance(rows[0], cfg.sample_rate).dtype == np.float32
    assert dev.features_raw([rows[0]])[0].shape == (1, 0, 60)
    # a model directory loads like from_weights: the key forms, the two loaders, the factory
    want = dev.enhance(rows[3], cfg.sample_rate)
    body = {k: v for k, v in asdict(cfg).items() if k not in ("max_batch", "max_seconds", "quantization_config")}
    short = lambda k: k[len("model."):]
    d = tmp_path / "MossFormer2-test"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(body))
    keys = sorted(W)
    half = len(keys) // 2
    save_file({"module." + short(k): W[k].contiguous() for k in keys[:half]}, str(d / "a.safetensors"))
    save_file({short(k): W[k].contiguous() for k in keys[half:]}, str(d / "b.safetensors"))
    for load in (mas.MossFormer2SE.from_model_directory, mas.MossFormer2SE.from_local, mas.load_sts_model):
        mm = load(str(d), max_batch=2, max_seconds=2.5)
        assert mm.config.out_channels == 96 and np.array_equal(_bits(mm.enhance(rows[3], cfg.sample_rate)), _bits(want)), load
        mm.close()
    # the same tensor under a second spelling: fromDirectory overwrites by raw key and then fails on nothing; fromLocal refuses
    save_file({k: W[k].contiguous() for k in keys[:1]}, str(d / "c.safetensors"))
    with pytest.raises(mas.MossFormer2SEError) as e:
        mas.MossFormer2SE.from_local(str(d), max_batch=2, max_seconds=2.5)
    assert e.value.sts_case == "duplicateWeightKey"
    mm = mas.MossFormer2SE.from_model_directory(str(d), max_batch=2, max_seconds=2.5)
    assert np.array_equal(_bits(mm.enhance(rows[3], cfg.sample_rate)), _bits(want))
    mm.close()
    (d / "config.json").write_text(json.dumps(dict(body, quantization_config={"bits": 4, "group_size": 64})))
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.MossFormer2SE.from_model_directory(str(d))
    assert "quantis" in str(e.value)
    empty = tmp_path / "mossformer-empty"
    empty.mkdir()
    with pytest.raises(mas.MossFormer2SEError) as e:
        mas.load_sts_model(str(empty))
    assert e.value.sts_case == "missingSafetensors"
