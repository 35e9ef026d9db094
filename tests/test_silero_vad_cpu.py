"""Silero VAD, CPU side: the reference (tests/silero_vad_ref.py) against independent realisations - torch.nn.Conv1d, torch.nn.LSTM, the
literal reflect index list and the literal predictProba windowing, in float32 and float64 - and the host mirror (configs, sanitize,
loader checks, probsToTimestamps and segment_speech against line-by-line transliterations, the errors that need no device), the
decision rows the GPU test relies on, and the resource bounds of the new kernels from the code object's metadata."""
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
import silero_vad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
DTYPES = [torch.float32, torch.float64]


def _tol(dtype):
    return 1e-12 if dtype == torch.float64 else 2e-5


# ---------------------------------------------------------------------------------------------- the network
def test_geometry_of_the_three_configs():
    assert R.geometry(mas.SileroVADBranchConfig.default_16k()) == (576, 4, 2, 1)
    assert R.geometry(mas.SileroVADBranchConfig.default_8k()) == (288, 4, 2, 1)
    assert R.geometry(mas.SileroVADBranchConfig(**R.SMALL)) == (240, 7, 4, 2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_reflect_pad_is_the_literal_index_list(dtype):
    w = torch.arange(576, dtype=dtype)
    got = R.reflect_pad_right(w[None], 64)[0]
    want = [float(i) for i in range(576)] + [float(576 - 2 - j) for j in range(64)]
    assert got.tolist() == want and got[576] == 574 and got[-1] == 511
    # the edge sample is not repeated: the list is n - 2 - j (torch's "reflect"), not n - 1 - j (a symmetric pad)
    assert torch.equal(torch.nn.functional.pad(w[None, None], (0, 64), mode="reflect")[0, 0], got)
    assert torch.equal(R.reflect_pad_right(w[None], 0)[0], w)
    with pytest.raises(AssertionError):
        R.reflect_pad_right(w[None, :64], 64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["16k", "8k", "S"])
def test_front_end_matches_torch_nn_conv1d(name, dtype):
    cfg = R.case_config(name)
    W = R.make_weights(cfg, 1, decisive=False)
    ref = R.case_ref(name, W, dtype)
    b = ref.b
    x = torch.randn(3, ref.n, generator=torch.Generator().manual_seed(2), dtype=torch.float64).to(dtype)

    def nn_conv(key, cin, cout, k, stride, pad, bias=True):
        m = torch.nn.Conv1d(cin, cout, k, stride=stride, padding=pad, bias=bias).to(dtype)
        m.weight.data = ref.W[key + ".weight"].permute(0, 2, 1).contiguous()      # MLX [out, k, in] -> torch [out, in, k]
        if bias:
            m.bias.data = ref.W[key + ".bias"]
        return m

    with torch.no_grad():
        padded = torch.cat([x, x[:, [ref.n - 2 - j for j in range(b.pad)]]], dim=1)
        y = nn_conv("stft_conv", 1, 2 * b.cutoff, b.filter_length, b.hop_length, 0, False)(padded[:, None])      # [N, 2C, F]
        want = [torch.sqrt(y[:, : b.cutoff] ** 2 + y[:, b.cutoff:] ** 2).permute(0, 2, 1)]
        for i, (cin, cout, st) in enumerate(((b.cutoff, 128, 1), (128, 64, 2), (64, 64, 2), (64, 128, 1)), 1):
            want.append(torch.relu(nn_conv(f"conv{i}", cin, cout, 3, st, 1)(want[-1].permute(0, 2, 1))).permute(0, 2, 1))
    got = x
    frames = [ref.F, ref.F, ref.F2, ref.S, ref.S]
    for s in range(5):
        got = ref.step(s, got)
        assert got.shape == want[s].shape and got.shape[1] == frames[s] and got.dtype == dtype
        assert (got - want[s]).abs().max() <= _tol(dtype) * max(1.0, float(want[s].abs().max())), s


@pytest.mark.parametrize("dtype", DTYPES)
def test_recurrence_matches_torch_nn_lstm(dtype):
    """Gate order i, f, g, o; MLX's single bias is torch's bias_ih with bias_hh = 0."""
    cfg = R.case_config("S")
    W = R.make_weights(cfg, 4, decisive=False)
    ref = R.case_ref("S", W, dtype)
    g = torch.Generator().manual_seed(3)
    a4 = torch.randn(5, ref.S, 128, generator=g, dtype=torch.float64).to(dtype)
    st = torch.randn(2, 128, generator=g, dtype=torch.float64).to(dtype)
    m = torch.nn.LSTM(128, 128, batch_first=True).to(dtype)
    m.weight_ih_l0.data, m.weight_hh_l0.data = ref.W["lstm.Wx"], ref.W["lstm.Wh"]
    m.bias_ih_l0.data, m.bias_hh_l0.data = ref.W["lstm.bias"], torch.zeros(512, dtype=dtype)
    with torch.no_grad():
        hseq, (hn, cn) = m(a4.reshape(1, 5 * ref.S, 128), (st[0][None, None], st[1][None, None]))
        want = torch.sigmoid(torch.relu(hseq[0]) @ ref.W["final_conv.weight"].reshape(128) + ref.W["final_conv.bias"][0]).reshape(5, ref.S).mean(1)
    probs, new = ref.recur(ref.step(5, a4), st)
    assert (probs - want).abs().max() <= _tol(dtype) and (new[0] - hn[0, 0]).abs().max() <= _tol(dtype) and (new[1] - cn[0, 0]).abs().max() <= _tol(dtype)
    hid = ref.recur(ref.step(5, a4), st, want_hidden=True)
    assert (hid.reshape(-1, 128) - hseq[0]).abs().max() <= _tol(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_windowing_is_the_literal_predict_proba(dtype):
    cfg = R.case_config("16k")
    ref = R.case_ref("16k", R.make_weights(cfg, 1, decisive=False), dtype)
    x = np.arange(1, 1300, dtype=np.float32)                          # 1299 samples: 3 chunks, 237 zeros of tail
    w = ref.windows(x)
    padded = np.concatenate([np.zeros(64), x, np.zeros(3 * 512 - 1299)])
    assert tuple(w.shape) == (3, 576)
    for j in range(3):
        assert w[j].tolist() == padded[j * 512: j * 512 + 576].tolist()
    assert ref.windows(np.zeros(0, np.float32)).shape[0] == 0 and ref.windows(x[:512]).shape[0] == 1 and ref.windows(x[:513]).shape[0] == 2
    # chunk by chunk with a carried context and state = the whole row
    probs, st = ref.predict(x)
    state, ctx, got = None, torch.zeros(64, dtype=dtype), []
    for j in range(3):
        c = torch.as_tensor(padded[64 + j * 512: 64 + (j + 1) * 512]).to(dtype)
        p, state = ref.recur(ref.gates(torch.cat([ctx, c])[None]), state)
        got.append(p[0]); ctx = c[-64:]
    assert (torch.stack(got) - probs).abs().max() <= _tol(dtype) and (state - st).abs().max() <= _tol(dtype)     # (torch's matmul is not batch-invariant)
    assert ref.predict(np.zeros(0, np.float32))[0].numel() == 0


# ---------------------------------------------------------------------------------------------- config, sanitize, loader
def test_branch_defaults():
    c = mas.SileroVADBranchConfig.default_16k()
    assert (c.sample_rate, c.filter_length, c.hop_length, c.pad, c.cutoff, c.context_size, c.chunk_size) == (16000, 256, 128, 64, 129, 64, 512)
    c = mas.SileroVADBranchConfig.default_8k()
    assert (c.sample_rate, c.filter_length, c.hop_length, c.pad, c.cutoff, c.context_size, c.chunk_size) == (8000, 128, 64, 32, 65, 32, 256)


def test_config_decoding():
    c = mas.SileroVADConfig.from_dict({})
    assert (c.model_type, c.threshold, c.branch16k.chunk_size, c.branch8k.chunk_size) == ("silero_vad", 0.5, 512, 256)
    assert (c.architecture, c.dtype, c.min_speech_duration_ms, c.min_silence_duration_ms, c.speech_pad_ms) == ("silero_vad", "float32", 250, 100, 30)
    up = {"model_type": "silero_vad", "architecture": "silero_vad", "dtype": "float32", "threshold": 0.5, "min_speech_duration_ms": 250,
          "min_silence_duration_ms": 100, "speech_pad_ms": 30,
          "branch_16k": {"sample_rate": 16000, "filter_length": 256, "hop_length": 128, "pad": 64, "cutoff": 129, "context_size": 64,
                         "chunk_size": 512}}
    c = mas.SileroVADConfig.from_dict(json.loads(json.dumps(up)), max_batch=2)
    assert (c.min_speech_duration_ms, c.branch16k.cutoff, c.branch8k.chunk_size, c.max_batch, c.max_chunks) == (250, 129, 256, 2, 1024)
    with pytest.raises(mas.AudioGenerationError):
        mas.SileroVADConfig.from_dict({"branch_8k": {"sample_rate": 8000}})
    cc = mas.SileroVADConfig(max_batch=3, max_chunks=7).to_c()
    assert (cc.branch16k.cutoff, cc.branch8k.chunk_size, cc.branch8k.sample_rate, cc.max_batch, cc.max_chunks) == (129, 256, 8000, 3, 7)


def test_sanitize_and_weight_checks():
    w = {"vad_16k.lstm.Wx": 1, "vad_8k.conv1.bias": 2, "val_loss": 3, "val_acc": 4}
    cleaned = mas.silero_vad_sanitize(w)
    assert set(cleaned) == {"branch16k.lstm.Wx", "branch8k.conv1.bias"} and mas.SileroVAD.sanitize(w) == cleaned
    cfg = R.case_config("S")
    W = R.make_weights(cfg, 1, decisive=False)
    want = mas.silero_vad_expected_shapes(cfg)
    assert len(want) == 28 and want["branch16k.stft_conv.weight"] == (66, 64, 1) and want["branch8k.conv1.weight"] == (128, 3, 65)
    assert want["branch16k.lstm.Wh"] == (512, 128) and want["branch8k.final_conv.weight"] == (1, 1, 128)
    mas.silero_vad_check_weights(cfg, W)
    for broken, word in (({k: v for k, v in W.items() if k != "branch8k.lstm.bias"}, "missing keys ['branch8k.lstm.bias']"),
                         ({**W, "branch16k.conv5.weight": W["branch16k.conv4.weight"]}, "unexpected keys"),
                         ({**W, "branch16k.lstm.Wx": W["branch16k.lstm.Wx"].t().contiguous()}, "branch16k.lstm.Wx has shape")):
        with pytest.raises(mas.AudioGenerationError) as e:
            mas.silero_vad_check_weights(cfg, broken)
        assert word in str(e.value)


def test_read_directory(tmp_path):
    from safetensors.torch import save_file
    cfg = R.case_config("S")
    W = R.make_weights(cfg, 1, decisive=False)
    raw = {k.replace("branch16k.", "vad_16k.").replace("branch8k.", "vad_8k."): v.contiguous() for k, v in W.items()}
    names = sorted(raw)
    save_file({k: raw[k] for k in names[:10]}, str(tmp_path / "a.safetensors"))
    save_file({**{k: raw[k] for k in names[10:]}, "val_loss": torch.zeros(1)}, str(tmp_path / "b.safetensors"))
    with pytest.raises(mas.AudioGenerationError):
        mas.silero_vad_read_directory(str(tmp_path))                  # no config.json
    (tmp_path / "config.json").write_text(json.dumps({"branch_16k": R.SMALL, "threshold": 0.4}))
    c2, W2 = mas.silero_vad_read_directory(str(tmp_path), max_chunks=5)
    assert c2.branch16k == cfg.branch16k and c2.threshold == 0.4 and c2.max_chunks == 5 and set(W2) == set(W)
    assert all(torch.equal(W2[k], W[k]) for k in W)
    with pytest.raises(mas.SileroVADError) as e:
        mas.SileroVAD.from_pretrained(str(tmp_path / "nowhere"))
    assert e.value.kind == "invalidRepositoryID"


def test_errors_that_need_no_device():
    cfg = mas.SileroVADConfig()
    assert cfg.branch(16000) is cfg.branch16k and cfg.branch(8000) is cfg.branch8k
    with pytest.raises(mas.SileroVADError) as e:
        cfg.branch(22050)
    assert e.value.kind == "unsupportedSampleRate" and "Silero VAD supports 8000 Hz and 16000 Hz audio (got 22050)" in str(e.value)
    assert isinstance(e.value, mas.AudioGenerationError) and e.value.case == "invalidInput"
    msgs = {"stateSampleRateMismatch": (mas.SileroVADError.state_sample_rate_mismatch(16000, 8000), "Streaming state is for 16000 Hz, got 8000 Hz"),
            "unexpectedChunkSize": (mas.SileroVADError.unexpected_chunk_size(512, 256), "Expected 512 samples per chunk, got 256"),
            "insufficientReflectPadInput": (mas.SileroVADError.insufficient_reflect_pad_input(64, 64), "Reflect padding of 64 requires more than 64 samples (got 64)"),
            "invalidRepositoryID": (mas.SileroVADError.invalid_repository_id("x"), "Invalid repository ID: x")}
    for kind, (err, text) in msgs.items():
        assert err.kind == kind and text in str(err)


# ---------------------------------------------------------------------------------------------- probsToTimestamps
def _ts(probs, n=100 * 512, rate=16000, thr=0.5, sp=250, si=100, pad=30):
    got = mas.silero_vad_probs_to_timestamps(probs, n, rate, thr, sp, si, pad)
    assert got == R.swift_probs_to_timestamps(probs, n, rate, thr, sp, si, pad) == mas.SileroVAD.probs_to_timestamps(probs, n, rate, thr, sp, si, pad)
    return got


def test_probs_to_timestamps_all_speech():
    assert _ts(np.full(100, 0.9, np.float32)) == [(0, 100 * 512)]


def test_probs_to_timestamps_all_silence():
    assert _ts(np.full(100, 0.01, np.float32)) == []


def test_probs_to_timestamps_two_segments():
    v = np.full(100, 0.01, np.float32)
    v[5:30] = 0.9
    v[50:80] = 0.9
    ts = _ts(v)
    assert len(ts) == 2 and ts == [(5 * 512 - 480, 30 * 512 + 480), (50 * 512 - 480, 80 * 512 + 480)]
    assert _ts(v[None]) == ts                                         # a 2-D input gives its first row


def test_probs_to_timestamps_random():
    rng = np.random.default_rng(11)
    seen = set()
    for trial in range(40):
        n = int(rng.integers(1, 400))
        runs = np.repeat(rng.random(n // 6 + 1), 6)[:n]
        p = np.clip(runs + 0.15 * rng.standard_normal(n), 0, 1).astype(np.float32)
        rate = 16000 if trial % 2 == 0 else 8000
        chunk = 512 if rate == 16000 else 256
        audio_len = n * chunk - int(rng.integers(0, chunk))
        got = _ts(p, audio_len, rate, float(rng.choice([0.5, 0.3, 0.1, 0.9])), int(rng.choice([0, 100, 250])), int(rng.choice([0, 32, 100, 300])),
                  int(rng.choice([0, 30, 200])))
        assert all(0 <= a < b <= audio_len for a, b in got) and all(got[i][1] < got[i + 1][0] for i in range(len(got) - 1))
        seen.add(min(len(got), 3))
    assert seen >= {0, 1, 3}


# ---------------------------------------------------------------------------------------------- segment_speech
def _segments(audio, probs, rate, cfg=None):
    cfg = cfg if cfg is not None else mas.SpeechSegmentConfig()
    got = mas.segment_speech(audio, rate, R.FakeVad(probs), cfg)
    want = R.swift_segment_speech(np.asarray(audio).reshape(len(audio), -1).mean(-1), probs, rate, cfg)
    assert len(got) == len(want)
    mono = np.asarray(audio, np.float32)
    mono = mono.mean(-1) if mono.ndim > 1 else mono
    for (seg, off), (s, e, o) in zip(got, want):
        assert off == o and np.array_equal(seg, mono[s:e])
    return [(s, e) for s, e, _ in want]


def test_segment_speech_against_the_transliteration():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(100 * 512).astype(np.float32)
    d = mas.SpeechSegmentConfig()
    assert (d.threshold, d.min_speech_ms, d.min_silence_ms, d.speech_pad_ms, d.merge_gap_s, d.max_chunk_s) == (0.5, 250, 100, 30, 1.0, 30.0)
    assert _segments(x, np.full(100, 0.01, np.float32), 16000) == [(0, len(x))]            # no speech: the whole buffer
    assert _segments(x, np.full(7, 0.99, np.float32), 16000) == [(0, len(x))]              # fewer than 8 chunks: no block
    assert _segments(x, np.full(100, 0.9, np.float32), 16000) == [(0, 96 * 512)]           # 12 whole blocks
    v = np.full(100, 0.01, np.float32)
    v[8:24] = 0.9
    v[64:88] = 0.9
    assert _segments(x, v, 16000, mas.SpeechSegmentConfig(merge_gap_s=0.5)) == [(8 * 512, 24 * 512), (64 * 512, 88 * 512)]
    assert _segments(x, v, 16000) == [(4096, 12288), (32768, 45056)]                        # a gap of 1.28 s is above merge_gap_s
    assert _segments(x, v, 16000, mas.SpeechSegmentConfig(merge_gap_s=1.5)) == [(4096, 45056)]
    # eight weak chunks make a strong block: 1 - 0.9^8 = 0.57
    assert _segments(x, np.full(100, 0.1, np.float32), 16000) == [(0, 96 * 512)]
    # minimum durations round up: 300 ms of speech needs 2 blocks
    one = np.full(100, 0.0, np.float32)
    one[16:24] = 0.9
    assert _segments(x, one, 16000, mas.SpeechSegmentConfig(min_speech_ms=300)) == [(0, len(x))]
    assert _segments(x, one, 16000) == [(16 * 512, 24 * 512)]
    assert _segments(np.stack([x, 0.5 * x], -1), one, 16000) == [(8192, 12288)]              # channels are averaged
    assert _segments(x, v, 16000, mas.SpeechSegmentConfig(max_chunk_s=0.3)) == [(4096, 8896), (8896, 12288), (32768, 37568), (37568, 42368),
                                                                                 (42368, 45056)]
    for trial in range(30):
        n = int(rng.integers(1, 300))
        p = np.clip(np.repeat(rng.random(n // 10 + 1), 10)[:n] * 0.6 - 0.1 + 0.05 * rng.standard_normal(n), 0, 1).astype(np.float32)
        rate = 16000 if trial % 2 == 0 else 8000
        audio = rng.standard_normal(n * (512 if rate == 16000 else 256) - int(rng.integers(0, 200))).astype(np.float32)
        cfg = mas.SpeechSegmentConfig(threshold=float(rng.choice([0.5, 0.8])), min_speech_ms=int(rng.choice([250, 600])),
                                      min_silence_ms=int(rng.choice([100, 500])), speech_pad_ms=int(rng.choice([30, 300])),
                                      merge_gap_s=float(rng.choice([1.0, 0.2])), max_chunk_s=float(rng.choice([30.0, 1.5])))
        _segments(audio, p, rate, cfg)
    assert mas.speech_runs_from_probs(v, len(x), 16000) == [(8 * 512, 24 * 512), (64 * 512, 88 * 512)]
    assert mas.merge_runs([(0, 10), (20, 30)], 10, 1.0, 30.0) == [(0, 30)]


# ---------------------------------------------------------------------------------------------- decision rows
def test_decision_rows():
    """What test_gpu_silero_vad.py::test_decisions relies on: with the committed seed the float64 reference alone leaves at most 2 % of
    the decision rows' chunks within the exemption margin of either threshold, and the probabilities cross both thresholds many times."""
    cfg = R.case_config("16k")
    W = R.make_weights(cfg, R.DECISION_SEED)
    r32, r64 = R.case_ref("16k", W, torch.float32), R.case_ref("16k", W, torch.float64)
    rows = R.decision_rows()
    assert len(rows) == 8 and all(2 * 16000 <= len(r) <= 4 * 16000 for r in rows)
    cross = {0.5: 0, 0.35: 0}
    exempt = chunks = 0
    stamps = []
    for x in rows:
        p64, p32 = r64.predict(x)[0].numpy(), r32.predict(x)[0].numpy()
        e = R.exempt_chunks(p64, p32)
        exempt += int(e.sum()); chunks += len(e)
        for t in cross:
            a = p64 > t
            cross[t] += int((a[:-1] != a[1:]).sum())
        stamps.append(mas.silero_vad_probs_to_timestamps(p32, len(x), 16000, 0.5, 250, 100, 30))
    print(f"decision rows: crossings {cross}, {exempt}/{chunks} exempt, timestamps {stamps}")
    assert exempt <= 0.02 * chunks and cross[0.5] >= 16 and cross[0.35] >= 16
    assert stamps[1] == [] and any(len(s) >= 2 for s in stamps) and any(s and s[-1][1] == len(x) for s, x in zip(stamps, rows))


# ---------------------------------------------------------------------------------------------- resources
@pytest.fixture(scope="module")
def usage():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S",
                            os.path.join(ROOT, "mlx-audio-swift_amd", "csrc", "silero_vad.hip"), "-o", os.path.join(td, "k.s"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    use, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = use.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for key, pat in (("vgprs", r"remark:\s+VGPRs: (\d+)"), ("agprs", r"remark:\s+AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m:
                cur[key] = int(m.group(1))
    return use


def test_silero_vad_kernels_do_not_spill(usage):
    """No kernel of silero_vad.hip uses scratch and every one fits 64 KiB of LDS.  The recurrence keeps a row of Wh (128 floats) in
    each of its 512 threads: two waves a SIMD, so VGPRs + AGPRs stay within 256 and above the 128 weights."""
    mine = {k: v for k, v in usage.items() if "k_sv_" in k}
    assert len([k for k in mine if "k_sv_gemm" in k]) == 2 and len([k for k in mine if "k_sv_lstm" in k]) == 1
    for k, v in mine.items():
        assert v["scratch"] == 0 and v["lds"] <= 65536 and v["vgprs"] + v["agprs"] <= 256, (k, v)
    lstm = next(v for k, v in mine.items() if "k_sv_lstm" in k)
    assert 128 < lstm["vgprs"] + lstm["agprs"] <= 256, lstm
