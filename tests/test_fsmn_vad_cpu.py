"""FSMN VAD, CPU side: the reference (tests/fsmn_vad_ref.py) against independent realisations - the encoder against torch.nn.Linear and
a left-padded grouped Conv1d, the front end against numpy / scipy in float64 - and the host mirror (configs, sanitize, loader, CMVN
parsing, the post-processing port against the literal transliteration, chunks_from_segments), the decision rows the GPU test relies
on, and the resource bounds of the new kernels from the code object's metadata."""
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
import fsmn_vad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


# ---------------------------------------------------------------------------------------------- encoder
def _nn_encoder(cfg, W, x):
    e = cfg.encoder

    def lin(name, i, o, bias=True):
        m = torch.nn.Linear(i, o, bias=bias).double()
        m.weight.data = W[name + ".weight"].double()
        if bias:
            m.bias.data = W[name + ".bias"].double()
        return m

    with torch.no_grad():
        h = torch.relu(lin("in_linear2", e.input_affine_dim, e.linear_dim)(lin("in_linear1", e.input_dim, e.input_affine_dim)(x)))
        for i in range(e.fsmn_layers):
            p = lin(f"fsmn.{i}.linear", e.linear_dim, e.proj_dim, False)(h)
            conv = torch.nn.Conv1d(e.proj_dim, e.proj_dim, e.lorder, groups=e.proj_dim, bias=False).double()
            conv.weight.data = W[f"fsmn.{i}.fsmn_block.conv_left.weight"].double().permute(0, 2, 1)      # [proj, lorder, 1] -> [proj, 1, lorder]
            m = p + conv(torch.nn.functional.pad(p.t()[None], (e.lorder - 1, 0)))[0].t()
            h = torch.relu(lin(f"fsmn.{i}.affine", e.proj_dim, e.linear_dim)(m))
        z = lin("out_linear2", e.output_affine_dim, e.output_dim)(lin("out_linear1", e.linear_dim, e.output_affine_dim)(h))
        return torch.softmax(z, dim=-1)


@pytest.mark.parametrize("name", ["S", "P"])
def test_encoder_matches_torch_nn(name):
    cfg = R.case_config(name)
    W = R.make_weights(cfg, 3, decisive=False)
    x = torch.randn(57, cfg.encoder.input_dim, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    got = R.FsmnVadRef(cfg, W, None, torch.float64).stages(x)[6 + 2 * cfg.encoder.fsmn_layers]
    want = _nn_encoder(cfg, W, x)
    assert got.shape == want.shape == (57, cfg.encoder.output_dim) and (got - want).abs().max() < 1e-12


def test_reference_smoke_shape():
    enc = mas.FSMNVADEncoderConfig(input_dim=8, input_affine_dim=6, fsmn_layers=2, linear_dim=10, proj_dim=4, lorder=3, output_affine_dim=5,
                                   output_dim=7)
    cfg = mas.FSMNVADConfig(encoder=enc)
    W = R.make_weights(cfg, 1, decisive=False)
    x = ((torch.arange(6 * 8) % 101 - 50) / 50.0).reshape(6, 8)
    out = R.FsmnVadRef(cfg, W, None, torch.float32).stages(x)[6 + 2 * 2][None]
    assert tuple(out.shape) == (1, 6, 7) and (out.sum(-1) - 1.0).abs().max() < 1e-5


# ---------------------------------------------------------------------------------------------- front end
def _front_end_scipy(x):
    sig = pytest.importorskip("scipy.signal")
    x = np.asarray(x, np.float64) * 32768.0
    T = R.frames_of(len(x))
    win = sig.get_window("hamming", 400, fftbins=False)

    def mel(f):
        return 1127.0 * np.log(1.0 + f / 700.0)

    edges = mel(20.0) + np.arange(82) * (mel(8000.0) - mel(20.0)) / 81.0
    m = mel(np.arange(257) * 16000.0 / 512.0)
    fb = np.zeros((257, 80))
    for j in range(80):
        fb[:, j] = np.maximum(0.0, np.minimum((m - edges[j]) / (edges[j + 1] - edges[j]), (edges[j + 2] - m) / (edges[j + 2] - edges[j + 1])))
    fb[256] = 0.0
    out = np.zeros((T, 80))
    for t in range(T):
        fr = x[t * 160: t * 160 + 400]
        fr = fr - fr.mean()
        fr = np.concatenate([fr[:1], fr[1:] - 0.97 * fr[:-1]]) * win
        out[t] = np.log(np.maximum(np.abs(np.fft.rfft(fr, 512)) ** 2 @ fb, 1e-8))
    return out, fb


@pytest.mark.parametrize("n", [400, 559, 560, 16000])
def test_front_end_matches_scipy(n):
    x = (0.1 * np.random.default_rng(n).standard_normal(n)).astype(np.float32)
    want, fb = _front_end_scipy(x)
    got = R.fbank(x, 80, torch.float64).numpy()
    assert got.shape == want.shape == (R.frames_of(n), 80)
    assert np.abs(got - want).max() < 1e-9 * max(1.0, np.abs(want).max())
    assert np.abs(R.mel_filters(80, torch.float64).numpy() - fb).max() < 1e-12
    d = R.decibel(x, torch.float64).numpy()
    assert np.allclose(d, [10 * np.log10(np.sum(x[t * 160: t * 160 + 400].astype(np.float64) ** 2) + 1e-6) for t in range(len(d))], rtol=1e-12)
    f32 = R.fbank(x, 80, torch.float32).numpy()
    assert f32.dtype == np.float32 and np.abs(f32 - want).max() < 1e-2


def test_feature_shapes_and_the_filter_matrix():
    cfg = R.case_config("P")
    ref = R.FsmnVadRef(cfg, R.make_weights(cfg, 1, decisive=False), None, torch.float64)
    x = (0.1 * np.random.default_rng(0).standard_normal(16000)).astype(np.float32)
    assert tuple(ref.features(x).shape) == (100, 400) and tuple(ref.features(x[:399]).shape) == (0, 400)
    one = ref.features(x[:400])
    fb = R.fbank(x[:400], 80, torch.float64)
    assert tuple(one.shape) == (3, 400) and tuple(fb.shape) == (1, 80)
    for r in range(3):
        for i in range(5):
            assert torch.equal(one[r, 80 * i: 80 * i + 80], fb[0])
    for dt in (torch.float32, torch.float64):
        m = R.mel_filters(80, dt)
        assert tuple(m.shape) == (257, 80) and not m[256].any() and (m[:256].sum(0) > 0).all()
        assert ((m > 0).sum(1) <= 2).all()                            # a bin touches at most two filters
    assert R.rows_of(98) == 100 and R.rows_of(0) == 0 and R.rows_of(10, 5, 2) == 6
    f = torch.arange(12.0).reshape(6, 2)
    assert R.lfr(f, 5, 1)[0].tolist() == [0, 1, 0, 1, 0, 1, 2, 3, 4, 5] and R.lfr(f, 5, 1)[7].tolist() == [10, 11] * 5
    assert np.array_equal(R.lfr_cmvn_numpy(f.numpy(), None), R.lfr(f).numpy())


# ---------------------------------------------------------------------------------------------- CMVN
def test_cmvn_parsing(tmp_path):
    text = "<Nnet>\n<Splice> 400 400\n[ 0 ]\n<AddShift> 4 4\n<LearnRateCoef> 0 [ -8.5 -8.25\t1e-1 x 2 ]\n<Rescale> 4 4\n<LearnRateCoef> 0 [ 0.5 0.25\n0.125 1 ]\n</Nnet>"
    shift, scale = mas.parse_kaldi_cmvn(text)
    assert shift.dtype == np.float32 and shift.tolist() == [-8.5, -8.25, np.float32(0.1), 2.0] and scale.tolist() == [0.5, 0.25, 0.125, 1.0]
    assert mas.parse_kaldi_cmvn(text.encode())[1].tolist() == scale.tolist()
    for bad in ("<AddShift> [ 1 ]", "<Rescale> [ 1 ] <AddShift> 1 2", "<AddShift> [ 1 <Rescale> 2"):
        with pytest.raises(mas.AudioGenerationError) as e:
            mas.parse_kaldi_cmvn(bad)
        assert "Could not parse Kaldi CMVN data" in str(e.value)
    assert mas.fsmn_vad_read_cmvn(str(tmp_path)) is None
    (tmp_path / "am.mvn").write_text(text)
    assert mas.fsmn_vad_read_cmvn(str(tmp_path))[0].tolist() == shift.tolist()
    (tmp_path / "cmvn.json").write_text(json.dumps({"shift": [1.0, 2.0], "scale": [3.0, 4.0]}))
    assert mas.fsmn_vad_read_cmvn(str(tmp_path))[1].tolist() == [3.0, 4.0]                 # cmvn.json wins
    # a CMVN of the wrong length is not applied
    cfg = R.case_config("S")
    W = R.make_weights(cfg, 1, decisive=False)
    x = (0.1 * np.random.default_rng(0).standard_normal(4000)).astype(np.float32)
    plain = R.FsmnVadRef(cfg, W, None).features(x)
    assert torch.equal(R.FsmnVadRef(cfg, W, (np.ones(80, np.float32), np.ones(80, np.float32))).features(x), plain)
    assert not torch.equal(R.FsmnVadRef(cfg, W, R.make_cmvn(cfg, 1)).features(x), plain)
    assert np.array_equal(R.lfr_cmvn_numpy(np.ones((3, 80), np.float32), (np.ones(80), np.ones(80))), np.ones((5, 400), np.float32))


# ---------------------------------------------------------------------------------------------- config and loader
def test_config_defaults_and_keys():
    c = mas.FSMNVADConfig()
    e = c.encoder
    assert (e.input_dim, e.input_affine_dim, e.fsmn_layers, e.linear_dim, e.proj_dim, e.lorder, e.rorder, e.lstride, e.rstride,
            e.output_affine_dim, e.output_dim) == (400, 140, 4, 250, 128, 20, 0, 1, 0, 140, 248)
    assert (c.model_type, c.architecture, c.sample_rate, c.n_mels, c.frame_length, c.frame_shift, c.lfr_m, c.lfr_n) == \
        ("fsmn", "fsmn_vad", 16000, 80, 25, 10, 5, 1)
    assert (c.max_end_silence_time, c.max_start_silence_time, c.window_size_ms, c.sil_to_speech_time_thres, c.speech_to_sil_time_thres,
            c.speech_noise_thres, c.sil_pdf_ids, c.frame_in_ms, c.max_batch, c.chunk_frames) == (800, 3000, 200, 150, 150, 0.6, [0], 10, 8, 3000)
    d = mas.FSMNVADConfig.from_dict({"sample_rate": 8000, "sil_pdf_ids": [0, 3], "speech_noise_thres": 0.5, "n_mels": None, "unknown": 1,
                                     "encoder": {"input_dim": 400, "input_affine_dim": 24, "fsmn_layers": 2, "linear_dim": 40, "proj_dim": 16,
                                                 "lorder": 3, "rorder": 0, "lstride": 1, "rstride": 0, "output_affine_dim": 20,
                                                 "output_dim": 7}}, max_batch=2)
    assert (d.sample_rate, d.sil_pdf_ids, d.speech_noise_thres, d.n_mels, d.encoder.lorder, d.max_batch) == (8000, [0, 3], 0.5, 80, 3, 2)
    with pytest.raises(mas.AudioGenerationError):
        mas.FSMNVADConfig.from_dict({"encoder": {"input_dim": 400}})
    cc = d.to_c()
    assert (cc.lorder, cc.n_sil, list(cc.sil_pdf_ids)[:2], cc.max_batch, cc.chunk_frames) == (3, 2, [0, 3], 2, 3000)
    assert mas.FSMNVADConfig(sil_pdf_ids=[0, 999]).to_c().n_sil == 1


def test_sanitize_and_weight_checks(tmp_path):
    from safetensors.torch import save_file
    cfg = R.case_config("S")
    W = R.make_weights(cfg, 1, decisive=False)
    raw = {"encoder." + k: v for k, v in W.items()}
    assert set(mas.fsmn_vad_sanitize(raw)) == set(W) == set(mas.fsmn_vad_expected_shapes(cfg))
    assert mas.fsmn_vad_expected_shapes(cfg)["fsmn.1.fsmn_block.conv_left.weight"] == (16, 3, 1)
    mas.fsmn_vad_check_weights(cfg, W)
    for broken, word in (({k: v for k, v in W.items() if k != "out_linear2.bias"}, "missing keys ['out_linear2.bias']"),
                         ({**W, "fsmn.0.fsmn_block.conv_right.weight": W["fsmn.0.fsmn_block.conv_left.weight"]}, "unexpected keys"),
                         ({**W, "in_linear1.weight": W["in_linear1.weight"].t().contiguous()}, "in_linear1.weight has shape")):
        with pytest.raises(mas.AudioGenerationError) as e:
            mas.fsmn_vad_check_weights(cfg, broken)
        assert word in str(e.value)
    body = {"encoder": {k: getattr(cfg.encoder, k) for k in cfg.encoder.__dataclass_fields__}, "sil_pdf_ids": [0]}
    (tmp_path / "config.json").write_text(json.dumps(body))
    save_file({k: v.contiguous() for k, v in raw.items()}, str(tmp_path / "model.safetensors"))
    (tmp_path / "am.mvn").write_text("<AddShift> [ 1 2 ] <Rescale> [ 3 4 ]")
    c2, W2, cmvn = mas.fsmn_vad_read_directory(str(tmp_path), chunk_frames=64)
    assert c2.encoder == cfg.encoder and c2.chunk_frames == 64 and set(W2) == set(W) and cmvn[1].tolist() == [3.0, 4.0]
    assert all(torch.equal(W2[k], W[k]) for k in W)
    with pytest.raises(mas.AudioGenerationError):
        mas.FSMNVAD.from_pretrained(str(tmp_path / "nowhere"))


# ---------------------------------------------------------------------------------------------- post-processing
def _both(cfg, sil, dec, n):
    got = mas.fsmn_vad_postprocess(sil, dec, n, cfg)
    assert got == R.swift_segments(cfg, sil, dec, n)
    return got


def test_post_processing_facts():
    cfg = mas.FSMNVADConfig()
    assert _both(cfg, np.ones(300, np.float32), np.zeros(300, np.float32), 48000) == []
    # the window reaches 15 at frame 14, the start backs off to frame 0, the final frame closes at (299 + 1) x 10
    assert _both(cfg, np.zeros(300, np.float32), np.zeros(300, np.float32), 48000) == [[0, 3000]]
    segs = mas.fsmn_vad_postprocess(np.zeros(7000, np.float32), np.zeros(7000, np.float32), 7000 * 160 + 240, cfg)
    assert len(segs) >= 2 and segs[0] == [0, 60010] and all(a < b for a, b in segs)
    assert all(segs[i][1] <= segs[i + 1][0] for i in range(len(segs) - 1))
    # decibel below -100 is silence whatever the score; fewer decibel frames than scores: the tail is silence
    assert _both(cfg, np.zeros(300, np.float32), np.full(300, -120.0, np.float32), 48000) == []
    assert _both(cfg, np.zeros(302, np.float32), np.zeros(300, np.float32), 48400) == _both(cfg, np.r_[np.zeros(300), np.ones(2)], np.zeros(302), 48400)
    rng = np.random.default_rng(4)
    for trial in range(6):                                            # random runs of speech and silence, random energies
        n = int(rng.integers(50, 900))
        sil = np.repeat(rng.random(n // 10 + 1) < 0.5, 10)[:n].astype(np.float32) * 0.9 + 0.05
        dec = (rng.standard_normal(n) * 30 - 20).astype(np.float32)
        _both(cfg, sil, dec, n * 160 + 240)
    multi = mas.FSMNVADConfig(sil_pdf_ids=[0, 2], window_size_ms=100, max_end_silence_time=400)
    _both(multi, sil, dec, n * 160 + 240)


def test_the_transliteration_computes_its_own_decibel():
    x = R.decision_rows()[4][:8000]
    post = R.SwiftPostprocess(mas.FSMNVADConfig())
    post.computeDecibel(x)
    assert len(post.decibel) == R.frames_of(len(x)) and np.allclose(post.decibel, R.decibel(x, torch.float64).numpy(), atol=1e-3)


def test_chunks_from_segments():
    f = mas.chunks_from_segments
    assert f([[0, 1000], [1500, 2500]], 10 ** 6, 16000) == [(0, 40000, 0.0)]
    assert f([[0, 1000], [2500, 3000]], 10 ** 6, 16000) == [(0, 16000, 0.0), (40000, 48000, 2.5)]
    assert [(b - a) for a, b, _ in f([[0, 70000]], 70 * 16000, 16000)] == [480000, 480000, 160000]
    assert [o for _, _, o in f([[0, 70000]], 70 * 16000, 16000)] == [0.0, 30.0, 60.0]
    assert f([], 5, 16000) == [(0, 5, 0.0)]
    assert f([[0, 2000]], 20000, 16000) == [(0, 20000, 0.0)]                               # an end beyond n_samples is clamped
    assert f([[5000, 6000]], 20000, 16000) == [(0, 20000, 0.0)]                            # nothing left inside the buffer: the whole of it
    assert f([[0, 1]], 100, 16000, max_chunk_s=0.0) == [(i, i + 1, i / 16000.0) for i in range(16)]
    assert f([[0, 1000], [1500, 2500]], 10 ** 6, 16000, merge_gap_s=0.25) == [(0, 16000, 0.0), (24000, 40000, 1.5)]


# ---------------------------------------------------------------------------------------------- decision rows
def test_decision_rows():
    """What test_gpu_fsmn_vad.py::test_decisions relies on, with the float32-vs-float64 distance as the error."""
    cfg = R.case_config("P")
    W, cmvn = R.make_weights(cfg, R.DECISION_SEED), R.make_cmvn(cfg, R.DECISION_SEED)
    r32, r64 = R.FsmnVadRef(cfg, W, cmvn, torch.float32), R.FsmnVadRef(cfg, W, cmvn, torch.float64)
    k = 7 + 2 * cfg.encoder.fsmn_layers
    rows = R.decision_rows()
    assert len(rows) == 8 and all(2 * 16000 <= len(r) <= 4 * 16000 for r in rows)
    up = down = exempt = frames = clean = 0
    segs = []
    for x in rows:
        s64, s32 = r64.stages(r64.features(x))[k].numpy(), r32.stages(r32.features(x))[k].numpy()
        above = s64 > 0.2
        up += int((~above[:-1] & above[1:]).sum()); down += int((above[:-1] & ~above[1:]).sum())
        e = float(np.abs(s32 - s64).max())
        unsure = np.abs(1.0 - 2.0 * s64 - cfg.speech_noise_thres) < 4 * e + 1e-6
        exempt += int(unsure.sum()); frames += len(unsure); clean += int(not unsure.any())
        d = R.decibel(x).numpy()
        segs.append(_both(cfg, s32, d, len(x)))
        assert np.array_equal(R.speech_flags(s32, d, cfg.speech_noise_thres)[~unsure[: len(d)]], R.speech_flags(s64, d, cfg.speech_noise_thres)[~unsure[: len(d)]])
    print(f"decision rows: {up} up / {down} down crossings, {exempt}/{frames} exempt, {clean} clean rows, segments {segs}")
    assert up > 0 and down > 0 and exempt <= 0.01 * frames and clean >= 4
    assert any(len(s) == 2 for s in segs) and any(s == [] for s in segs)
    assert any(s and s[-1][1] == R.rows_of(R.frames_of(len(x))) * 10 for s, x in zip(segs, rows))   # still open at the last frame


# ---------------------------------------------------------------------------------------------- resources
@pytest.fixture(scope="module")
def usage():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S",
                            os.path.join(ROOT, "mlx-audio-swift_amd", "csrc", "fsmn_vad.hip"), "-o", os.path.join(td, "k.s"),
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
        for key, pat in (("vgprs", r"remark:\s+VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m:
                cur[key] = int(m.group(1))
    return use


def test_fsmn_vad_kernels_do_not_spill(usage):
    """No kernel of fsmn_vad.hip uses scratch and every one fits 64 KiB of LDS.  The 64 x 64 tile (16 accumulators, the lorder - 1 rows
    of halo in LDS) stays within 128 VGPRs, four of its waves per SIMD; the 32 x 256 tile that holds a score row carries 32 accumulators
    and 32 staged weights a lane and stays within 256, two waves per SIMD."""
    mine = {k: v for k, v in usage.items() if "k_fvad_" in k}
    assert len([k for k in mine if "k_fvad_gemm" in k]) == 2 and any("k_fvad_fbank" in k for k in mine) and any("k_fvad_lfr" in k for k in mine)
    for k, v in mine.items():
        assert v["scratch"] == 0 and v["vgprs"] <= (256 if "ILi1ELi2EE" in k else 128) and v["lds"] <= 65536, (k, v)
