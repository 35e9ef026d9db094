"""MossFormer2-SE, CPU side: the reference (tests/mossformer2_ref.py) against independent realisations - the front end against numpy /
scipy in float64, the layers against torch.nn, the transform pair against its own round trip - and the host mirror (config, sanitize,
the two loaders' policies, the STS factory's routing, frame arithmetic), the conditions the GPU test relies on for the chosen seed, and
the resource bounds of the new kernels from the code object's metadata."""
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
import mossformer2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
F64 = torch.float64


def _ref(name, nb=2, dtype=F64):
    cfg = R.case_config(name, nb)
    return cfg, R.MossFormer2Ref(cfg, R.make_weights(cfg), dtype)


# ---------------------------------------------------------------------------------------------- front end
@pytest.mark.parametrize("name", ["S", "P"])
def test_front_end_matches_numpy_scipy(name):
    from scipy.signal import get_window
    cfg, ref = _ref(name)
    x = R.case_rows(cfg)[3][: cfg.win_len + 20 * cfg.win_inc + 5]
    got = ref.fbank(x).numpy()
    T = R.frames_of(cfg, len(x))
    assert T == 21 and got.shape == (T, cfg.num_mels)
    a = x.astype(np.float64) * 32768.0
    nfft = R.nfft_of(cfg)
    assert nfft == (512 if name == "S" else 2048)
    win = get_window("hamming", cfg.win_len, fftbins=False)
    # triangles in Hz between HTK-mel-spaced points from 20 Hz to Nyquist, the Nyquist bin included, no normalisation
    h2m = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)
    pts = 700.0 * (10.0 ** (np.linspace(h2m(20.0), h2m(cfg.sample_rate / 2.0), cfg.num_mels + 2) / 2595.0) - 1.0)
    freqs = np.arange(nfft // 2 + 1) * cfg.sample_rate / nfft
    fb = np.zeros((nfft // 2 + 1, cfg.num_mels))
    for j in range(cfg.num_mels):
        fb[:, j] = np.maximum(0.0, np.minimum((freqs - pts[j]) / (pts[j + 1] - pts[j]), (pts[j + 2] - freqs) / (pts[j + 2] - pts[j + 1])))
    assert np.abs(R.mel_filters_f32(cfg) - fb).max() < 2e-4 and fb[-1].max() >= 0.0
    want = np.zeros((T, cfg.num_mels))
    for t in range(T):
        fr = a[t * cfg.win_inc: t * cfg.win_inc + cfg.win_len].copy()
        fr -= fr.mean()
        fr = np.concatenate([[fr[0] - 0.97 * fr[0]], fr[1:] - 0.97 * fr[:-1]]) * win
        want[t] = np.log(np.maximum(np.abs(np.fft.rfft(fr, nfft)) ** 2 @ fb, 1e-10))
    assert np.abs(got - want).max() < 2e-3                           # the float32 filter table against the float64 one
    assert np.abs(R.window_f32(cfg) - win).max() < 1e-6


def test_deltas_match_the_swift_fixture_and_scipy():
    from scipy.ndimage import correlate1d
    d = R.MossFormer2Ref.deltas(torch.tensor([[1.0], [2.0], [3.0], [4.0], [5.0]], dtype=F64))[:, 0]
    assert np.abs(d.numpy() - np.array([0.5, 0.8, 1.0, 0.8, 0.5])).max() < 1e-12          # computeDeltasKaldiNumerical
    f = torch.randn(37, 6, generator=torch.Generator().manual_seed(2), dtype=F64)
    want = correlate1d(f.numpy(), np.arange(-2, 3) / 10.0, axis=0, mode="nearest")
    assert np.abs(R.MossFormer2Ref.deltas(f).numpy() - want).max() < 1e-12
    cfg, ref = _ref("S")
    feats = ref.features(R.case_rows(cfg)[2])
    assert feats.shape == (2, 60)
    one = ref.features(R.case_rows(cfg)[1])
    assert one.shape == (1, 60) and not one[:, 20:].any()             # one frame: edge padding makes both deltas zero
    silent = ref.features(R.case_rows(cfg)[7])
    assert torch.all(silent[:, :20] == float(np.log(np.float64(np.float32(1e-10))))) and not silent[:, 20:].any()


# ---------------------------------------------------------------------------------------------- layers
def test_layers_match_torch_nn():
    cfg, ref = _ref("S")
    g = torch.Generator().manual_seed(3)
    D, T = cfg.out_channels, 300
    x = torch.randn(T, D, generator=g, dtype=F64)
    L, Fs = ref.L(0), ref.Fs(0)
    # FFConvM with ScaleNorm: x g / max(|x| D^-1/2, 1e-8), Linear, SiLU, y + depthwise17(y)
    lin = torch.nn.Linear(D, 4 * D).double()
    lin.weight.data, lin.bias.data = ref.W[L + ".to_hidden.linear.weight"], ref.W[L + ".to_hidden.linear.bias"]
    conv = torch.nn.Conv1d(4 * D, 4 * D, 17, padding=8, groups=4 * D, bias=False).double()
    conv.weight.data = ref.W[L + ".to_hidden.conv_module.weight"].permute(0, 2, 1)
    with torch.no_grad():
        s = torch.cat([torch.cat([torch.zeros(1, D // 2, dtype=F64), x[:-1, : D // 2]]), x[:, D // 2:]], 1)
        n = s * ref.W[L + ".to_hidden.norm.g"] / torch.clamp(torch.linalg.vector_norm(s, dim=-1, keepdim=True) * D ** -0.5, min=1e-8)
        y = torch.nn.functional.silu(lin(n))
        want = y + conv(y.t()[None])[0].t()
    hq = ref.hq(0, x)
    assert (ref.vu(0, hq) - want).abs().max() < 1e-11
    assert torch.equal(ref.shift(x[:1]), x[:1])                       # no shift when T == 1
    # RoPE: traditional pairs, the first 32 dims, untouched beyond
    q4 = ref.qk4(0, hq).reshape(T, 4, R.QK)
    qk = ref.dwres(L + ".to_qk.conv_module.weight", hq[:, 4 * D:])
    heads = qk[:, None, :] * ref.W[L + ".qk_offset_scale.gamma"] + ref.W[L + ".qk_offset_scale.beta"]
    assert torch.equal(q4[:, :, 32:], heads[:, :, 32:]) and torch.equal(q4[0], heads[0])
    t, i = 17, 5
    th = float(np.float32(t) * R.rope_inv_freq()[i])
    a, b = heads[t, 2, 2 * i], heads[t, 2, 2 * i + 1]
    assert abs(q4[t, 2, 2 * i] - (a * np.cos(th) - b * np.sin(th))) < 1e-12 and abs(q4[t, 2, 2 * i + 1] - (a * np.sin(th) + b * np.cos(th))) < 1e-12
    # attention: a literal double loop over groups and keys
    vu = ref.vu(0, hq)
    att = ref.attention(q4.reshape(T, -1), vu)
    D2 = 2 * D
    tq = 270                                                          # second group: keys 256..299
    sim = torch.relu(q4[tq, 0] @ q4[256:300, 2].t() / 256.0) ** 2
    full = sim @ vu[256:300] + q4[tq, 1] @ (q4[:, 3].t() @ vu / T)
    want_t = (full[D2:] * vu[tq, :D2]) * torch.sigmoid(full[:D2] * vu[tq, D2:])
    assert (att[tq] - want_t).abs().max() < 1e-12
    # GatedFSMNBlock
    xa = ref.flash(0, x)
    with torch.no_grad():
        c1 = torch.nn.PReLU(init=float(ref.W[Fs + ".prelu.weight"])).double()(xa @ ref.W[Fs + ".conv1.weight"][:, 0].t() + ref.W[Fs + ".conv1.bias"])
        ln = lambda p, z, eps: torch.nn.functional.layer_norm(z, (256,), ref.W[p + ".weight"], ref.W[p + ".bias"], eps)
        n1 = ln(Fs + ".norm1", c1, 1e-8)
        outs = []
        for h in ("to_u", "to_v"):
            p = Fs + ".gated_fsmn." + h
            y = torch.nn.functional.silu(ln(p + ".norm", n1, 1e-5) @ ref.W[p + ".linear.weight"].t() + ref.W[p + ".linear.bias"])
            cv = torch.nn.Conv1d(256, 256, 17, padding=8, groups=256, bias=False).double()
            cv.weight.data = ref.W[p + ".conv_module.weight"].permute(0, 2, 1)
            outs.append(y + cv(y.t()[None])[0].t())
        xu, xv = outs
        p = Fs + ".gated_fsmn.fsmn"
        p1 = torch.relu(xu @ ref.W[p + ".linear.weight"].t() + ref.W[p + ".linear.bias"]) @ ref.W[p + ".project.weight"].t()
        cv = torch.nn.Conv1d(256, 256, 39, padding=19, groups=256, bias=False).double()
        cv.weight.data = ref.W[p + ".conv1.weight"][:, :, 0, 0][:, None, :]
        xu2 = xu + p1 + cv(p1.t()[None])[0].t()
        want = ln(Fs + ".norm2", xv * xu2 + n1, 1e-8) @ ref.W[Fs + ".conv2.weight"][:, 0].t() + ref.W[Fs + ".conv2.bias"] + xa
    assert (ref.fsmn_block(0, xa) - want).abs().max() < 1e-10
    # GlobalLayerNorm over the whole [T, C] and the sinusoidal table
    f = torch.randn(40, cfg.in_channels, generator=g, dtype=F64)
    want = torch.nn.functional.layer_norm(f, f.shape, eps=1e-8) * ref.W["norm.weight"][:, 0] + ref.W["norm.bias"][:, 0]
    assert (ref.gln(f) - want).abs().max() < 1e-12
    pos = ref.positions(5)
    assert pos.shape == (5, D) and abs(float(pos[0, D // 2]) - float(ref.W["pos_enc.scale"])) < 1e-12 and not pos[0, : D // 2].any()
    # every stage of step() composes to the whole network
    feats = ref.features(R.case_rows(cfg)[2])
    taps = {1: feats}
    order = list(range(2, ref.base + 4)) + list(range(ref.base + 7, ref.base + 7 + R.INNER_STAGES))
    for s in order:
        taps[s] = ref.step(s, lambda k: taps[k])
    assert torch.equal(taps[ref.base + 3], ref.mask_from_features(feats))
    assert (taps[ref.base - 1] - ref.fsmn_block(1, ref.flash(1, taps[ref.base - 3]))).abs().max() == 0


@pytest.mark.parametrize("name", ["S", "P"])
def test_stft_istft_round_trip(name):
    cfg, ref = _ref(name)
    assert cfg.fft_len == (320 if name == "S" else 1920)
    x = R.case_rows(cfg)[3][: cfg.win_len + 30 * cfg.win_inc + 11]
    T = R.frames_of(cfg, len(x))
    spec = ref.stft(x)
    assert spec.shape == (T, 2 * cfg.out_channels_final)
    want = np.fft.rfft(x[: cfg.win_len].astype(np.float64) * 32768.0 * R.window_f32(cfg), cfg.fft_len)
    assert np.abs(spec[0, : cfg.out_channels_final].numpy() - want.real).max() < 1e-7 * np.abs(want).max()
    y = ref.synthesize(x, torch.ones(T, cfg.out_channels_final, dtype=F64)).numpy()
    assert len(y) == R.out_len(cfg, T) and np.abs(y - x[: len(y)]).max() < 1e-9
    half = ref.synthesize(x, torch.full((T, cfg.out_channels_final), 0.5, dtype=F64)).numpy()
    assert np.abs(half - 0.5 * x[: len(y)]).max() < 1e-9


# ---------------------------------------------------------------------------------------------- host mirror
def test_config_defaults_and_decoding():
    c = mas.MossFormer2SEConfig()
    assert (c.model_type, c.sample_rate, c.win_len, c.win_inc, c.fft_len, c.num_mels, c.win_type) == ("mossformer2_se", 48000, 1920, 384, 1920, 60, "hamming")
    assert abs(c.preemphasis - 0.97) < 1e-6 and (c.in_channels, c.out_channels, c.out_channels_final, c.num_blocks) == (180, 512, 961, 24)
    assert (c.one_time_decode_length, c.decode_window, c.chunk_seconds, c.chunk_overlap, c.auto_chunk_threshold, c.quantization_config) == (20, 4, 4.0, 0.25, 60.0, None)
    d = mas.MossFormer2SEConfig.from_dict({"model_type": "mossformer2_se", "sample_rate": 16000, "win_len": 512, "win_inc": 160, "fft_len": 512,
                                           "num_mels": 80, "win_type": "hann", "preemphasis": 0.95, "in_channels": 240, "out_channels": 256,
                                           "out_channels_final": 257, "num_blocks": 6})
    assert (d.sample_rate, d.win_len, d.win_inc, d.fft_len, d.num_mels, d.win_type, d.in_channels, d.out_channels, d.out_channels_final,
            d.num_blocks) == (16000, 512, 160, 512, 80, "hann", 240, 256, 257, 6) and abs(d.preemphasis - 0.95) < 1e-6
    assert d.to_c().win_hann == 1 and c.to_c().win_hann == 0 and c.to_c().max_samples == 60 * 48000
    e = mas.MossFormer2SEConfig.from_dict({}, max_batch=2)
    assert e == mas.MossFormer2SEConfig(max_batch=2)
    q = mas.MossFormer2SEConfig.from_dict({"quantization_config": {"bits": 8, "group_size": 128}, "unknown": 1})
    assert q.quantization_config == {"bits": 8, "group_size": 128}
    assert mas.MossFormer2SEConfig.from_dict({"quantization_config": {}}).quantization_config == {"bits": 4, "group_size": 64}
    with pytest.raises(mas.AudioGenerationError) as err:
        q.to_c()
    assert "quantis" in str(err.value)


def test_sanitize_and_expected_shapes():
    w = {"module.mossformer.norm.weight": 1, "mossformer.norm.bias": 2, "model.mossformer.prelu.weight": 3, "other.key": 4}
    assert mas.mossformer2_sanitize(w) == {"model.mossformer.norm.weight": 1, "model.mossformer.norm.bias": 2, "model.mossformer.prelu.weight": 3,
                                           "other.key": 4}
    assert mas.MossFormer2SE.sanitize is mas.mossformer2_sanitize
    cfg = R.case_config("P", 24)
    s = mas.mossformer2_expected_shapes(cfg)
    assert len(s) == 17 + 24 * (14 + 23) and all(k.startswith("model.mossformer.") for k in s)
    p = "model.mossformer.mdl.intra_mdl.mossformerM."
    assert s[p + "layers.23.to_hidden.linear.weight"] == (2048, 512) and s[p + "layers.0.to_out.linear.weight"] == (512, 1024)
    assert s[p + "fsmn.7.gated_fsmn.fsmn.conv1.weight"] == (256, 39, 1, 1) and s[p + "fsmn.7.prelu.weight"] == ()
    assert s["model.mossformer.conv1d_out.weight"] == (1024, 1, 512) and s["model.mossformer.conv1_decoder.weight"] == (961, 1, 512)
    W = R.make_weights(R.case_config("S"))
    mas.mossformer2_check_weights(R.case_config("S"), W)
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.mossformer2_check_weights(R.case_config("S"), {k: v for k, v in W.items() if not k.endswith("pos_enc.scale")})
    assert "pos_enc.scale" in str(e.value)
    bad = dict(W)
    bad["model.mossformer.conv1_decoder.weight"] = bad["model.mossformer.conv1_decoder.weight"][:-1]
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.mossformer2_check_weights(R.case_config("S"), bad)
    assert "conv1_decoder" in str(e.value)
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.mossformer2_check_weights(R.case_config("S"), dict(W, **{"model.mossformer.output.scales": W["model.mossformer.output.bias"]}))
    assert "quantis" in str(e.value)


def test_loader_policies(tmp_path):
    from safetensors.torch import save_file
    from mlx_audio_swift_amd import sts
    d = tmp_path / "m"
    d.mkdir()
    with pytest.raises(mas.MossFormer2SEError) as e:
        sts._read_weights(str(d), False)
    assert e.value.sts_case == "missingSafetensors" and "No .safetensors files found" in str(e.value)
    one, two = torch.ones(2), torch.full((2,), 2.0)
    save_file({"module.mossformer.a": one, "b": one.clone()}, str(d / "a.safetensors"))
    save_file({"mossformer.a": two, "b": two.clone()}, str(d / "b.SAFETENSORS"))
    w = sts._read_weights(str(d), False)                              # overwrite: later files win, key by key
    assert sorted(w) == ["b", "module.mossformer.a", "mossformer.a"] and float(w["b"][0]) == 2.0
    with pytest.raises(mas.MossFormer2SEError) as e:
        sts._read_weights(str(d), True)                               # fail: the normalised key was seen
    assert e.value.sts_case == "duplicateWeightKey" and "Duplicate normalized weight key" in str(e.value)
    (d / "b.SAFETENSORS").unlink()
    save_file({"mossformer.a": two}, str(d / "b.safetensors"))
    with pytest.raises(mas.MossFormer2SEError) as e:
        sts._read_weights(str(d), True)                               # two spellings of one normalised key
    assert "model.mossformer.a" in str(e.value)
    # config: defaults when missing (both); unreadable -> defaults for fromDirectory, an error for fromLocal; a read file must decode
    assert sts._read_config(str(d), "read_error") == mas.MossFormer2SEConfig() == sts._read_config(str(d), "missing")
    (d / "config.json").mkdir()
    assert sts._read_config(str(d), "read_error") == mas.MossFormer2SEConfig()
    with pytest.raises(OSError):
        sts._read_config(str(d), "missing")
    (d / "config.json").rmdir()
    (d / "config.json").write_text(json.dumps({"num_blocks": 3}))
    assert sts._read_config(str(d), "missing", max_batch=2).num_blocks == 3
    (d / "config.json").write_text("{")
    with pytest.raises(ValueError):
        sts._read_config(str(d), "read_error")


def test_sts_factory_routing(tmp_path):
    r = mas.resolve_sts_model_type
    assert r("anything", " MossFormer2 ") == "mossformer2" and r("x/MossFormer2-SE-fp16") == "mossformer2_se"
    assert r("x/lfm-mossformer") == "lfm_audio" and r("x/DeepFilterNet3") == "deepfilternet3" and r("x/sam-audio") == "sam_audio"
    assert r("nothing-known") is None and r("x/mossformer", "  ") == "mossformer2_se"
    d = tmp_path / "dfn-dir"
    d.mkdir()
    assert r(str(d)) == "deepfilternet3"                              # no config.json: inferred from the path
    (d / "config.json").write_text(json.dumps({"architecture": "MossFormer", "model_version": "x"}))
    (d / "model.safetensors").write_bytes(b"")
    assert r(str(d)) == "mossformer" and r(str(d / "model.safetensors")) == "mossformer"
    (d / "config.json").write_text(json.dumps({"model_version": "DeepFilterNet2"}))
    assert r(str(d)) == "deepfilternet2"
    (d / "config.json").write_text(json.dumps({"model_type": "MossFormer2_SE", "architecture": "sam"}))
    assert r(str(d)) == "mossformer2_se"
    for path, kind in (("x/sam-audio", None), ("x/whatever", "dfn"), ("x/unknown", None)):
        with pytest.raises(mas.STSModelError) as e:
            mas.load_sts_model(path, kind)
        assert "Unsupported STS model type" in str(e.value)


def test_frame_and_length_arithmetic():
    for name in ("S", "P"):
        cfg = R.case_config(name)
        rows = R.case_rows(cfg)
        assert [R.frames_of(cfg, len(r)) for r in rows] == list(R.ROW_FRAMES)
        assert len(rows[0]) == cfg.win_len - 1 and not rows[7].any() and max(len(r) for r in rows) <= cfg.max_samples
        assert R.out_len(cfg, 0) == 0 and R.out_len(cfg, 1) == cfg.win_len and R.out_len(cfg, 600) == 599 * cfg.win_inc + cfg.win_len
        assert all(R.out_len(cfg, R.frames_of(cfg, len(r))) <= len(r) for r in rows)


# ---------------------------------------------------------------------------------------------- the chosen seed
@pytest.mark.parametrize("name,nb,row", [("S", 2, 6), ("P", 2, 5), ("P", 24, None)])
def test_seed_conditions(name, nb, row):
    """What the GPU gates rely on, in every layer of the float64 reference: a mask with zeros and positives, quadratic scores on both
    sides of the ReLU, both attention terms within a factor of 100 of each other (a kernel can drop neither unnoticed), bounded
    activations at depth."""
    cfg, ref = _ref(name, nb)
    x = R.case_rows(cfg)[row] if row is not None else (0.05 * torch.randn(116736, generator=torch.Generator().manual_seed(9))).numpy()
    f = ref.features(x)
    assert f.shape[0] == (300 if row is None else R.ROW_FRAMES[row])
    m, big = ref.mask_from_features(f, want_max=True)
    zeros, pos = float((m == 0).double().mean()), float((m > 0).double().mean())
    assert 0.1 <= zeros <= 0.9 and 0.1 <= pos <= 0.9 and big < 1e4
    xi = ref.encode(ref.gln(f))
    for i in range(nb):
        hq = ref.hq(i, xi)
        _, quad, lin, frac = ref.attention(ref.qk4(i, hq), ref.vu(i, hq), parts=True)
        ql, qq = float(lin.pow(2).mean().sqrt()), float(quad.pow(2).mean().sqrt())
        assert 0.1 <= frac <= 0.9 and ql >= 0.01 * qq and qq >= 0.01 * ql, (i, frac, ql, qq)
        xi = ref.fsmn_block(i, ref.flash(i, xi))


# ---------------------------------------------------------------------------------------------- resources
@pytest.fixture(scope="module")
def usage():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S",
                            os.path.join(ROOT, "mlx-audio-swift_amd", "csrc", "mossformer2.hip"), "-o", os.path.join(td, "k.s"),
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


def test_mossformer2_kernels_do_not_spill(usage):
    """No kernel of mossformer2.hip uses scratch, every one fits 64 KiB of LDS and 256 VGPRs (two waves per SIMD at least)."""
    mine = {k: v for k, v in usage.items() if "k_mf2_" in k}
    for name in ("fbank", "deltas", "gln", "row", "gemm", "dwconv", "linkv", "linsum", "attn", "ola"):
        assert any(f"k_mf2_{name}" in k for k in mine), name
    assert len(mine) == 10
    for k, v in mine.items():
        assert v["scratch"] == 0 and v["vgprs"] <= 256 and v["lds"] <= 65536, (k, v)
