"""DeepFilterNet, CPU side: the reference (tests/deepfilternet_ref.py) against independent realisations - torch.nn.Conv2d /
ConvTranspose2d with groups, BatchNorm2d in eval, nn.GRU, einsum - the normalisation's two forms, the host arithmetic (ERB widths,
norm alpha, Vorbis window, frame counts), the host mirror (config, loader rules, refusals, factory routing) and the resource bounds of
the new kernels from the code object's metadata."""
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
import deepfilternet_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
PUBLISHED_WIDTHS = [2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 5, 5, 7, 7, 8, 10, 12, 13, 15, 18, 20, 24, 28, 31, 37, 42, 50, 56, 67]


def close(a, b, tol=1e-10):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max()), np.abs(a - b).max()


# ---------------------------------------------------------------------------------------------- layers against torch
@pytest.mark.parametrize("cin,cout,ipg,kt,kf,fs", [(1, 8, 1, 3, 3, 1), (8, 8, 1, 1, 3, 2), (2, 8, 1, 3, 3, 1), (8, 10, 4, 5, 1, 1), (8, 8, 1, 1, 1, 1),
                                                   (8, 1, 8, 1, 3, 1), (6, 6, 1, 2, 3, 2)])
def test_conv2d_matches_torch(cin, cout, ipg, kt, kf, fs):
    rng = np.random.default_rng(cin * 100 + cout)
    T, F = 7, 9
    x, w = rng.standard_normal((T, F, cin)), rng.standard_normal((cout, ipg, kt, kf))
    conv = torch.nn.Conv2d(cin, cout, (kt, kf), stride=(1, fs), padding=(0, kf // 2), groups=cin // ipg, bias=False).double()
    conv.weight.data = torch.from_numpy(w)
    xt = torch.nn.functional.pad(torch.from_numpy(x).permute(2, 0, 1)[None], (0, 0, kt - 1, 0))       # ConstantPad2d((0, 0, kT - 1, 0))
    want = conv(xt)[0].permute(1, 2, 0).detach().numpy()
    close(R.conv2d(x, w, fs), want)


@pytest.mark.parametrize("C,opg,kf,F", [(8, 1, 3, 5), (4, 2, 3, 4), (8, 1, 1, 6)])
def test_conv_transpose2d_matches_torch(C, opg, kf, F):
    rng = np.random.default_rng(C + kf)
    x, w = rng.standard_normal((6, F, C)), rng.standard_normal((C, opg, 1, kf))
    ct = torch.nn.ConvTranspose2d(C, C * opg, (1, kf), stride=(1, 2), padding=(0, kf // 2), output_padding=(0, kf // 2), groups=C, bias=False).double()
    ct.weight.data = torch.from_numpy(w)
    want = ct(torch.from_numpy(x).permute(2, 0, 1)[None])[0].permute(1, 2, 0).detach().numpy()
    close(R.conv_transpose2d(x, w, 2, C), want)


def test_batch_norm_matches_torch_eval():
    rng = np.random.default_rng(3)
    n = 6
    W = {"p.weight": rng.uniform(0.5, 1.5, n), "p.bias": rng.standard_normal(n), "p.running_mean": rng.standard_normal(n),
         "p.running_var": rng.uniform(0.5, 1.5, n)}
    bn = torch.nn.BatchNorm2d(n).double().eval()
    bn.weight.data, bn.bias.data = torch.from_numpy(W["p.weight"]), torch.from_numpy(W["p.bias"])
    bn.running_mean.data, bn.running_var.data = torch.from_numpy(W["p.running_mean"]), torch.from_numpy(W["p.running_var"])
    x = rng.standard_normal((5, 4, n))
    close(R.batch_norm(x, W, "p"), bn(torch.from_numpy(x).permute(2, 0, 1)[None])[0].permute(1, 2, 0).detach().numpy())


@pytest.mark.parametrize("layers", [1, 2])
def test_gru_matches_torch(layers):
    """Fixes the gate order r | z | n and b_hn inside the r product."""
    rng = np.random.default_rng(layers)
    H, T = 12, 9
    gru = torch.nn.GRU(H, H, layers).double()
    W = {f"g.{k}": v.detach().numpy() for k, v in gru.named_parameters()}
    x = rng.standard_normal((T, H))
    y = x
    for l in range(layers):
        y = R.gru_layer(y, W, "g", l)
    close(y, gru(torch.from_numpy(x)[:, None])[0][:, 0].detach().numpy())


def test_grouped_linear_matches_einsum():
    rng = np.random.default_rng(0)
    x, w = rng.standard_normal((5, 24)), rng.standard_normal((4, 6, 3))
    close(R.grouped_linear(x, w), np.einsum("tgi,gih->tgh", x.reshape(5, 4, 6), w).reshape(5, 12))


# ---------------------------------------------------------------------------------------------- the normalisation
def test_closed_form_is_the_recurrence_in_float64():
    """a^t (init + (1 - a) cumsum(x / a^t)) is the recurrence s_t = a s_(t-1) + (1 - a) x_t started one decay earlier: from init / a.
    Against the recurrence from init itself (libDF, bandMeanNormExact, the engine) it differs by exactly a^t (1 - a) init: 1 % of the
    initial state at frame 0, 4e-7 of it at frame 1 000."""
    rng = np.random.default_rng(1)
    a = np.float64(np.float32(0.99))
    for T in (1, 2, 10, 1000):
        x = -60 + 20 * rng.standard_normal((T, 8))
        init = R.linspace(-60.0, -90.0, 8, np.float64)
        closed = R.ema_closed(x, a, init)
        assert np.abs(closed - R.ema(x, a, init / a)).max() <= 1e-9 * 90
        want = (a ** np.arange(T))[:, None] * (1 - a) * init[None]
        assert np.abs((closed - R.ema(x, a, init)) - want).max() <= 1e-9 * 90
    x = np.abs(rng.standard_normal((500, 4)))
    re, im = R.band_unit_norm(x, 0 * x, a, closed=True)
    assert np.isfinite(re).all() and not im.any()


def test_float32_closed_form_leaves_the_float32_range():
    """0.99^-t overflows float32 where t > log(FLT_MAX) / -log(0.99): the closed form is non-finite from there on, the recurrence
    stays finite.  This is the documented departure."""
    a = np.float32(0.99)
    t_over = int(np.ceil(np.log(float(np.finfo(np.float32).max)) / -np.log(float(a))))
    assert 8700 < t_over < 8900
    T = t_over + 50
    x = (-60 + np.zeros((T, 2))).astype(np.float32)
    init = R.linspace(-60.0, -90.0, 2, np.float32)
    closed, rec = R.ema_closed(x, a, init), R.ema(x, a, init)
    assert np.isfinite(rec).all()
    # (the running sum of x / a^t, about 100 |x| / a^t, leaves the range some hundred frames before 1 / a^t itself does)
    assert np.isfinite(closed[:7000]).all() and not np.isfinite(closed[t_over + 1:]).any()
    lost = np.abs(closed[4000].astype(np.float64) - R.ema_closed(x.astype(np.float64), a, init)[4000]).max()
    kept = np.abs(rec[4000].astype(np.float64) - R.ema(x.astype(np.float64), a, init)[4000]).max()
    print(f"frame 4000: closed form off by {lost:.3e}, recurrence off by {kept:.3e}")
    assert kept <= 1e-4


# ---------------------------------------------------------------------------------------------- host arithmetic
def test_erb_band_widths():
    assert mas.libdf_erb_band_widths(48000, 960, 32, 2) == PUBLISHED_WIDTHS
    for name in "SWP":
        cfg, _ = R.case(name)
        w = cfg.erb_band_widths
        assert len(w) == cfg.nb_erb and sum(w) == cfg.freq_bins and min(w) >= 1
    cfg = mas.DeepFilterNetConfig(erb_widths=[1] * 31 + [450])
    assert cfg.erb_band_widths == [1] * 31 + [450]
    assert mas.DeepFilterNetConfig(erb_widths=[1] * 32).erb_band_widths == PUBLISHED_WIDTHS      # a sum that does not fit: libDF's


def test_norm_alpha():
    assert mas.compute_norm_alpha(480, 48000) == float(np.float32(0.99))
    assert mas.compute_norm_alpha(96, 48000) == float(np.float32(0.998))


def test_vorbis_window_is_power_complementary():
    for n in (192, 960):
        w = R.vorbis_window(n)
        assert np.abs(w[: n // 2] ** 2 + w[n // 2:] ** 2 - 1).max() < 1e-12


def test_stft_istft_round_trip_and_lengths():
    for name in "SP":
        cfg, W = R.case(name)
        r = R.DeepFilterNetRef(cfg, W)
        hop = cfg.hop_size
        assert [r.frames(n) for n in (0, 1, hop - 1, hop, hop + 1)] == [2, 2, 2, 3, 3]
        for n in (0, 1, hop + 1, 5 * hop + 7):
            x = np.random.default_rng(n).uniform(-0.5, 0.5, n)
            spec = r.stft(x)
            T = r.frames(n)
            assert spec.shape == (T, 2 * cfg.freq_bins)
            coefs = np.zeros((T, cfg.nb_df, cfg.df_order, 2))
            coefs[:, :, cfg.df_order - 1 - cfg.df_lookahead, 0] = 1.0                            # (0, 0, 1 + 0j, 0, 0)
            enh = r.enhanced(spec, np.ones((T, cfg.nb_erb, 1)), coefs)
            inv = r.w("mask.erb_inv_fb")
            assert np.array_equal(inv.sum(axis=0), np.ones(cfg.freq_bins))
            y = r.istft(enh, n)
            assert y.shape == (n,)
            if n:
                assert np.abs(y - x).max() < 1e-6


def test_config_decoding():
    c = mas.DeepFilterNetConfig.from_dict({})
    assert (c.sample_rate, c.fft_size, c.hop_size, c.min_nb_erb_freqs, c.nb_erb, c.nb_df, c.df_order, c.df_lookahead, c.conv_lookahead) == \
        (48000, 960, 480, 2, 32, 96, 5, 2, 2)
    assert (c.conv_ch, c.conv_k_enc, c.conv_k_dec, c.conv_width_factor, c.emb_hidden_dim, c.emb_num_layers, c.df_hidden_dim, c.df_num_layers) == \
        (64, 1, 1, 1, 256, 3, 256, 2)
    assert (c.gru_groups, c.linear_groups, c.enc_linear_groups, c.group_shuffle, c.enc_concat, c.df_gru_skip) == (8, 16, 32, False, False, "groupedlinear")
    assert (list(c.conv_kernel), list(c.convt_kernel), list(c.conv_kernel_inp), c.df_pathway_kernel_size_t, c.lsnr_max, c.lsnr_min) == \
        ([1, 3], [1, 3], [3, 3], 5, 35, -15)
    assert c.model_version == "DeepFilterNet3" and c.model_type == "deepfilternet3" and c.erb_widths is None and c.freq_bins == 481
    c = mas.DeepFilterNetConfig.from_dict({"model_version": "", "hop_size": 240, "erb_widths": [3, 4], "unknown": 1, "nb_df": None}, max_batch=2)
    assert c.model_version == "DeepFilterNet3" and c.hop_size == 240 and c.erb_widths == [3, 4] and c.nb_df == 96 and c.max_batch == 2
    assert mas.DeepFilterNetConfig(model_version="DeepFilterNet2").model_type == "deepfilternet2"
    assert mas.DeepFilterNetConfig(model_version="DeepFilterNet").model_type == "deepfilternet"
    assert abs(c.wnorm - 2 * 240 / 960 ** 2) < 1e-9 and mas.DeepFilterNetConfig(max_seconds=2).max_samples == 96000


def test_expected_shapes():
    for name in "SWP":
        cfg, W = R.case(name)
        want = mas.deepfilternet_expected_shapes(cfg, dict(W, extra=np.zeros(3)))
        assert set(want) == set(W) and list(want)[0] == "mask.erb_inv_fb"
    cfg, W = R.case("S")
    with pytest.raises(mas.DeepFilterNetError) as e:
        mas.deepfilternet_expected_shapes(cfg, {})
    assert e.value.sts_case == "missingWeightKey" and "mask.erb_inv_fb" in str(e.value)
    for key in ("enc.erb_conv2.1.weight", "df_dec.df_gru.gru.bias_hh_l0", "erb_dec.conv0_out.1.running_var"):
        with pytest.raises(mas.DeepFilterNetError) as e:
            mas.deepfilternet_expected_shapes(cfg, {k: v for k, v in W.items() if k != key})
        assert e.value.sts_case == "missingWeightKey" and key in str(e.value)
    for key in ("erb_fb", "df_dec.df_skip.weight"):                                                # optional
        cfg_w, W_w = R.case("W")
        assert key not in mas.deepfilternet_expected_shapes(cfg_w, {k: v for k, v in W_w.items() if k != key})
    fewer = {k: v for k, v in W.items() if not k.startswith("erb_dec.emb_gru.gru.") or k.endswith("_l0")}       # the layer count is the tensors'
    assert "erb_dec.emb_gru.gru.weight_ih_l1" in mas.deepfilternet_expected_shapes(cfg, W)
    assert "erb_dec.emb_gru.gru.weight_ih_l1" not in mas.deepfilternet_expected_shapes(cfg, fewer)
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.deepfilternet_expected_shapes(cfg, dict(W, **{"enc.df_conv1.1.weight": W["enc.df_conv1.1.weight"][:, :3]}))
    assert "enc.df_conv1.1.weight" in str(e.value) and "shape" in str(e.value)


# ---------------------------------------------------------------------------------------------- loader rules, refusals, routing
def _write(d, cfg=None, files=("model.safetensors",)):
    from safetensors.torch import save_file
    os.makedirs(d, exist_ok=True)
    if cfg is not None:
        with open(os.path.join(d, "config.json"), "w") as f:
            json.dump(cfg, f)
    for fn in files:
        save_file({"x": torch.zeros(1)}, os.path.join(d, fn))


def test_from_local_rules(tmp_path):
    d = str(tmp_path)
    with pytest.raises(mas.DeepFilterNetError) as e:
        mas.DeepFilterNet.from_local(d)
    assert e.value.sts_case == "missingConfig" and d in str(e.value)
    with pytest.raises(mas.DeepFilterNetError) as e:
        mas.DeepFilterNet.from_local(d, "v3")
    assert e.value.sts_case == "missingConfig" and os.path.join(d, "v3") in str(e.value)
    _write(os.path.join(d, "v3"), {}, files=())
    with pytest.raises(mas.DeepFilterNetError) as e:
        mas.DeepFilterNet.from_local(d, "v3")
    assert e.value.sts_case == "missingWeights"
    _write(os.path.join(d, "v3"), {}, files=("b.safetensors", "a.SAFETENSORS"))
    with pytest.raises(mas.DeepFilterNetError) as e:                       # the subfolder is used, a file is read, its keys are asked for
        mas.DeepFilterNet.from_local(d, "v3")
    assert e.value.sts_case == "missingWeightKey" and "mask.erb_inv_fb" in str(e.value)
    _write(d, {"model_version": "DeepFilterNet"})                          # the directory's own config.json wins over the subfolder
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.DeepFilterNet.from_local(d, "v3")
    assert "V1" in str(e.value)
    with pytest.raises(mas.DeepFilterNetError) as e:
        mas.DeepFilterNet.from_pretrained(os.path.join(d, "nothing-here"))
    assert e.value.sts_case == "modelPathNotFound"
    with pytest.raises(mas.AudioGenerationError) as e:                     # a file path means its directory
        mas.DeepFilterNet.from_pretrained(os.path.join(d, "model.safetensors"))
    assert "V1" in str(e.value)


def test_refusals_that_need_no_device():
    for kw, word in ((dict(model_version="DeepFilterNet"), "V1"), (dict(enc_concat=True), "enc_concat")):
        with pytest.raises(mas.AudioGenerationError) as e:
            mas.DeepFilterNetConfig(**kw).to_c()
        assert word in str(e.value)
        with pytest.raises(mas.AudioGenerationError):
            mas.DeepFilterNet.from_weights(mas.DeepFilterNetConfig(**kw), {})
    m = object.__new__(mas.DeepFilterNet)
    m.config, m.model_version = mas.DeepFilterNetConfig(max_seconds=0.01), "DeepFilterNet3"
    with pytest.raises(mas.DeepFilterNetError) as e:
        m._row(np.zeros((2, 3)), None)
    assert e.value.sts_case == "invalidAudioShape" and "[2, 3]" in str(e.value)
    with pytest.raises(mas.AudioGenerationError) as e:
        m._row(np.zeros(4), 16000)
    assert "16000" in str(e.value) and "resampler" in str(e.value)
    with pytest.raises(mas.AudioGenerationError) as e:
        m._row(np.zeros(481), None)
    assert "max_seconds" in str(e.value)
    with pytest.raises(mas.DeepFilterNetError) as e:
        m.enhance_streaming(np.zeros(4))
    assert e.value.sts_case == "streamingNotSupportedForModelVersion"
    assert not hasattr(mas.DeepFilterNet, "create_streamer")


def test_factory_routing(tmp_path):
    d = str(tmp_path / "some-dfn-model")
    _write(os.path.join(d, "v3"), {})
    with pytest.raises(mas.DeepFilterNetError) as e:                       # a local dfn directory reaches the loader
        mas.load_sts_model(d)
    assert e.value.sts_case == "missingWeightKey"
    with pytest.raises(mas.DeepFilterNetError):
        mas.load_sts_model(str(tmp_path), model_type="DeepFilterNet3 ")
    with pytest.raises(mas.STSModelError) as e:                            # no directory: unchanged
        mas.load_sts_model("mlx-community/DeepFilterNet-mlx")
    assert "Unsupported STS model type" in str(e.value) and e.value.model_type == "deepfilternet3"


# ---------------------------------------------------------------------------------------------- resources
@pytest.fixture(scope="module")
def usage():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S",
                            os.path.join(ROOT, "mlx-audio-swift_amd", "csrc", "deepfilternet.hip"), "-o", os.path.join(td, "k.s"),
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


def test_deepfilternet_kernels_do_not_spill(usage):
    """No kernel of deepfilternet.hip uses scratch and every one fits 64 KiB of LDS.  The recurrence at hidden size H runs 3 H threads
    a block: 3 H / 64 waves over 4 SIMDs of 512 registers a lane, so at H = 256 (three waves a SIMD) VGPRs + AGPRs stay within 168,
    and an instantiation with KR register columns holds more than KR."""
    mine = {k: v for k, v in usage.items() if "k_dfn_" in k}
    gru = {tuple(int(g) for g in re.search(r"k_dfn_gruILi(\d+)ELi(\d+)E", k).groups()): v for k, v in mine.items() if "k_dfn_gru" in k}
    assert sorted(gru) == [(32, 32), (64, 64), (128, 128), (256, 64), (256, 96), (256, 128)] and len(mine) == len(gru) + 4
    for k, v in mine.items():
        assert v["scratch"] == 0 and v["lds"] <= 65536 and v["vgprs"] + v["agprs"] <= 512, (k, v)
    for (H, KR), v in gru.items():
        waves_per_simd = -(-(3 * H // 64) // 4) if 3 * H >= 64 else 1
        budget = min(512, (512 // waves_per_simd) // 8 * 8)
        assert KR < v["vgprs"] + v["agprs"] <= budget, (H, KR, v, budget)
