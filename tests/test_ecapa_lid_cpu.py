"""CPU tier of the language-identification family: the reference of the GPU tests (tests/ecapa_lid_ref.py) is held to independent
realisations (numpy / scipy for the front end, torch.nn for the layers), and the host side of mlx_audio_swift_amd.lid (config, sanitize,
labels, directory parsing) to the facts the reference's EcapaTdnnConfigTests / SanitizeTests / ModelTests hold, all without a GPU."""
import json
import os
import re

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
import ecapa_lid_ref as er
from mlx_audio_swift_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- front end
def _mel_numpy(wave, n_mels=60):
    """The same front end from its description alone, float64: scipy's periodic Hamming window, np.fft.rfft, HTK triangles."""
    from scipy.signal import get_window
    x = np.concatenate([np.zeros(200), np.asarray(wave, np.float64), np.zeros(200)])
    T = 1 + (len(x) - 400) // 160
    win = get_window("hamming", 400, fftbins=True)
    power = np.stack([np.abs(np.fft.rfft(x[t * 160: t * 160 + 400] * win)) ** 2 for t in range(T)])
    hz = lambda m: 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    pts = hz(np.linspace(0.0, 2595.0 * np.log10(1.0 + 8000.0 / 700.0), n_mels + 2))
    f = np.arange(201) * 40.0
    fb = np.zeros((201, n_mels))
    for j in range(n_mels):
        lo, ce, hi = pts[j], pts[j + 1], pts[j + 2]
        fb[:, j] = np.where((f >= lo) & (f < ce), (f - lo) / (ce - lo), np.where((f >= ce) & (f <= hi), (hi - f) / (hi - ce), 0.0))
    db = 10.0 * np.log10(np.maximum(power @ fb, 1e-10))
    return np.maximum(db, db.max() - 80.0)


def test_mel_reference_against_numpy_and_its_float32_distance():
    """float64 reference = the numpy realisation; the float32 reference stays inside the stage-0 bounds of test_gpu_ecapa_lid.py
    (test_gpu_mel.py's, times 10 for 10 log10) on every case row, so those bounds are used as they are."""
    worst = [0.0, 0.0, 0.0]
    for row in er.case_rows():
        r64 = er.mel_db(row, 60, torch.float64).numpy()
        assert r64.shape == (er.frames_of(len(row)), 60)
        assert np.abs(r64 - _mel_numpy(row)).max() < 1e-8
        d = np.abs(er.mel_db(row, 60, torch.float32).numpy().astype(np.float64) - r64)
        worst = [max(worst[0], d.max()), max(worst[1], float(np.mean(d > 1e-3))), max(worst[2], float(np.sqrt(np.mean(d ** 2))))]
    print("ecapa mel f32 vs f64: max %.3g dB, share beyond 1e-3 dB %.3g, rms %.3g dB" % tuple(worst))
    assert worst[0] < 2e-2 and worst[1] < 1e-3 and worst[2] < 2e-4, worst
    quiet = er.mel_db(er.case_rows()[4], 60, torch.float64)
    assert float((quiet == quiet.max() - 80.0).double().mean()) > 0.2      # the top_db floor binds on the 7999 row
    silent = er.mel_db(np.zeros(4000, np.float32), 60, torch.float32)
    assert torch.all(silent == -100.0) and torch.all(er.sentence_mean_normalize(silent) == 0.0)
    assert [er.frames_of(n) for n in er.CASE_LENS[:3]] == [1, 2, 11]


# ---------------------------------------------------------------------------------------------------- layers
def _bn_module(ref, p, n):
    m = torch.nn.BatchNorm1d(n, eps=1e-5).double().eval()
    with torch.no_grad():
        m.weight.copy_(ref.W[p + ".weight"]); m.bias.copy_(ref.W[p + ".bias"])
        m.running_mean.copy_(ref.W[p + ".running_mean"]); m.running_var.copy_(ref.W[p + ".running_var"])
    return m


def test_layers_against_torch_nn():
    cfg = er.case_config("S64")
    ref = er.EcapaLidRef(cfg, er.make_weights(cfg, 3), torch.float64)
    g = torch.Generator().manual_seed(0)
    C, H, T = cfg.channels, cfg.channels // 8, 37
    x = torch.randn(T, H, generator=g, dtype=torch.float64)
    p = "embedding_model.block3.res2net_block.blocks.2"
    conv = torch.nn.Conv1d(H, H, 3, dilation=4, padding="same").double()
    with torch.no_grad():
        conv.weight.copy_(ref.W[p + ".conv.weight"].permute(0, 2, 1)); conv.bias.copy_(ref.W[p + ".conv.bias"])
        want = _bn_module(ref, p + ".norm", H)(torch.relu(conv(x.t()[None])))[0].t()
    assert torch.allclose(ref.tdnn(x, p, 4), want, atol=1e-12)
    with torch.no_grad():                                             # a row shorter than the dilated kernel: zero padding, not reflection
        short = _bn_module(ref, p + ".norm", H)(torch.relu(conv(x[:3].t()[None])))[0].t()
    assert torch.allclose(ref.tdnn(x[:3], p, 4), short, atol=1e-12)
    # SE: gate from the mean over time
    y = torch.randn(T, C, generator=g, dtype=torch.float64)
    q = "embedding_model.block1.se_block"
    s = torch.relu(ref.W[q + ".conv1.weight"][:, 0] @ y.mean(0) + ref.W[q + ".conv1.bias"])
    gate = torch.sigmoid(ref.W[q + ".conv2.weight"][:, 0] @ s + ref.W[q + ".conv2.bias"])
    assert torch.allclose(ref.se(y, q), y * gate, atol=1e-12)
    # ASP written out per channel
    z = torch.randn(T, 3 * C, generator=g, dtype=torch.float64)
    a = "embedding_model.asp"
    ctx = torch.cat([z, z.mean(0).expand(T, -1), torch.sqrt(z.var(0, unbiased=False) + 1e-9).expand(T, -1)], dim=1)
    hid = torch.relu(ctx @ ref.W[a + ".tdnn.conv.weight"][:, 0].t() + ref.W[a + ".tdnn.conv.bias"])
    with torch.no_grad():
        hid = torch.tanh(_bn_module(ref, a + ".tdnn.norm", cfg.attention_channels)(hid.t()[None])[0].t())
    att = torch.softmax(hid @ ref.W[a + ".conv.weight"][:, 0].t() + ref.W[a + ".conv.bias"], dim=0)
    mean = (att * z).sum(0)
    sd = torch.sqrt(torch.clamp((att * z * z).sum(0) - mean ** 2, min=1e-9))
    assert torch.allclose(ref.asp(z, a), torch.cat([mean, sd]), atol=1e-12)
    # the whole model: shapes of every stage, log-probabilities that sum to one
    st = ref.stages(er.sentence_mean_normalize(er.mel_db(er.case_rows()[2], 60, torch.float64)))
    assert [tuple(st[k].shape) for k in range(2, 10)] == [(11, C)] * 4 + [(11, 3 * C), (6 * C,), (cfg.embedding_dim,), (cfg.num_classes,)]
    assert abs(float(torch.exp(st[9]).sum()) - 1.0) < 1e-12


def test_decision_seed_separates_the_case_rows():
    cfg = er.case_config("S128")
    ref = er.EcapaLidRef(cfg, er.make_weights(cfg, er.DECISION_SEED), torch.float32)
    for row in er.case_rows():
        lp = torch.sort(ref.log_probs(row), descending=True).values
        assert float(lp[0] - lp[1]) >= 1e-2 and len(set(lp[:5].tolist())) == 5, lp[:5]


# ---------------------------------------------------------------------------------------------------- host side
def test_config_defaults_and_json_keys():
    c = mas.EcapaTdnnConfig.from_dict({})
    assert (c.n_mels, c.channels, c.kernel_sizes, c.dilations, c.attention_channels, c.res2net_scale, c.se_channels, c.embedding_dim,
            c.classifier_hidden_dim, c.num_classes, c.id2label) == (60, 1024, [5, 3, 3, 3, 1], [1, 2, 3, 4, 1], 128, 8, 128, 256, 512, 107, None)
    d = mas.EcapaTdnnConfig.from_dict({"n_mels": 60, "channels": 1024, "embedding_dim": 256,
                                       "id2label": {"0": "en: English", "1": "fr: French", "2": "de: German"}, "unknown": 1})
    assert d.num_classes == 3 and d.id2label["2"] == "de: German"
    assert mas.EcapaTdnnConfig.from_dict({"num_classes": 7, "id2label": {"0": "a"}}).num_classes == 7
    e = mas.EcapaTdnnConfig(n_mels=40, channels=512, num_classes=50)
    assert (e.n_mels, e.channels, e.num_classes, e.embedding_dim) == (40, 512, 50, 256)
    cc = mas.EcapaTdnnConfig(max_batch=4, max_samples=8000).to_c()
    assert (list(cc.kernel_sizes), list(cc.dilations), cc.num_classes, cc.max_batch, cc.max_samples) == ([5, 3, 3, 3, 1], [1, 2, 3, 4, 1], 107, 4, 8000)
    with pytest.raises(mas.AudioGenerationError):
        mas.EcapaTdnnConfig(kernel_sizes=[5, 3]).to_c()


def test_sanitize_rewrites():
    z = np.zeros(1, np.float32)
    raw = {"embedding_model.blocks.0.conv.conv.weight": z, "embedding_model.blocks.0.conv.conv.bias": z,
           "embedding_model.blocks.0.norm.norm.weight": z, "embedding_model.blocks.0.norm.norm.num_batches_tracked": z,
           "embedding_model.blocks.1.tdnn1.conv.conv.weight": z, "embedding_model.blocks.2.tdnn1.conv.conv.weight": z,
           "embedding_model.blocks.3.tdnn1.conv.conv.weight": z, "embedding_model.blocks.1.se_block.conv1.conv.weight": z,
           "embedding_model.blocks.1.se_block.conv2.conv.weight": z, "embedding_model.asp_bn.norm.weight": z,
           "embedding_model.fc.conv.weight": z, "embedding_model.blocks.1.res2net_block.blocks.0.conv.conv.weight": z,
           "embedding_model.blocks.1.res2net_block.blocks.1.conv.conv.weight": z, "classifier.out.w.weight": z}
    assert set(mas.ecapa_lid_sanitize(raw)) == {
        "embedding_model.block0.conv.weight", "embedding_model.block0.conv.bias", "embedding_model.block0.norm.weight",
        "embedding_model.block1.tdnn1.conv.weight", "embedding_model.block2.tdnn1.conv.weight", "embedding_model.block3.tdnn1.conv.weight",
        "embedding_model.block1.se_block.conv1.weight", "embedding_model.block1.se_block.conv2.weight", "embedding_model.asp_bn.weight",
        "embedding_model.fc.weight", "embedding_model.block1.res2net_block.blocks.0.conv.weight",
        "embedding_model.block1.res2net_block.blocks.1.conv.weight", "classifier.out.w.weight"}
    assert mas.EcapaTdnnLID.sanitize is mas.ecapa_lid_sanitize
    cfg = er.case_config("S64")
    W = er.make_weights(cfg, 1)
    back = mas.ecapa_lid_sanitize(er.raw_checkpoint(W))               # raw_checkpoint is sanitize's inverse
    assert set(back) == set(W) == set(mas.ecapa_lid_expected_shapes(cfg)) and all(torch.equal(back[k], W[k]) for k in W)
    assert len(er.raw_checkpoint(W)) > len(W)


def test_labels_and_ranking():
    assert mas.ecapa_lid_labels({"0": "en: English", "1": "ceb: Cebuano", "x": "?", "2": " plain "}) == {0: "en", 1: "ceb", 2: "plain"}
    assert mas.ecapa_lid_labels(None) == {}
    cfg = er.case_config("S64")
    ref = er.EcapaLidRef(cfg, er.make_weights(cfg, 2), torch.float32)
    lp = ref.log_probs(er.case_rows()[3])[None]
    assert tuple(lp.shape) == (1, 10)                                 # [1, classes]
    idx, p = er.top_k(lp[0], 3)
    assert len(idx) == 3 and np.all(np.diff(p) <= 0)
    assert len(er.top_k(lp[0], 500)[0]) == 10                         # clamped


def test_directory_round_trip(tmp_path):
    from safetensors.torch import save_file
    cfg = er.case_config("S64")
    W = er.make_weights(cfg, 4)
    raw = er.raw_checkpoint(W)
    names = sorted(raw)
    with pytest.raises(mas.LIDError) as e:
        mas.ecapa_lid_read_directory(str(tmp_path))
    assert e.value.lid_case == "configNotFound" and "config.json" in str(e.value)
    body = {k: getattr(cfg, k) for k in ("n_mels", "channels", "kernel_sizes", "dilations", "attention_channels", "res2net_scale",
                                         "se_channels", "embedding_dim", "classifier_hidden_dim")}
    (tmp_path / "config.json").write_text(json.dumps(body))
    with pytest.raises(mas.LIDError) as e:
        mas.ecapa_lid_read_directory(str(tmp_path))
    assert e.value.lid_case == "noLabels"
    (tmp_path / "config.json").write_text(json.dumps({**body, "id2label": cfg.id2label}))
    with pytest.raises(mas.LIDError) as e:
        mas.ecapa_lid_read_directory(str(tmp_path))
    assert e.value.lid_case == "weightsNotFound" and "safetensors" in str(e.value)
    half = len(names) // 2                                             # two files, read in name order; the later file wins a shared key
    save_file({k: raw[k].contiguous() for k in names[:half]} | {names[-1]: torch.zeros_like(raw[names[-1]])}, str(tmp_path / "a.safetensors"))
    save_file({k: raw[k].contiguous() for k in names[half:]}, str(tmp_path / "b.safetensors"))
    got_cfg, got = mas.ecapa_lid_read_directory(str(tmp_path), max_batch=2, max_samples=4000)
    assert (got_cfg.num_classes, got_cfg.channels, got_cfg.max_batch, got_cfg.max_samples) == (10, 64, 2, 4000)
    assert set(got) == set(W) and all(torch.equal(got[k], W[k]) for k in W)
    assert {k: tuple(v.shape) for k, v in got.items()} == mas.ecapa_lid_expected_shapes(got_cfg)
    save_file({"embedding_model.extra.weight": torch.zeros(1)}, str(tmp_path / "c.safetensors"))
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.ecapa_lid_read_directory(str(tmp_path))
    assert e.value.case == "invalidInput" and "extra" in str(e.value)


def test_header_and_binding_carry_the_abi():
    txt = open(os.path.join(ROOT, "include", "mi_speech.h")).read()
    for name in ("create", "set_tensor", "init_synthetic", "finalize", "destroy", "predict", "forward_features", "tap", "launches"):
        assert re.search(r"\bmis_ecapa_lid_%s\s*\(" % name, txt), name
        assert "mis_ecapa_lid_" + name in _lib.SYMBOLS
    import ctypes as C
    assert C.sizeof(_lib.EcapaLidConfigC) == 4 * (2 + 5 + 5 + 6 + 2)
    assert hasattr(C.CDLL(_lib.LIB_PATH), "mis_ecapa_lid_predict")
    bad = mas.EcapaTdnnConfig(kernel_sizes=[5, 3, 4, 3, 1]).to_c()      # the configuration is judged before the device is touched
    h = C.c_void_p()
    assert _lib.lib().mis_ecapa_lid_create(C.byref(bad), 0, C.byref(h)) == 3 and "kernel_sizes[2]" in _lib.last_error()
    assert _lib.lib().mis_ecapa_lid_launches(None) == 0
