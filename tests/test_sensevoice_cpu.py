"""SenseVoice, CPU side: the specification (tests/sensevoice_ref.py) against independent realisations - a layer against torch.nn
(LayerNorm, Linear, scaled_dot_product_attention, a grouped Conv1d with explicit asymmetric padding), the front end against numpy /
scipy, the clamp LFR against the literal one, the facts the reference's own tests keep - and the host mirror (configs, sanitize,
expected keys, language normalisation, rich-info maps, the tokenizer's order of preference, loader errors), the decision seeds the GPU
test relies on, and the resource bounds of the new kernels from the code object's metadata."""
import json
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
import sensevoice_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


# ---------------------------------------------------------------------------------------------- a layer against torch.nn
def _nn_layer(cfg, W, q, x, first):
    e = cfg.encoder_conf
    D, H, k = e.output_size, e.attention_heads, e.kernel_size
    t = lambda n: torch.from_numpy(W[n]).double()

    def lin(name, i, o):
        m = torch.nn.Linear(i, o).double()
        m.weight.data, m.bias.data = t(name + ".weight"), t(name + ".bias")
        return m

    def norm(name, n):
        m = torch.nn.LayerNorm(n, eps=1e-5).double()
        m.weight.data, m.bias.data = t(name + ".weight"), t(name + ".bias")
        return m

    with torch.no_grad():
        x = torch.from_numpy(x).double()
        y = norm(q + ".norm1", x.shape[1])(x)
        qkv = lin(q + ".self_attn.linear_q_k_v", x.shape[1], 3 * D)(y)
        qq, kk, vv = qkv.split(D, dim=-1)
        heads = lambda a: a.reshape(1, -1, H, D // H).transpose(1, 2)
        att = torch.nn.functional.scaled_dot_product_attention(heads(qq), heads(kk), heads(vv)).transpose(1, 2).reshape(-1, D)
        conv = torch.nn.Conv1d(D, D, k, groups=D, bias=False).double()
        conv.weight.data = t(q + ".self_attn.fsmn_block.weight").permute(0, 2, 1)         # [D, k, 1] -> [D, 1, k]
        left = (k - 1) // 2 + max(e.sanm_shift, 0)
        mem = conv(torch.nn.functional.pad(vv.t()[None], (left, k - 1 - left)))[0].t() + vv
        a = lin(q + ".self_attn.linear_out", D, D)(att) + mem
        y = a if first else x + a
        z = norm(q + ".norm2", D)(y)
        return (y + lin(q + ".feed_forward.w_2", e.linear_units, D)(torch.relu(lin(q + ".feed_forward.w_1", D, e.linear_units)(z)))).numpy()


@pytest.mark.parametrize("name", ["A", "B", "F"])
def test_layers_match_torch_nn(name):
    cfg = R.case_config(name)
    W = R.make_weights(cfg, 3)
    ref = R.SenseVoiceRef(cfg, W, None, np.float64)
    g = np.random.default_rng(1)
    for T in (3, 37):                                                 # shorter than the kernel, and longer
        x = g.standard_normal((T, cfg.input_size))
        for i, q in enumerate(ref.prefixes[:2]):
            want = _nn_layer(cfg, W, q, x, i == 0)
            got = ref.layer(i, x)
            assert got.shape == want.shape and np.abs(got - want).max() < 1e-10 * max(1.0, np.abs(want).max()), (name, T, i)
            x = want
    h = g.standard_normal((5, cfg.encoder_conf.output_size))
    ln = torch.nn.LayerNorm(h.shape[1]).double()
    ln.weight.data, ln.bias.data = torch.from_numpy(W["encoder.tp_norm.weight"]).double(), torch.from_numpy(W["encoder.tp_norm.bias"]).double()
    with torch.no_grad():
        assert np.abs(ref.step(ref.stages - 1, h) - ln(torch.from_numpy(h)).numpy()).max() < 1e-12
    z = ref.log_probs_from(h)
    assert np.abs(z - torch.log_softmax(torch.from_numpy(ref.logits(h)), dim=-1).numpy()).max() < 1e-12
    # float32 stays near float64
    x = g.standard_normal((20, cfg.input_size)).astype(np.float32)
    a, b = ref.encoder(x), R.SenseVoiceRef(cfg, W, None, np.float32).encoder(x)
    assert b.dtype == np.float32 and np.abs(a - b).max() < 1e-3 * max(1.0, np.abs(a).max())


# ---------------------------------------------------------------------------------------------- front end
def test_fbank_matches_numpy_scipy():
    import scipy.signal
    cfg = R.case_config("A")
    x = R.tone_row(2, 4000)
    got = R.fbank(x, cfg, np.float64)
    a = x.astype(np.float64) * 32768
    F = 1 + (len(a) - 400) // 160
    assert got.shape == (F, 80)
    win = scipy.signal.get_window("hamming", 400, fftbins=False)
    pts = 700.0 * (10.0 ** (np.linspace(2595 * np.log10(1 + 20 / 700.0), 2595 * np.log10(1 + 8000 / 700.0), 82) / 2595.0) - 1.0)
    fr = np.arange(257) * 16000.0 / 512
    want = np.zeros((F, 80))
    for t in range(F):
        s = a[t * 160: t * 160 + 400]
        s = s - s.mean()
        s = np.concatenate([[s[0] - 0.97 * s[0]], s[1:] - 0.97 * s[:-1]]) * win
        p = np.abs(np.fft.rfft(s, 512)) ** 2
        for j in range(80):
            tri = np.maximum(0.0, np.minimum((fr - pts[j]) / (pts[j + 1] - pts[j]), (pts[j + 2] - fr) / (pts[j + 2] - pts[j + 1])))
            want[t, j] = np.log(max(float(p @ tri), 1e-10))
    assert np.abs(got - want).max() < 1e-9
    assert np.abs(R.fbank(x, cfg, np.float32) - want).max() < 2e-3
    # the peak rule: a row above 1 is not scaled; the hann window; rows below one window
    assert np.allclose(R.fbank(x * np.float32(32768), cfg), got, atol=1e-9)
    hann = R.case_config("B")
    assert np.allclose(R.window("hann", 400, np.float64), scipy.signal.get_window("hann", 400, fftbins=False), atol=1e-15)
    assert R.fbank(x, hann).shape == (F, 40) and R.fbank(x[:399], cfg).shape == (0, 80) and R.fbank(x[:400], cfg).shape == (1, 80)
    assert R.fbank(np.stack([x, x], axis=-1), cfg).shape == (F, 80)
    # the sinusoid: sin | cos halves, cut or zero-padded
    p = R.position_table(3, 5, np.float64)
    assert p.shape == (3, 5) and p[0, 4] == 0.0 and np.isclose(p[1, 0], np.sin(2.0)) and np.isclose(p[1, 2], np.cos(2.0))
    assert R.position_table(2, 1, np.float64).shape == (2, 1)


def test_the_references_held_facts(tmp_path):
    f = np.arange(20, dtype=np.float32)[:, None]
    out = R.lfr_clamp(f, 7, 6)
    assert out.shape == (4, 7) and out[0].tolist() == [0, 0, 0, 0, 1, 2, 3]
    g = np.random.default_rng(0)
    for T in (1, 2, 5, 6, 7, 19, 20, 43):
        for m, n in ((7, 6), (5, 3), (5, 1), (1, 1), (4, 6)):
            x = g.standard_normal((T, 3))
            assert np.array_equal(R.lfr_clamp(x, m, n), R.lfr_literal(x, m, n)), (T, m, n)
    assert R.lfr_clamp(np.zeros((0, 3)), 7, 6).shape == (0, 21) and R.lfr_literal(np.zeros((0, 3)), 7, 6).shape == (0, 21)
    assert R.cmvn_apply(np.asarray([[1.0, 2.0]]), (np.asarray([0.5, -1.0]), np.asarray([2.0, 4.0])), np.float64).tolist() == [[3.0, 4.0]]
    shift, scale = mas.parse_kaldi_cmvn("<Nnet>\n<AddShift> 2 2\n<LearnRateCoef> 0 [ -1.0 0.5 ]\n<Rescale> 2 2\n<LearnRateCoef> 0 [ 2.0 4.0 ]\n</Nnet>")
    assert shift.tolist() == [-1.0, 0.5] and scale.tolist() == [2.0, 4.0]
    (tmp_path / "toy.model").write_bytes(_toy_model_bytes())
    assert mas.SenseVoiceTokenizer.from_model_directory(str(tmp_path)).decode([3, 4]) == "hello world"
    assert R.greedy_ctc([0, 5, 5, 0, 5, 6, 6, 0]) == [5, 5, 6] and R.greedy_ctc([]) == [] and R.greedy_ctc([0, 0]) == []


# ---------------------------------------------------------------------------------------------- host logic
def _toy_model_bytes():
    def varint(v):
        out = b""
        while True:
            b, v = v & 0x7F, v >> 7
            out += bytes([b | (0x80 if v else 0)])
            if not v:
                return out

    def piece(text, score, kind):
        t = text.encode("utf-8")
        body = b"\x0a" + varint(len(t)) + t + b"\x15" + struct.pack("<f", score) + (b"\x18" + varint(kind) if kind != 1 else b"")
        return b"\x0a" + varint(len(body)) + body

    trainer = b"\x12\x04\x08\x01\x10\x02"                             # another field of the ModelProto: skipped
    return trainer + b"".join(piece(t, s, k) for t, s, k in (("<unk>", 0.0, 2), ("<s>", 0.0, 3), ("</s>", 0.0, 3), ("▁hello", -1.0, 1),
                                                             ("▁world", -2.0, 1)))


def test_config_defaults_and_the_misspelled_key():
    c = mas.SenseVoiceConfig()
    e, f = c.encoder_conf, c.frontend_conf
    assert (c.model_type, c.vocab_size, c.input_size, c.cmvn_means, c.cmvn_istd) == ("sensevoice", 25055, 560, None, None)
    assert (e.output_size, e.attention_heads, e.linear_units, e.num_blocks, e.tp_blocks, e.kernel_size, e.sanm_shift, e.normalize_before) == \
        (512, 4, 2048, 50, 20, 11, 0, True)
    assert (e.dropout_rate, e.positional_dropout_rate, e.attention_dropout_rate) == (0.1, 0.1, 0.1)
    assert (f.fs, f.window, f.n_mels, f.frame_length, f.frame_shift, f.lfr_m, f.lfr_n) == (16000, "hamming", 80, 25, 10, 7, 6)
    assert c.num_layers == 70 and mas.SenseVoiceConfig.from_dict({}).encoder_conf.num_blocks == 50
    d = mas.SenseVoiceConfig.from_dict({"encoder_conf": {"sanm_shfit": 3, "num_blocks": None}, "frontend_conf": {"window": "hanning"},
                                        "cmvn_means": [1.0], "cmvn_istd": [2.0], "unknown": 1}, max_batch=2)
    assert d.encoder_conf.sanm_shift == 3 and d.encoder_conf.num_blocks == 50 and d.cmvn_means == [1.0] and d.max_batch == 2
    assert mas.SenseVoiceEncoderConfig.from_dict({"sanm_shift": 1, "sanm_shfit": 3}).sanm_shift == 1
    assert d.to_c().window_hann == 1 and c.to_c().window_hann == 0 and c.to_c().head_rows == 2048


def test_sanitize_and_expected_keys():
    cfg = R.case_config("F")
    W = R.make_weights(cfg, 1)
    assert set(W) == mas.sensevoice_expected_keys(cfg) and len(W) == 1 + 13 + 4 + 2
    assert mas.sensevoice_expected_shapes(cfg)["encoder.encoders0.0.self_attn.fsmn_block.weight"] == (8, 5, 1)
    assert mas.sensevoice_expected_shapes(cfg)["encoder.encoders0.0.norm1.weight"] == (560,)
    A = R.case_config("A")
    assert mas.sensevoice_layer_prefixes(A) == ["encoder.encoders0.0", "encoder.encoders.0", "encoder.encoders.1", "encoder.tp_encoders.0",
                                                "encoder.tp_encoders.1"]
    k = "encoder.encoders0.0.self_attn.fsmn_block.weight"
    raw = {kk.replace("ctc_lo.", "ctc.ctc_lo."): v for kk, v in W.items()}
    raw[k] = np.ascontiguousarray(W[k].transpose(0, 2, 1))            # torch's [channels, 1, kernel]
    for given in (raw, {kk: torch.from_numpy(v) for kk, v in raw.items()}):
        s = mas.sensevoice_sanitize(given)
        assert set(s) == set(W) and tuple(s[k].shape) == (8, 5, 1) and np.array_equal(np.asarray(s[k]), W[k])
        mas.sensevoice_check_weights(cfg, s)
    again = mas.sensevoice_sanitize(W)                                # MLX's layout passes through
    assert tuple(again[k].shape) == (8, 5, 1) and np.array_equal(again[k], W[k])
    for broken, word in (({**W, "extra": W["ctc_lo.bias"]}, "extra"), ({kk: v for kk, v in W.items() if kk != "embed.weight"}, "embed.weight"),
                         ({**W, "ctc_lo.bias": W["ctc_lo.bias"][:3]}, "ctc_lo.bias")):
        with pytest.raises(mas.AudioGenerationError) as e:
            mas.sensevoice_check_weights(cfg, broken)
        assert word in str(e.value)


def test_language_and_rich_info():
    from mlx_audio_swift_amd import sensevoice as S
    n = S.normalized_language
    assert [n(v) for v in (None, "ZH", "Mandarin", "english", "Cantonese", "ja", "Korean", "nospeech", "fr", "auto")] == \
        ["auto", "zh", "zh", "en", "yue", "ja", "ko", "nospeech", "auto", "auto"]
    assert S.LID_IDS == {"auto": 0, "zh": 3, "en": 4, "yue": 7, "ja": 11, "ko": 12, "nospeech": 13} and S.TEXTNORM_IDS == {"withitn": 14, "woitn": 15}
    assert S.rich_info(24885, 25004, 24993) == {"language": "en", "emotion": "neutral", "event": "Speech"}
    assert S.rich_info(1, 2, 3) == {"language": "unknown", "emotion": "token_2", "event": "token_3"}
    assert S.rich_info(24992, 25009, 24999) == {"language": "nospeech", "emotion": "unk", "event": "Applause"}
    assert len(S.LID_MAP) == 6 and len(S.EMO_MAP) == 9 and len(S.EVENT_MAP) == 4
    assert mas.SenseVoiceModel._query("Chinese", True) == (3, 14) and mas.SenseVoiceModel._query(None, False) == (0, 15)
    two = mas.SenseVoiceModel._mono(np.asarray([[1.0, 3.0], [2.0, 4.0]], np.float32))
    assert two.tolist() == [2.0, 3.0]


def test_tokenizer_preference(tmp_path):
    T = mas.SenseVoiceTokenizer
    assert T.from_model_directory(str(tmp_path)).decode([3, 4]) == "3 4"
    (tmp_path / "tokens.json").write_text(json.dumps(["a", "b", "c", "▁x", "▁y"]))
    t = T.from_model_directory(str(tmp_path))
    assert t.tokenizer is None and t.decode([3, 4, 99]) == "x y"
    (tmp_path / "z.model").write_bytes(b"\x0a\x03\x0a\x01q")
    (tmp_path / "toy.model").write_bytes(_toy_model_bytes())
    t = T.from_model_directory(str(tmp_path))                         # the first *.model in name order wins over tokens.json
    assert t.decode([0, 1, 3, 4, 2]) == "<unk> hello world" and t.token_list is not None
    (tmp_path / "tokenizer.json").write_text(json.dumps({"model": {"vocab": [["<unk>", 0], ["▁from", -1], ["▁json", -2]]},
                                                         "added_tokens": [{"id": 0, "special": True}]}))
    assert T.from_model_directory(str(tmp_path)).decode([0, 1, 2]) == "from json"
    pieces = mas.read_sentencepiece_pieces(_toy_model_bytes())
    assert [p for p, _, _ in pieces] == ["<unk>", "<s>", "</s>", "▁hello", "▁world"] and [k for _, _, k in pieces] == [2, 3, 3, 1, 1]
    assert pieces[4][1] == -2.0
    with pytest.raises(mas.AudioGenerationError):
        mas.read_sentencepiece_pieces(b"\x0a\x7f\x01")


def test_loader_errors(tmp_path):
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.sensevoice_read_directory(str(tmp_path))
    assert "config.json" in str(e.value)
    (tmp_path / "config.json").write_text("{}")
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.sensevoice_read_directory(str(tmp_path))
    assert "safetensors" in str(e.value)
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.SenseVoiceModel.from_pretrained(str(tmp_path / "nothing"))
    assert "local" in str(e.value)
    from safetensors.torch import save_file
    cfg = R.case_config("F")
    W = R.make_weights(cfg, 1)
    e_, f_ = cfg.encoder_conf, cfg.frontend_conf
    body = {"vocab_size": 6, "input_size": 560, "cmvn_means": [0.0] * 560, "cmvn_istd": [1.0] * 560,
            "encoder_conf": {"output_size": 8, "attention_heads": 2, "linear_units": 16, "num_blocks": 1, "tp_blocks": 0, "kernel_size": 5}}
    (tmp_path / "config.json").write_text(json.dumps(body))
    t = {k: torch.from_numpy(v) for k, v in W.items()}
    save_file({k: v for k, v in t.items() if k < "f"}, str(tmp_path / "a.safetensors"))
    save_file({k: v for k, v in t.items() if k >= "c"}, str(tmp_path / "b.safetensors"))
    c2, W2, cmvn, tok = mas.sensevoice_read_directory(str(tmp_path), max_batch=2)
    assert set(W2) == set(W) and c2.max_batch == 2 and tok is None and cmvn[1].tolist() == [1.0] * 560          # the config's lists
    (tmp_path / "am.mvn").write_text("<AddShift> 2 2 <LearnRateCoef> 0 [ 1 2 ] <Rescale> 2 2 <LearnRateCoef> 0 [ 3 4 ]")
    assert mas.sensevoice_read_directory(str(tmp_path))[2][0].tolist() == [1.0, 2.0]                            # am.mvn wins
    save_file({"stray.weight": t["ctc_lo.bias"]}, str(tmp_path / "c.safetensors"))
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.sensevoice_read_directory(str(tmp_path))
    assert "stray.weight" in str(e.value)


# ---------------------------------------------------------------------------------------------- decision seeds
def test_decision_seeds():
    """What test_gpu_sensevoice.py::test_decisions relies on: at the decision seed the float32 specification alone leaves at most 1 % of
    the frames exempt (a frame is sure when the float64 top-2 log-prob margin is at least 8 x the float32-to-float64 gap at that frame),
    and the rows decode to something: tokens, repeats and blanks all occur."""
    cfg = R.case_config("A")
    W, cmvn = R.make_weights(cfg, R.DECISION_SEED), R.make_cmvn(cfg, R.DECISION_SEED)
    r32, r64 = R.SenseVoiceRef(cfg, W, cmvn, np.float32), R.SenseVoiceRef(cfg, W, cmvn, np.float64)
    exempt = frames = tokens = repeats = 0
    for i in range(8):
        x = R.tone_row(500 + i, 32000 + 3000 * i)
        l64, l32 = r64.log_probs(x), r32.log_probs(x)
        top = np.sort(l64, axis=1)
        sure = (top[:, -1] - top[:, -2]) >= 8 * np.abs(l32 - l64).max(axis=1)
        exempt += int((~sure).sum()); frames += len(sure)
        p64, p32 = l64.argmax(axis=1), l32.argmax(axis=1)
        assert np.array_equal(p64[sure], p32[sure])
        tokens += len(R.greedy_ctc(p64[4:].tolist())); repeats += int((p64[5:] == p64[4:-1]).sum())
    print(f"decision seeds: {exempt}/{frames} exempt, {tokens} tokens, {repeats} repeated frames")
    assert exempt <= 0.01 * frames and tokens >= 8 and repeats >= 8


# ---------------------------------------------------------------------------------------------- resources
@pytest.fixture(scope="module")
def usage():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S",
                            os.path.join(ROOT, "mlx-audio-swift_amd", "csrc", "sensevoice.hip"), "-o", os.path.join(td, "k.s"),
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


def test_sensevoice_kernels_stay_within_their_bounds(usage):
    """No kernel of sensevoice.hip uses scratch.  DESIGN.md's figures: the 64 x 64 contraction stays within 96 VGPRs (five waves a SIMD)
    with 17,408 B of LDS plain, 17,920 B with the arg-max hand-over and 50,560 B with the memory block's time tile + halo (three blocks a
    CU); the attention kernel holds its query fragments in registers - within 128 VGPRs up to d_k 64, within 256 at d_k 128 (two waves a
    SIMD) - and its two 32-key tiles take 2 x 32 x (HD + 1) x 4 B of LDS: 8,448 / 16,640 / 33,024 B (four blocks a CU at d_k 128)."""
    mine = {k: v for k, v in usage.items() if "k_sv_" in k}
    assert len([k for k in mine if "k_sv_gemm" in k]) == 3 and len([k for k in mine if "k_sv_attn" in k]) == 3 and len(mine) == 12
    for k, v in mine.items():
        assert v["scratch"] == 0 and v["lds"] <= 65536, (k, v)
        if "k_sv_gemm" in k:
            assert v["vgprs"] <= 96 and v["lds"] == {"ILi0E": 17408, "ILi1E": 50560, "ILi2E": 17920}[re.search(r"ILi\dE", k).group(0)], (k, v)
        elif "k_sv_attn" in k:
            nd = int(re.search(r"ILi(\d)E", k).group(1))
            assert v["vgprs"] <= (256 if nd == 4 else 128) and v["lds"] == 2 * 32 * (32 * nd + 1) * 4, (k, v)
        else:
            assert v["vgprs"] <= 64, (k, v)
