"""LASR CTC, CPU side: the float64/float32 reference (tests/lasr_ref.py) against independent implementations - the model body against
transformers' LasrForCTC, the front end against scipy.signal and a written-out slaney filter bank - and the host mirror (config
parsing, sanitize, greedy CTC, tokenizer), the decision margins the GPU test relies on, and the ISA bounds of the two new hot kernels."""
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import mlx_audio_swift_amd as mas
import lasr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _rel(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2) / np.mean(np.asarray(b, np.float64) ** 2)))


# ---------------------------------------------------------------------------------------------- model body against transformers
@pytest.mark.parametrize("name", ["B", "H"])
def test_model_body_matches_transformers(name):
    """LasrForCTC (transformers.models.lasr) with the same weights, float32, against the reference's float32 realisation; the gate is
    10 x the distance between the reference's own float32 and float64 realisations.  Where HF's module and the Swift file differ, the
    Swift file wins:
      * HF's LayerNorms are created with bias=False; the Swift LayerNorm has a bias (zero unless a checkpoint sets it).  The
        comparison runs without LayerNorm biases - the one configuration both can express;
      * BatchNorm eps: 1e-5 in both (torch default, MLXNN default);
      * padding for even k: HF's padding="same" puts (k - 1) / 2 in front and the larger half behind, the Swift split (:146-147);
      * residual weights: the same a * residual + b * module in both."""
    torch = pytest.importorskip("torch")
    tl = pytest.importorskip("transformers.models.lasr")
    cfg = R.case_config(name)
    W = {k: v for k, v in R.make_weights(cfg, 11).items() if not ("norm" in k and k.endswith(".bias") and "conv.norm" not in k)}
    e = dict(cfg["encoder_config"])
    e["rope_parameters"] = {"rope_theta": e.pop("rope_theta"), "rope_type": "default"}
    hf_cfg = tl.LasrCTCConfig(vocab_size=cfg["vocab_size"], pad_token_id=cfg["pad_token_id"], encoder_config=e)
    model = tl.LasrForCTC(hf_cfg).eval().float()
    sd = {}
    for k, v in W.items():
        t = torch.from_numpy(v)
        if "conv" in k and k.endswith(".weight") and t.ndim == 3:
            t = t.permute(0, 2, 1).contiguous()                    # [out, k, in] -> torch's [out, in, k]
        if k == "ctc_head.weight":
            t = t[:, :, None]
        sd[k] = t
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("num_batches_tracked" in m or "inv_freq" in m for m in missing), (missing, unexpected)
    feats = np.random.default_rng(5).standard_normal((70, cfg["encoder_config"]["num_mel_bins"])).astype(np.float32)
    with torch.no_grad():
        hf = model(input_features=torch.from_numpy(feats)[None]).logits[0].numpy()
    r32 = R.Ref(cfg, W, acc=np.float32).forward(feats)["logits"]
    r64 = R.Ref(cfg, W, acc=np.float64).forward(feats)["logits"]
    own, dist = _rel(r32, r64), _rel(hf, r32)
    print(f"lasr {name}: |ref32 - ref64| {own:.3e}  |hf - ref32| {dist:.3e}  |hf - ref64| {_rel(hf, r64):.3e}")
    assert hf.shape == r32.shape and own < 1e-5
    assert dist <= 10 * own, (dist, own)


# ---------------------------------------------------------------------------------------------- front end
def _front_end_scipy(x, mels):
    """An independent front end: scipy.signal for the pre-emphasis filter, the window and the STFT; the slaney bank written out."""
    sig = pytest.importorskip("scipy.signal")
    x = np.asarray(x, np.float64)
    if len(x) > 1:
        y = sig.lfilter([1.0, -0.97], [1.0], x)
        y[0] = x[0]
    else:
        y = x
    win = np.zeros(512)
    win[56:456] = sig.get_window("hann", 400, fftbins=False)
    p = np.concatenate([np.zeros(256), y, np.zeros(256)])
    F = 1 + len(x) // 160
    power = np.stack([np.abs(np.fft.rfft(p[t * 160: t * 160 + 512] * win)) ** 2 for t in range(F)])

    def mel2hz(m):
        return 200.0 / 3.0 * m if m < 15 else 1000.0 * 6.4 ** ((m - 15) / 27.0)

    top = 15.0 + 27.0 * np.log(8.0) / np.log(6.4)
    edges = [mel2hz(top * i / (mels + 1)) for i in range(mels + 2)]
    freqs = np.arange(257) * 31.25
    fb = np.zeros((257, mels))
    for j in range(mels):
        lo, ce, hi = edges[j: j + 3]
        fb[:, j] = np.maximum(0.0, np.minimum((freqs - lo) / (ce - lo), (hi - freqs) / (hi - ce))) * 2.0 / (hi - lo)
    mel = np.log(power @ fb + 2.0 ** -24)
    std = mel.std(axis=0, ddof=1) if F > 1 else np.zeros(mels)
    return (mel - mel.mean(axis=0)) / (std + 1e-5)


@pytest.mark.parametrize("n", [1, 159, 160, 161, 48000])
def test_front_end_matches_scipy(n):
    x = (0.1 * np.random.default_rng(n).standard_normal(n)).astype(np.float32)
    got, want = R.front_end(x, 40), _front_end_scipy(x, 40)
    assert got.shape == want.shape == (1 + n // 160, 40)
    assert np.abs(got - want).max() < 1e-7 * max(1.0, np.abs(want).max())
    f32 = R.front_end(x, 40, np.float32)
    assert f32.dtype == np.float32 and (n < 1000 or _rel(f32, want) < 1e-3)


def test_frame_counts_follow_the_conv_arithmetic():
    torch = pytest.importorskip("torch")
    for k, s in ((5, 2), (3, 2), (2, 1), (8, 4)):
        conv = torch.nn.Conv1d(1, 1, k, stride=s)
        for F in list(range(1, 70)) + [1001, 3001]:
            t1 = R.conv_out(F, k, s)
            t2 = R.conv_out(t1, k, s)
            if F >= k:
                assert conv(torch.zeros(1, 1, F)).shape[-1] == t1
            if t1 >= k:
                assert conv(torch.zeros(1, 1, t1)).shape[-1] == t2
            else:
                assert t2 == 0
    assert [R.frames_of(n) for n in (0, 159, 160, 16000)] == [1, 1, 2, 101]
    assert R.t2_of(R.case_config("A"), 160000) == 248


# ---------------------------------------------------------------------------------------------- host mirror
def test_config_decodes_nested_encoder_and_rope_parameters():
    c = mas.LasrCTCConfig.from_dict(json.loads("""{"vocab_size": 2000, "pad_token_id": 1, "ctc_loss_reduction": "sum",
        "encoder_config": {"hidden_size": 128, "num_hidden_layers": 4, "num_mel_bins": 80,
                           "rope_parameters": {"rope_theta": 5000.0, "rope_type": "default"}}}"""))
    e = c.encoder_config
    assert (c.vocab_size, c.pad_token_id, c.ctc_loss_reduction, c.model_type) == (2000, 1, "sum", "lasr")
    assert (e.hidden_size, e.num_hidden_layers, e.num_mel_bins, e.rope_theta, e.rope_type) == (128, 4, 80, 5000.0, "default")
    assert (e.num_attention_heads, e.num_key_value_heads, e.conv_kernel_size, e.intermediate_size) == (8, 8, 32, 2048)
    assert e.conv_residual_weights == [2.0, 1.0] and e.feed_forward_residual_weights == [1.5, 0.5] and e.layer_norm_eps == 1e-6
    d = mas.LasrCTCConfig()
    assert (d.vocab_size, d.encoder_config.num_hidden_layers, d.encoder_config.subsampling_conv_channels) == (512, 17, 256)
    assert mas.LasrEncoderConfig.from_dict({"num_attention_heads": 4}).num_key_value_heads == 4
    assert mas.LasrEncoderConfig.from_dict({"rope_theta": 7.0, "rope_parameters": {"rope_type": "linear"}}).rope_type == "linear"
    cc = c.to_c()
    assert (cc.vocab_size, cc.hidden_size, cc.rope_type, cc.hidden_act, cc.pad_token_id) == (2000, 128, 0, 0, 1)
    assert abs(cc.rope_theta - 5000.0) < 1e-3 and list(cc.conv_residual_weights) == [2.0, 1.0]


def test_sanitizer_transposes_conv_and_squeezes_ctc_head():
    out = mas.lasr_sanitize({"encoder.layers.0.conv.depthwise_conv.weight": np.ones((32, 1, 5), np.float32),
                             "ctc_head.weight": np.ones((12, 32, 1), np.float32),
                             "encoder.rotary_emb.inv_freq": np.ones(4, np.float32),
                             "encoder.layers.0.conv.norm.num_batches_tracked": np.zeros((), np.int64)})
    assert out["encoder.layers.0.conv.depthwise_conv.weight"].shape == (32, 5, 1)
    assert out["ctc_head.weight"].shape == (12, 32)
    assert set(out) == {"encoder.layers.0.conv.depthwise_conv.weight", "ctc_head.weight"}


def test_greedy_ctc_hand_cases():
    def logits(ids, V=6):
        x = np.zeros((1, len(ids), V), np.float32)
        x[0, np.arange(len(ids)), ids] = 1.0
        return x

    g = mas.greedy_ctc_tokens
    assert g(logits([1, 1, 0, 1, 2, 2, 0, 0, 3]), 0) == [[1, 1, 2, 3]]        # a repeat across a blank is kept
    assert g(logits([0, 0, 4, 4, 5]), 0) == [[4, 5]]                          # leading blank
    assert g(logits([0, 0, 0]), 0) == [[]]                                    # all blank
    assert g(logits([0, 3, 3, 0, 3, 1]), 3) == [[0, 0, 1]]                    # pad_token_id != 0: 0 is a token, 3 the blank
    assert g(logits([1, 2, 3]), 0, frames=[2]) == [[1, 2]]                    # the row's own frame count
    tie = np.zeros((1, 2, 4), np.float32)
    tie[0, 1, 2:] = 1.0
    assert g(tie, 1) == [[0, 2]]                                              # ties go to the lowest index
    assert R.greedy_ctc(logits([1, 1, 0, 1, 2, 2, 0, 0, 3])[0], 0) == [1, 1, 2, 3]


def test_tokenizer_decode_folds_byte_pieces():
    pieces = ["<pad>", "▁he", "llo", "▁wor", "ld", "<0xC3>", "<0xA9>", "<0x41>", "▁", "<0xZZ>"]
    tok = mas.SentencePieceTokenizer(pieces, control={0})
    assert tok.decode([1, 2, 3, 4]) == "he llo wor ld".replace("he llo", "hello").replace("wor ld", "world")
    assert tok.decode([0, 1, 2, 99, -1]) == "hello"                           # control piece and ids out of range are skipped
    assert tok.decode([1, 5, 6, 2]) == "heéllo"                               # <0xC3><0xA9> is one character
    assert tok.decode([5, 2]) == "llo"                                        # an invalid byte run is dropped
    assert tok.decode([8, 7, 8]) == "A"
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "tokenizer.json")
        with open(p, "w", encoding="utf-8") as f:
            json.dump({"model": {"type": "Unigram", "vocab": [[t, 0.0] for t in pieces]},
                       "added_tokens": [{"id": 0, "content": "<pad>", "special": True}]}, f)
        assert mas.SentencePieceTokenizer.from_tokenizer_json(p).decode([0, 3, 4]) == "world"


def test_expected_keys_follow_the_bias_switches():
    for name in ("A", "B"):
        cfg = R.case_config(name)
        assert set(R.make_weights(cfg, 1)) == mas.lasr_expected_keys(mas.LasrCTCConfig.from_dict(cfg))


# ---------------------------------------------------------------------------------------------- decision margins
@pytest.mark.parametrize("name", ["A", "B"])
def test_decision_margins(name):
    """The GPU decision test compares tokens and may exempt 1 % of the frames.  That only means something if rounding alone does not
    move the arg-max: the bf16-rounding reference and the float64 one must agree on at least 99 % of the frames."""
    cfg = R.case_config(name)
    W = R.make_weights(cfg, R.DECISION_SEED)
    rng = np.random.default_rng(R.DECISION_SEED)
    agree = total = 0
    for n in (16000, 19333, 24000, 30001):
        feats = R.front_end(0.1 * rng.standard_normal(n), cfg["encoder_config"]["num_mel_bins"])
        a = R.Ref(cfg, W, round=True, acc=np.float32).forward(feats)["logits"]
        b = R.Ref(cfg, W).forward(feats)["logits"]
        agree += int((a.argmax(-1) == b.argmax(-1)).sum())
        total += len(a)
    print(f"lasr {name}: arg-max agreement {agree}/{total}")
    assert agree >= 0.99 * total


# ---------------------------------------------------------------------------------------------- ISA
@pytest.fixture(scope="module")
def usage():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S",
                            os.path.join(ROOT, "mlx-audio-swift_amd", "csrc", "lasr.hip"), "-o", os.path.join(td, "k.s"),
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


def test_lasr_kernels_do_not_spill(usage):
    """No kernel of lasr.hip uses scratch, the log-mel front end it shares with sortformer.hip (k_nemo_*, csrc/audio_front.h) included.
    The attention kernel stays within 128 VGPRs (four of its 256-thread blocks' waves per SIMD), the GLU + depthwise kernel within 64
    (its 16 accumulators, not its up to 64 taps, live in registers) with the 32.5 KB tile + halo in LDS."""
    names = {re.search(r"k_(lasr|nemo)_[a-z_0-9]+?(?=I|P)", k).group(0) for k in usage if "k_lasr_" in k or "k_nemo_" in k}
    assert {"k_lasr_attn", "k_lasr_glu_dwconv", "k_lasr_gemm", "k_nemo_log_mel", "k_nemo_norm", "k_lasr_collapse"} <= names, names
    for k, v in usage.items():
        if "k_lasr_" in k or "k_nemo_" in k:
            assert v["scratch"] == 0, (k, v)
    attn = [v for k, v in usage.items() if "k_lasr_attn" in k]
    dw = [v for k, v in usage.items() if "k_lasr_glu_dwconv" in k]
    assert len(attn) == 1 and len(dw) == 2                                    # the SiLU and the ReLU instantiation
    assert attn[0]["vgprs"] <= 128 and attn[0]["lds"] <= 16384, attn
    assert all(v["vgprs"] <= 64 and v["lds"] == (64 + 63) * 64 * 4 for v in dw), dw
