"""Reference of the LASR CTC model, written from LasrCTCModel.swift / LasrCTCConfig.swift, ParakeetAudio.swift:6-62, DSP.swift
(hanningWindow, stft .constant, melFilters slaney / slaney) and Wav2Vec2CTC.swift:520-542.  numpy only, one row at a time (the engine's
ragged-batch rule is that a row gives what its own batch-1 call gives).

Realisations: `Ref(cfg, W, round=False, acc=np.float64)` is the model as written; `acc=np.float32` the same in float32 arithmetic;
`round=True` puts the device's bf16 rounding points in (weights rounded once, every kernel output rounded once, see csrc/lasr.hip),
with `acc` the precision of the sums in between - float32 as the device accumulates, float64 to measure what the summation order is
worth."""
import numpy as np

DECISION_SEED = 20251
SR, HOP, NFFT, WIN = 16000, 160, 512, 400

_CASES = {
    "A": dict(vocab_size=64, pad_token_id=0, encoder_config=dict(
        hidden_size=128, num_attention_heads=2, num_key_value_heads=2, intermediate_size=256, num_hidden_layers=2, num_mel_bins=40,
        subsampling_conv_channels=96, subsampling_conv_kernel_size=5, subsampling_conv_stride=2, conv_kernel_size=32, hidden_act="silu",
        attention_bias=False, convolution_bias=False)),
    "B": dict(vocab_size=101, pad_token_id=3, encoder_config=dict(
        hidden_size=192, num_attention_heads=3, num_key_value_heads=1, intermediate_size=384, num_hidden_layers=1, num_mel_bins=80,
        subsampling_conv_channels=64, subsampling_conv_kernel_size=3, subsampling_conv_stride=2, conv_kernel_size=5, hidden_act="relu",
        attention_bias=True, convolution_bias=True, feed_forward_residual_weights=[1.25, 0.75], conv_residual_weights=[1.0, 2.0])),
    "P": dict(vocab_size=512, pad_token_id=0, encoder_config=dict(
        hidden_size=512, num_attention_heads=8, num_key_value_heads=8, intermediate_size=2048, num_hidden_layers=2, num_mel_bins=128,
        subsampling_conv_channels=256, subsampling_conv_kernel_size=5, subsampling_conv_stride=2, conv_kernel_size=32)),
    # head size 64 at the smallest width, for the comparison with transformers
    "H": dict(vocab_size=32, pad_token_id=0, encoder_config=dict(
        hidden_size=64, num_attention_heads=1, num_key_value_heads=1, intermediate_size=96, num_hidden_layers=2, num_mel_bins=24,
        subsampling_conv_channels=32, subsampling_conv_kernel_size=3, subsampling_conv_stride=2, conv_kernel_size=4)),
}
_ENC_DEFAULTS = dict(hidden_act="silu", attention_bias=False, convolution_bias=False, layer_norm_eps=1e-6, rope_theta=10000.0,
                     conv_residual_weights=[2.0, 1.0], feed_forward_residual_weights=[1.5, 0.5])


def case_config(name: str) -> dict:
    """The JSON of test shape `name` (A, B, P of the GPU tests; H), every field the reference reads spelled out."""
    c = _CASES[name]
    return dict(vocab_size=c["vocab_size"], pad_token_id=c["pad_token_id"], encoder_config={**_ENC_DEFAULTS, **c["encoder_config"]})


def make_weights(cfg: dict, seed: int, blank_bias: float = 0.0) -> dict:
    """float32 weights under the names LasrCTCModel.sanitize leaves (conv weights [out, k, in]).  The logit scale: a ctc_head gain of 4 (logit
    std about 4) and a bias that leaves three tokens in competition, so that the per-frame top-2 margin is large against bf16 noise:
    test_lasr_cpu asserts it."""
    e, r = cfg["encoder_config"], np.random.default_rng(seed)
    d, f, cc, ks, ck, mels = (e["hidden_size"], e["intermediate_size"], e["subsampling_conv_channels"], e["subsampling_conv_kernel_size"],
                              e["conv_kernel_size"], e["num_mel_bins"])
    hk = e["num_key_value_heads"] * 64
    W = {}

    def u(shape, amp, plus=0.0):
        return (plus + r.uniform(-amp, amp, shape)).astype(np.float32)

    def lin(p, o, i, bias, gain=1.0):
        W[p + ".weight"] = u((o, i), gain * np.sqrt(3.0 / i))
        if bias:
            W[p + ".bias"] = u((o,), 0.05)

    def norm(p):
        W[p + ".weight"], W[p + ".bias"] = u((d,), 0.1, 1.0), u((d,), 0.05)

    S = "encoder.subsampler."
    lin(S + "dense_0", d, mels, True)
    W[S + "conv_0.weight"], W[S + "conv_0.bias"] = u((d, ks, d), np.sqrt(3.0 / (ks * d))), u((d,), 0.05)
    W[S + "conv_1.weight"], W[S + "conv_1.bias"] = u((cc, ks, d), np.sqrt(3.0 / (ks * d))), u((cc,), 0.05)
    lin(S + "dense_1", d, cc, True)
    ab, cb = e["attention_bias"], e["convolution_bias"]
    for i in range(e["num_hidden_layers"]):
        q = f"encoder.layers.{i}."
        for n in ("norm_feed_forward1", "norm_self_att", "norm_conv", "norm_feed_forward2", "norm_out"):
            norm(q + n)
        for n in ("feed_forward1", "feed_forward2"):
            lin(q + n + ".linear1", f, d, ab)
            lin(q + n + ".linear2", d, f, ab, 0.5)
        lin(q + "self_attn.q_proj", d, d, ab)
        lin(q + "self_attn.k_proj", hk, d, ab)
        lin(q + "self_attn.v_proj", hk, d, ab)
        lin(q + "self_attn.o_proj", d, d, ab, 0.5)
        W[q + "conv.pointwise_conv1.weight"] = u((2 * d, 1, d), np.sqrt(3.0 / d))
        W[q + "conv.pointwise_conv2.weight"] = u((d, 1, d), 0.5 * np.sqrt(3.0 / d))
        W[q + "conv.depthwise_conv.weight"] = u((d, ck, 1), np.sqrt(3.0 / ck))
        if cb:
            W[q + "conv.pointwise_conv1.bias"], W[q + "conv.pointwise_conv2.bias"] = u((2 * d,), 0.05), u((d,), 0.05)
            W[q + "conv.depthwise_conv.bias"] = u((d,), 0.05)
        W[q + "conv.norm.weight"], W[q + "conv.norm.bias"] = u((d,), 0.1, 1.0), u((d,), 0.05)
        W[q + "conv.norm.running_mean"], W[q + "conv.norm.running_var"] = u((d,), 0.05), u((d,), 0.1, 1.0)
    norm("encoder.out_norm")
    lin("ctc_head", cfg["vocab_size"], d, True, 4.0)
    # three tokens compete (the blank and two others, bias 0), the rest sit 40 below: the top-2 gap of three values has a quarter of
    # the density at zero that the gap of a whole vocabulary has, so fewer frames lie within rounding noise of a tie
    live = [cfg["pad_token_id"], 5, 9]
    W["ctc_head.bias"] = np.where(np.isin(np.arange(cfg["vocab_size"]), live), W["ctc_head.bias"], np.float32(-40.0)).astype(np.float32)
    W["ctc_head.bias"][cfg["pad_token_id"]] += np.float32(blank_bias)
    return W


# ---------------------------------------------------------------------------------------------- arithmetic helpers
def bf16(x):
    """Round to bfloat16 (nearest even), as float32."""
    a = np.ascontiguousarray(x, dtype=np.float32)
    u = a.view(np.uint32)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32)


def frames_of(n: int) -> int:
    return 1 + n // HOP


def conv_out(t: int, k: int, s: int) -> int:
    return (t - k) // s + 1 if t >= k else 0


def t2_of(cfg: dict, n: int) -> int:
    e = cfg["encoder_config"]
    k, s = e["subsampling_conv_kernel_size"], e["subsampling_conv_stride"]
    return conv_out(conv_out(frames_of(n), k, s), k, s)


def slaney_filters(mels: int, dtype=np.float64):
    """melFilters(sampleRate 16000, nFft 512, norm slaney, melScale .slaney) (DSP.swift:76-160) -> [257, mels]."""
    fsp, logstep = 200.0 / 3.0, np.log(6.4) / 27.0

    def hz2mel(f):
        return f / fsp if f < 1000.0 else 15.0 + np.log(f / 1000.0) / logstep

    def mel2hz(m):
        return fsp * m if m < 15.0 else 1000.0 * np.exp(logstep * (m - 15.0))

    mmax = hz2mel(8000.0)
    fp = [mel2hz(i * mmax / (mels + 1)) for i in range(mels + 2)]
    fr = np.arange(257) * (SR / NFFT)
    fb = np.zeros((257, mels))
    for j in range(mels):
        lo, ce, hi = fp[j], fp[j + 1], fp[j + 2]
        up, down = (fr >= lo) & (fr < ce), (fr >= ce) & (fr <= hi)
        fb[up, j] = (fr[up] - lo) / (ce - lo)
        fb[down, j] = (hi - fr[down]) / (hi - ce)
        fb[:, j] *= 2.0 / (hi - lo)
    return fb.astype(dtype)


def front_end(x, mels: int, dtype=np.float64):
    """ParakeetAudio.logMelSpectrogram with LasrCTCModel.prepareFeatures' configuration -> [F, mels] in `dtype` arithmetic."""
    x = np.asarray(x, dtype)
    if len(x) > 1:
        x = np.concatenate([x[:1], x[1:] - dtype(0.97) * x[:-1]])
    win = np.zeros(NFFT, dtype)
    win[56:456] = (0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(WIN) / (WIN - 1)))).astype(dtype)
    p = np.concatenate([np.zeros(256, dtype), x, np.zeros(256, dtype)])
    F = 1 + (len(p) - NFFT) // HOP
    fr = np.stack([p[t * HOP: t * HOP + NFFT] for t in range(F)]) * win
    spec = np.fft.rfft(fr.astype(np.float64), axis=1) if dtype == np.float64 else np.fft.rfft(fr, axis=1).astype(np.complex64)
    power = (spec.real.astype(dtype) ** 2 + spec.imag.astype(dtype) ** 2).astype(dtype)
    mel = np.log(power @ slaney_filters(mels, dtype) + dtype(2.0 ** -24)).astype(dtype)
    mean = mel.mean(axis=0, keepdims=True, dtype=dtype)
    var = ((mel - mean) ** 2).sum(axis=0, keepdims=True, dtype=dtype) / dtype(max(F - 1, 1))
    return ((mel - mean) / (np.sqrt(var) + dtype(1e-5))).astype(dtype)


def greedy_ctc(logits, blank: int) -> list:
    """greedyCTCTokens (Wav2Vec2CTC.swift:520-542) of one row's logits [T, V]."""
    prev, out = -1, []
    for tok in np.argmax(logits, axis=-1):
        tok = int(tok)
        if tok != prev and tok != blank:
            out.append(tok)
        prev = tok
    return out


class Ref:
    def __init__(self, cfg: dict, W: dict, round: bool = False, acc=np.float64):
        self.cfg, self.e, self.round, self.acc = cfg, cfg["encoder_config"], round, acc
        self.W = {k: np.asarray(v, np.float32) for k, v in W.items()}

    # T(): the device's rounding point; w(): a weight as the engine stores it
    def T(self, x):
        return bf16(x).astype(self.acc) if self.round else np.asarray(x, self.acc)

    def w(self, name):
        v = self.W[name]
        return (bf16(v) if self.round else v).astype(self.acc)

    def lin(self, x, p, bias=True):
        y = x.astype(self.acc) @ self.w(p + ".weight").reshape(self.W[p + ".weight"].shape[0], -1).T
        if bias and p + ".bias" in self.W:
            y = y + self.w(p + ".bias")
        return y

    def act(self, x):
        return np.maximum(x, 0) if self.e["hidden_act"] == "relu" else x / (1.0 + np.exp(-x))

    def ln(self, x, p):
        m = x.mean(axis=-1, keepdims=True)
        v = ((x - m) ** 2).mean(axis=-1, keepdims=True)
        b = self.w(p + ".bias") if p + ".bias" in self.W else 0.0
        return self.T((x - m) / np.sqrt(v + self.acc(self.e["layer_norm_eps"])) * self.w(p + ".weight") + b)

    def conv_stem(self, x, p, k, s):
        T = conv_out(x.shape[0], k, s)
        cols = np.stack([x[t * s: t * s + k].reshape(-1) for t in range(T)])
        return self.T(np.maximum(self.T(self.lin(cols, p)), 0))

    def stem(self, feats):
        k, s = self.e["subsampling_conv_kernel_size"], self.e["subsampling_conv_stride"]
        S = "encoder.subsampler."
        x = self.T(feats)                                                       # the front end's single rounding
        h = self.T(np.maximum(self.T(self.lin(x, S + "dense_0")), 0))
        h = self.conv_stem(h, S + "conv_0", k, s)
        h = self.conv_stem(h, S + "conv_1", k, s)
        return self.T(self.lin(h, S + "dense_1"))

    def ffn(self, x, p):
        h = self.T(self.act(self.T(self.lin(x, p + ".linear1"))))
        return self.T(self.lin(h, p + ".linear2"))

    def rope(self, x):
        """x [T, H, 64]; f32 tables as the engine builds them"""
        T = x.shape[0]
        inv = (np.float32(1.0) / np.power(np.float32(self.e["rope_theta"]), np.arange(0, 64, 2, dtype=np.float32) / np.float32(64))).astype(np.float32)
        ang = (np.arange(T, dtype=np.float32)[:, None] * inv[None]).astype(np.float32)
        cos, sin = np.cos(ang.astype(np.float64)).astype(np.float32), np.sin(ang.astype(np.float64)).astype(np.float32)
        if not self.round and self.acc == np.float64:
            inv64 = 1.0 / np.power(float(self.e["rope_theta"]), np.arange(0, 64, 2) / 64.0)
            cos, sin = np.cos(np.arange(T)[:, None] * inv64), np.sin(np.arange(T)[:, None] * inv64)
        cos, sin = np.concatenate([cos, cos], -1)[:, None].astype(self.acc), np.concatenate([sin, sin], -1)[:, None].astype(self.acc)
        rot = np.concatenate([-x[..., 32:], x[..., :32]], -1)
        return self.T(x * cos + rot * sin)

    def attn(self, x, p):
        H, Hk = self.e["num_attention_heads"], self.e["num_key_value_heads"]
        T = x.shape[0]
        q = self.rope(self.T(self.lin(x, p + ".q_proj")).reshape(T, H, 64))
        k = self.rope(self.T(self.lin(x, p + ".k_proj")).reshape(T, Hk, 64))
        v = self.T(self.lin(x, p + ".v_proj")).reshape(T, Hk, 64)
        k, v = np.repeat(k, H // Hk, axis=1), np.repeat(v, H // Hk, axis=1)
        s = np.einsum("thd,shd->hts", q, k) * self.acc(0.125)
        s = np.exp(s - s.max(axis=-1, keepdims=True))
        o = np.einsum("hts,shd->thd", s / s.sum(axis=-1, keepdims=True), v)
        return self.T(self.lin(self.T(o).reshape(T, H * 64), p + ".o_proj"))

    def conv_module(self, x, p):
        d, k = self.e["hidden_size"], self.e["conv_kernel_size"]
        h = self.T(self.lin(x, p + ".pointwise_conv1", self.e["convolution_bias"]))
        g = self.T(h[:, :d] / (1.0 + np.exp(-h[:, d:])))
        padl = (k - 1) // 2
        g = np.concatenate([np.zeros((padl, d), self.acc), g, np.zeros((k - 1 - padl, d), self.acc)])
        # inference BatchNorm (eps 1e-5) folded into the taps and a shift in f32, as the engine does at finalize
        f32 = np.float32
        scale = (self.W[p + ".norm.weight"] / np.sqrt(self.W[p + ".norm.running_var"] + f32(1e-5))).astype(f32)
        taps = (self.W[p + ".depthwise_conv.weight"][:, :, 0] * scale[:, None]).astype(f32)
        dwb = self.W.get(p + ".depthwise_conv.bias", np.zeros(d, f32)) if self.e["convolution_bias"] else np.zeros(d, f32)
        shift = ((dwb - self.W[p + ".norm.running_mean"]) * scale + self.W[p + ".norm.bias"]).astype(f32)
        T = x.shape[0]
        y = np.stack([(g[t: t + k] * taps.T.astype(self.acc)).sum(axis=0) for t in range(T)]) + shift.astype(self.acc)
        y = self.T(self.act(y))
        return self.T(self.lin(y, p + ".pointwise_conv2", self.e["convolution_bias"]))

    def block(self, x, i):
        q = f"encoder.layers.{i}."
        fa, fb = (self.acc(v) for v in self.e["feed_forward_residual_weights"])
        ca, cb = (self.acc(v) for v in self.e["conv_residual_weights"])
        h = self.T(fa * x + fb * self.ffn(self.ln(x, q + "norm_feed_forward1"), q + "feed_forward1"))
        h = self.T(h + self.attn(self.ln(h, q + "norm_self_att"), q + "self_attn"))
        h = self.T(ca * h + cb * self.conv_module(self.ln(h, q + "norm_conv"), q + "conv"))
        h = self.T(fa * h + fb * self.ffn(self.ln(h, q + "norm_feed_forward2"), q + "feed_forward2"))
        return self.ln(h, q + "norm_out")

    def forward(self, feats, start=None):
        """feats [F, mels] -> dict(stem, blocks [L], out_norm, logits).  start = (stage, tensor): resume behind tap `stage` (0 the stem,
        i the i-th block) from the given tensor, so that each stage can be held on the device's own previous stage."""
        out = {"blocks": []}
        L = self.e["num_hidden_layers"]
        if start is None:
            h = out["stem"] = self.stem(np.asarray(feats, self.acc))
            first = 0
        else:
            first, h = start[0], self.T(np.asarray(start[1], self.acc))
        for i in range(first, L):
            h = self.block(h, i)
            out["blocks"].append(h)
        out["out_norm"] = self.ln(h, "encoder.out_norm")
        out["logits"] = self.lin(out["out_norm"], "ctc_head")
        return out
