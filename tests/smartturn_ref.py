"""CPU restatement of the reference Smart Turn model (Sources/MLXAudioVAD/Models/SmartTurn/SmartTurn.swift:29-272,
SmartTurnFeatures.swift:10-81), written from the Swift - the parity reference of csrc/smartturn.hip.

round="bf16": the engine's rounding points - the prepared samples and the features stay f32; the features are rounded when they enter the
first convolution, then bf16 after every primitive of the encoder (conv / Linear + bias, GELU, the positional add, LayerNorm, attention
output, residual add) with bf16 encoder weights; the pool and the classifier are f32 with f32 weights.  round=None: no rounding anywhere
(the distance between the two is the cost of running an f32 checkpoint in bf16).  acc=torch.float64: same graph and rounding points with
every contraction, statistic and softmax accumulated in float64 - the noise floor two exact realisations of one specification have
between them.  GELU is the exact erf form everywhere (MLX's gelu); the engine's encoder epilogue evaluates erf by a 1.5e-7 polynomial,
which this file does not mirror.

Weights are taken in the SANITIZED layout (conv weights [out, k, in], head layers pool_attention_0 / classifier_4 ...), as make_weights()
produces them; raw_checkpoint() gives the same weights the way a conversion script stores them."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import mel as omel

POOL_HID, CLS_MID = 256, 64


def make_weights(cfg, seed=0):
    """Random weights for a mas.SmartTurnConfig-like cfg, sanitized names and layouts, float32.  Head gains: the scores s_t get a
    spread of order 1 (a softmax that is neither flat nor one-hot); LayerNorm(256) renormalises whatever the pooled vector's size is,
    and the last two layers' gains bring the logit to an rms of order 1 (checked in test_smartturn_cpu.py)."""
    g = torch.Generator().manual_seed(seed)
    e = cfg.encoder_config
    d, f, nm = e.d_model, e.encoder_ffn_dim, e.num_mel_bins
    W = {}

    def u(shape, amp, plus=0.0):
        return (torch.rand(shape, generator=g) * 2 - 1) * amp + plus

    def lin(p, o, i, bias=True, gain=1.0):
        W[p + ".weight"] = u((o, i), gain * math.sqrt(3.0 / i))
        if bias:
            W[p + ".bias"] = u((o,), 0.05)

    def norm(p, n):
        W[p + ".weight"] = u((n,), 0.1, 1.0); W[p + ".bias"] = u((n,), 0.05)

    E = "encoder"
    W[E + ".conv1.weight"] = u((d, 3, nm), math.sqrt(3.0 / (3 * nm))); W[E + ".conv1.bias"] = u((d,), 0.05)
    W[E + ".conv2.weight"] = u((d, 3, d), math.sqrt(3.0 / (3 * d))); W[E + ".conv2.bias"] = u((d,), 0.05)
    W[E + ".embed_positions.weight"] = u((e.max_source_positions, d), 0.1)
    for i in range(e.encoder_layers):
        q = f"{E}.layers.{i}"
        norm(q + ".self_attn_layer_norm", d); norm(q + ".final_layer_norm", d)
        lin(q + ".self_attn.q_proj", d, d); lin(q + ".self_attn.k_proj", d, d, bias=e.k_proj_bias)
        lin(q + ".self_attn.v_proj", d, d); lin(q + ".self_attn.out_proj", d, d, gain=0.5)
        lin(q + ".fc1", f, d); lin(q + ".fc2", d, f, gain=0.5)
    norm(E + ".layer_norm", d)
    lin("pool_attention_0", POOL_HID, d); lin("pool_attention_2", 1, POOL_HID, gain=2.0)
    lin("classifier_0", POOL_HID, d); norm("classifier_1", POOL_HID)
    lin("classifier_4", CLS_MID, POOL_HID, gain=2.0); lin("classifier_6", 1, CLS_MID, gain=2.0)
    return W


def raw_checkpoint(W):
    """The same weights under the keys and layouts a converted checkpoint has before SmartTurnModel.sanitize (:274-324): "inner."
    prefix, Sequential indices in the head, torch conv layout [out, in, k], fc1 / fc2 / pool_attention_{0,2} stored transposed (pool_attention_0 only where d_model != 256: a square matrix cannot be told apart), one val_ tensor."""
    out = {}
    for k, v in W.items():
        rk = k
        for a, b in (("pool_attention_0.", "pool_attention.0."), ("pool_attention_2.", "pool_attention.2."), ("classifier_0.", "classifier.0."),
                     ("classifier_1.", "classifier.1."), ("classifier_4.", "classifier.4."), ("classifier_6.", "classifier.6.")):
            rk = rk.replace(a, b)
        if k in ("encoder.conv1.weight", "encoder.conv2.weight"):
            v = v.permute(0, 2, 1)
        if k.endswith("fc1.weight") or k.endswith("fc2.weight") or k == "pool_attention_2.weight" or (k == "pool_attention_0.weight" and v.shape[1] != 256):
            v = v.t()
        out["inner." + rk] = v.contiguous()
    out["val_loss"] = torch.zeros(1)
    return out


# ---------------------------------------------------------------------------------------------- front end (numpy float32)
def prepare(audio, pc, stats="f32seq"):
    """smartTurnPrepareAudioSamples (SmartTurnFeatures.swift:27-45) without the resampler: the last W samples or zeros in FRONT, then
    (x - mean) / max(std, 1e-7) over the whole window.  stats="f32seq": the reference's own sequential float32 sums;  "f64": the same
    statistics in float64 (the value both the reference and the engine approximate)."""
    a = np.asarray(audio, np.float32).reshape(-1)
    Wn = pc.max_audio_seconds * pc.sampling_rate
    if len(a) > Wn:
        a = a[len(a) - Wn:]
    elif len(a) < Wn:
        a = np.concatenate([np.zeros(Wn - len(a), np.float32), a])
    if not pc.normalize_audio:
        return a.copy()
    if stats == "f64":
        x = a.astype(np.float64)
        mean = x.mean()
        sd = max(math.sqrt(((x - mean) ** 2).mean()), 1e-7)
        return ((x - mean) / sd).astype(np.float32)
    n = np.float32(len(a))
    mean = np.float32(np.cumsum(a, dtype=np.float32)[-1] / n)                    # reduce(0, +): sequential, float32
    dv = (a - mean).astype(np.float32)
    var = np.float32(np.cumsum((dv * dv).astype(np.float32), dtype=np.float32)[-1] / n)
    sd = max(np.float32(np.sqrt(var)), np.float32(1e-7))
    return ((a - mean) / sd).astype(np.float32)


def features(prepared, pc, window="symmetric"):
    """smartTurnLogMelSpectrogram (:48-81) -> [frames, n_mels] float32: stft (DSP.swift:181-227: reflect pad n_fft / 2, symmetric Hann),
    last frame dropped, Slaney-scale Slaney-norm filters, log10 floor 1e-10, clamp to max - 8, (x + 4) / 4.  window="periodic" swaps in
    the periodic Hann of OpenAI's front end (the comparison with transformers' WhisperFeatureExtractor)."""
    f32 = np.float32
    a = np.asarray(prepared, f32)
    n_fft, hop = pc.n_fft, pc.hop_length
    n, pad = a.shape[0], n_fft // 2
    padded = np.concatenate([a[1:min(pad + 1, n)][::-1], a, a[max(0, n - pad - 1):max(1, n - 1)][::-1]])
    n_frames = 1 + (padded.shape[0] - n_fft) // hop
    idx = np.arange(n_frames)[:, None] * hop + np.arange(n_fft)[None, :]
    win = omel.hanning_window(n_fft) if window == "symmetric" else (f32(0.5) * (f32(1.0) - np.cos(f32(2.0) * f32(np.pi) * np.arange(n_fft, dtype=f32) / f32(n_fft)))).astype(f32)
    spec = np.fft.rfft((padded[idx] * win[None, :]).astype(f32), axis=1)
    mag = (np.abs(spec).astype(f32) ** 2).astype(f32)
    if mag.shape[0] > 1:
        mag = mag[:-1]
    mel = (mag @ omel.mel_filters(pc.sampling_rate, n_fft, pc.n_mels, norm="slaney", mel_scale="slaney")).astype(f32)
    mel = np.log10(np.maximum(mel, f32(1e-10))).astype(f32)
    mel = np.maximum(mel, mel.max() - f32(8.0))
    return ((mel + f32(4.0)) / f32(4.0)).astype(f32)


def input_features(audio, cfg, stats="f32seq"):
    """prepareInputFeatures (SmartTurn.swift:212-246) -> [F, n_mels] (the reference returns the transpose)."""
    pc = cfg.processor_config
    mel = features(prepare(audio, pc, stats), pc)
    target = pc.max_audio_seconds * pc.sampling_rate // pc.hop_length
    if mel.shape[0] > target:
        mel = mel[mel.shape[0] - target:]
    elif mel.shape[0] < target:
        mel = np.concatenate([np.zeros((target - mel.shape[0], mel.shape[1]), np.float32), mel])
    return mel


# ---------------------------------------------------------------------------------------------- model (torch)
class SmartTurnRef:
    def __init__(self, cfg, W, round="bf16", acc=torch.float32):
        self.cfg, self.round, self.acc = cfg, round, acc
        self.e = cfg.encoder_config
        self.w = {k: (v.float().bfloat16().float() if (round == "bf16" and k.startswith("encoder.")) else v.float()) for k, v in W.items()}

    def r(self, x):
        x = x.float()
        return x.bfloat16().float() if self.round == "bf16" else x

    def linear(self, x, p):
        y = x.to(self.acc) @ self.w[p + ".weight"].to(self.acc).t()
        if p + ".bias" in self.w:
            y = y + self.w[p + ".bias"].to(self.acc)
        return self.r(y)

    def ln(self, x, p, rnd=True):
        xa = x.to(self.acc)
        m = xa.mean(-1, keepdim=True)
        v = ((xa - m) ** 2).mean(-1, keepdim=True)
        y = (xa - m) / torch.sqrt(v + 1e-5) * self.w[p + ".weight"].to(self.acc) + self.w[p + ".bias"].to(self.acc)
        return self.r(y) if rnd else y

    def gelu(self, x, rnd=True):
        xa = x.to(self.acc)
        y = 0.5 * xa * (1.0 + torch.erf(xa / math.sqrt(2.0)))
        return self.r(y) if rnd else y

    def conv(self, x, p, stride):                                    # x [L, C_in]; weight [out, k, in]; k 3, pad 1
        w = self.w[p + ".weight"].permute(0, 2, 1).to(self.acc)
        y = F.conv1d(x.t()[None].to(self.acc), w, self.w[p + ".bias"].to(self.acc), stride=stride, padding=1)[0]
        return self.r(y.t())

    def attention(self, x, p):                                       # SmartTurnWhisperAttention (:50-68)
        T, H = x.shape[0], self.e.encoder_attention_heads
        hd = self.e.d_model // H
        q = self.linear(x, p + ".q_proj").reshape(T, H, hd).transpose(0, 1)
        k = self.linear(x, p + ".k_proj").reshape(T, H, hd).transpose(0, 1)
        v = self.linear(x, p + ".v_proj").reshape(T, H, hd).transpose(0, 1)
        s = (q.to(self.acc) @ k.to(self.acc).transpose(1, 2)) / math.sqrt(hd)
        o = self.r(torch.softmax(s, -1) @ v.to(self.acc))
        return self.linear(o.transpose(0, 1).reshape(T, H * hd), p + ".out_proj")

    def encode(self, feats):
        """feats [F, n_mels] -> [T, d] (SmartTurnWhisperEncoder, :135-149)"""
        x = self.r(torch.as_tensor(feats, dtype=torch.float32))
        x = self.gelu(self.conv(x, "encoder.conv1", 1))
        x = self.gelu(self.conv(x, "encoder.conv2", 2))
        x = self.r(x.to(self.acc) + self.w["encoder.embed_positions.weight"][: x.shape[0]].to(self.acc))
        for i in range(self.e.encoder_layers):
            q = f"encoder.layers.{i}"
            x = self.r(self.attention(self.ln(x, q + ".self_attn_layer_norm"), q + ".self_attn").to(self.acc) + x.to(self.acc))
            y = self.linear(self.gelu(self.linear(self.ln(x, q + ".final_layer_norm"), q + ".fc1")), q + ".fc2")
            x = self.r(y.to(self.acc) + x.to(self.acc))
        return self.ln(x, "encoder.layer_norm")

    def head(self, h):
        """h [T, d] -> (pooled [d], logit) (:187-196); f32 weights, nothing rounded to bf16"""
        w, A = self.w, self.acc
        ha = h.to(A)
        s = torch.tanh(ha @ w["pool_attention_0.weight"].to(A).t() + w["pool_attention_0.bias"].to(A))
        s = s @ w["pool_attention_2.weight"].to(A).t() + w["pool_attention_2.bias"].to(A)                 # [T, 1]
        a = torch.softmax(s, 0)
        pooled = (ha * a).sum(0)
        x = pooled @ w["classifier_0.weight"].to(A).t() + w["classifier_0.bias"].to(A)
        x = self.gelu(self.ln(x, "classifier_1", rnd=False), rnd=False)
        x = self.gelu(x @ w["classifier_4.weight"].to(A).t() + w["classifier_4.bias"].to(A), rnd=False)
        logit = x @ w["classifier_6.weight"].to(A).t() + w["classifier_6.bias"].to(A)
        return pooled.float(), float(logit.float()[0])

    def forward_features(self, feats):
        """-> dict(enc [T, d], pooled [d], logit)"""
        h = self.encode(feats)
        pooled, logit = self.head(h)
        return dict(enc=h, pooled=pooled, logit=logit)

    def forward(self, audio):
        return self.forward_features(input_features(audio, self.cfg))


# ---------------------------------------------------------------------------------------------- the cases both test files share
SHAPES = {                                                           # max_audio_seconds, d, heads, layers, ffn, k_proj_bias
    "S64": (2, 128, 2, 2, 256, False),                               # T = 100: not a multiple of 64, the attention's tail blocks run
    "S128": (3, 256, 2, 2, 512, True),                               # head size 128
    "PUB": (8, 384, 6, 4, 1536, False),                              # the published shape, T = 400
}
DECISION_SHAPE, DECISION_SEED = "S64", 12


def case_config(name):
    import mlx_audio_swift_amd as mas
    sec, d, H, L, f, kb = SHAPES[name]
    return mas.SmartTurnConfig(encoder_config=mas.SmartTurnEncoderConfig(max_source_positions=sec * 50, d_model=d, encoder_attention_heads=H,
                                                                        encoder_layers=L, encoder_ffn_dim=f, k_proj_bias=kb),
                               max_audio_seconds=sec)


def wave(n, seed):                                                   # _wave() of test_gpu_moonshine.py
    g = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return (0.15 * np.sin(2 * np.pi * (180 + 40 * seed) * t) + 0.1 * g.standard_normal(n)).astype(np.float32)


def intention():
    import os
    import wave as wavemod
    with wavemod.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "intention.wav"), "rb") as w:
        return np.frombuffer(w.readframes(w.getnframes()), "<i2").astype(np.float32) / 32768.0


def case_rows(cfg):
    """[W, W + 12345, W // 3, 1600, 37, W - 1] samples of wave(), one all-zero row of W // 2, and intention.wav cut to W."""
    Wn = cfg.window_samples
    rows = [wave(n, i) for i, n in enumerate([Wn, Wn + 12345, Wn // 3, 1600, 37, Wn - 1])]
    return rows + [np.zeros(Wn // 2, np.float32), intention()[:Wn]]


def threshold_logit(thr):
    return math.log(thr / (1.0 - thr))
