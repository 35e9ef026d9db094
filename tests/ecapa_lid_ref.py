"""CPU restatement of the reference language-identification model (Sources/MLXAudioLID/Models/EcapaTdnn/EcapaTdnnLID.swift:13-195,
EcapaTdnnLayers.swift:52-78, EcapaMelSpectrogram.swift:15-55 on MLXAudioCore/DSP.swift:25-227, and the shared backbone
MLXAudioCodecs/EcapaTdnn/EcapaTdnnBackbone.swift:16-282 with reflectPadding false and globalContext true), written from the Swift - the
parity reference of csrc/ecapa_lid.hip.  One row at a time, [T, C] tensors, float32 or float64; test_ecapa_lid_cpu.py holds it to
independent realisations (numpy / scipy for the front end, torch.nn for the layers)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import mlx_audio_swift_amd as mas

N_FFT, HOP, SAMPLE_RATE = 400, 160, 16000
BN_EPS = 1e-5

# name -> n_mels, channels, attention, se, embedding, hidden, classes
CASES = {
    "S64": (60, 64, 16, 16, 32, 64, 10),           # the reference tests' small config: Res2Net chunk width 8, below an MFMA tile
    "S128": (60, 128, 32, 32, 48, 96, 107),        # odd class count, chunk width 16
    "PUB": (60, 1024, 128, 128, 256, 512, 107),    # the published shape
}
# T = 1, T = 2, and lengths around which the halo of 7 x 4 frames, the masks and the reductions can go wrong; the last row is all zeros
CASE_LENS = (159, 160, 1637, 4000, 7999, 12800, 16000, 4000)
# chosen on the CPU (test_ecapa_lid_cpu.py::test_decision_seed_separates_the_case_rows): in the float32 reference of S128 every case row
# has a top-1 / top-2 log-prob margin >= 1e-2 and no exact tie within its top 5
DECISION_SEED = 11


def case_config(name, max_batch=8, max_samples=16000):
    nm, c, a, se, e, h, n = CASES[name]
    labels = {str(i): f"l{i:03d}: Language {i}" for i in range(n)}
    return mas.EcapaTdnnConfig(n_mels=nm, channels=c, attention_channels=a, se_channels=se, embedding_dim=e, classifier_hidden_dim=h,
                               num_classes=n, id2label=labels, max_batch=max_batch, max_samples=max_samples)


def case_rows(seed=5, lens=CASE_LENS):
    """Noise under a slow envelope plus a tone; the first half of the 7999 row lies 100 dB down (the top_db floor binds there); the last
    row is silence."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for i, n in enumerate(lens):
        t = torch.arange(n, dtype=torch.float64)
        x = 0.1 * torch.randn(n, generator=g, dtype=torch.float64) * (1.0 + 0.5 * torch.sin(2 * math.pi * t / 3000.0 + i))
        x = x + 0.05 * torch.sin(2 * math.pi * (200.0 + 150.0 * i) * t / SAMPLE_RATE)
        if n == 7999:
            x[: n // 2] *= 1e-5
        rows.append(x.to(torch.float32).numpy())
    rows[-1] = np.zeros(lens[-1], np.float32)
    return rows


def frames_of(n_samples):
    return n_samples // HOP + 1


def make_weights(cfg, seed):
    """Random weights under the sanitized names, float32.  BatchNorm running statistics lie away from (0, 1) and the affine terms are
    not trivial; the classifier's gains bring the logits to a spread of order 1."""
    g = torch.Generator().manual_seed(seed)
    W = {}

    def uni(shape, amp, plus=0.0):
        return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * amp + plus).to(torch.float32)

    for name, shape in mas.ecapa_lid_expected_shapes(cfg).items():
        if name.endswith("running_var"):
            W[name] = uni(shape, 0.5, 1.0)
        elif name.endswith("running_mean"):
            W[name] = uni(shape, 0.3)
        elif ".norm." in name or "asp_bn" in name:
            W[name] = uni(shape, 0.3, 1.0) if name.endswith("weight") else uni(shape, 0.2)
        elif name.endswith("bias"):
            W[name] = uni(shape, 0.1)
        else:
            fan_in = int(np.prod(shape[1:]))
            gain = 3.0 if name.startswith("classifier.out") else 1.5 if "asp.conv" in name else 1.0
            W[name] = uni(shape, gain * math.sqrt(3.0 / fan_in))
    return W


def raw_checkpoint(W):
    """The same weights under the keys of a converted SpeechBrain checkpoint, before EcapaTdnn.sanitize (:99-131), with the
    num_batches_tracked counters a BatchNorm carries."""
    out = {}
    for k, v in W.items():
        r = k
        if ".se_block.conv" in r or ".fc." in r:
            r = r.replace(".weight", ".conv.weight").replace(".bias", ".conv.bias")
        elif ".asp_bn." in r:
            r = r.replace(".asp_bn.", ".asp_bn.norm.")
        elif r.startswith("embedding_model."):
            r = r.replace(".conv.", ".conv.conv.").replace(".norm.", ".norm.norm.")
        for i in range(4):
            r = r.replace(f"embedding_model.block{i}.", f"embedding_model.blocks.{i}.")
        out[r] = v
        if r.endswith("running_var"):
            out[r[: -len("running_var")] + "num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
    return out


# ---------------------------------------------------------------------------------------------------- front end
def hamming_window(dtype):
    """hammingWindow(size: 400, periodic: true) (DSP.swift:25-42)"""
    n = torch.arange(N_FFT, dtype=torch.float64)
    return (0.54 - 0.46 * torch.cos(2.0 * math.pi * n / N_FFT)).to(dtype)


def mel_filters(n_mels, dtype):
    """melFilters(sampleRate: 16000, nFft: 400, norm: nil, melScale: .htk) (DSP.swift:76-168) -> [201, n_mels]"""
    freqs = torch.arange(N_FFT // 2 + 1, dtype=torch.float64) * SAMPLE_RATE / N_FFT
    m_max = 2595.0 * math.log10(1.0 + (SAMPLE_RATE / 2.0) / 700.0)
    pts = 700.0 * (10.0 ** (torch.arange(n_mels + 2, dtype=torch.float64) * m_max / (n_mels + 1) / 2595.0) - 1.0)
    lo, ce, hi = pts[:-2][None], pts[1:-1][None], pts[2:][None]
    f = freqs[:, None]
    up, down = (f - lo) / (ce - lo), (hi - f) / (hi - ce)
    fb = torch.where((f >= lo) & (f < ce), up, torch.where((f >= ce) & (f <= hi), down, torch.zeros_like(up)))
    return fb.to(dtype)


def mel_db(wave, n_mels=60, dtype=torch.float32):
    """EcapaMelSpectrogram.compute (:35-54) -> [T, n_mels]: 200 zeros on each side, periodic Hamming, power, HTK filters,
    10 log10 max(., 1e-10), floor at the maximum - 80."""
    x = torch.as_tensor(wave).to(dtype)
    x = F.pad(x, (N_FFT // 2, N_FFT // 2))
    fr = x.unfold(0, N_FFT, HOP) * hamming_window(dtype)
    power = torch.fft.rfft(fr, dim=1).abs().square()
    db = 10.0 * torch.log10(torch.clamp(power @ mel_filters(n_mels, dtype), min=1e-10))
    return torch.maximum(db, db.max() - 80.0)


def sentence_mean_normalize(mel):
    """EcapaTdnnLID.swift:84-86"""
    return mel - mel.mean(dim=0, keepdim=True)


# ---------------------------------------------------------------------------------------------------- model
class EcapaLidRef:
    """stages(features) -> {2: block0, 3..5: SE-Res2Net blocks, 6: mfa, 7: pooled, 8: embedding, 9: log-probs}, one row [T, n_mels]."""

    def __init__(self, cfg, W, dtype=torch.float32):
        self.cfg, self.dtype = cfg, dtype
        self.W = {k: v.to(dtype) for k, v in W.items()}

    def bn(self, x, p):                                               # MLXNN.BatchNorm in eval mode, channels last
        W = self.W
        return (x - W[p + ".running_mean"]) / torch.sqrt(W[p + ".running_var"] + BN_EPS) * W[p + ".weight"] + W[p + ".bias"]

    def conv(self, x, p, dilation=1):                                 # MLXNN.Conv1d on [T, Cin], weight [out, k, in], zero "same" padding
        w = self.W[p + ".weight"]
        pad = (w.shape[1] - 1) * dilation // 2
        y = F.conv1d(x.t()[None], w.permute(0, 2, 1), self.W[p + ".bias"], padding=pad, dilation=dilation)
        return y[0].t()

    def tdnn(self, x, p, dilation=1):                                 # TDNNBlock (Backbone.swift:137-140)
        return self.bn(torch.relu(self.conv(x, p + ".conv", dilation)), p + ".norm")

    def res2net(self, x, p, dilation):                                # :167-175
        chunks = torch.chunk(x, self.cfg.res2net_scale, dim=-1)
        outs = [chunks[0]]
        for i in range(self.cfg.res2net_scale - 1):
            inp = chunks[i + 1] + outs[-1] if i > 0 else chunks[i + 1]
            outs.append(self.tdnn(inp, f"{p}.blocks.{i}", dilation))
        return torch.cat(outs, dim=-1)

    def se(self, x, p):                                               # :187-192
        s = x.mean(dim=0, keepdim=True)
        s = torch.relu(self.conv(s, p + ".conv1"))
        return x * torch.sigmoid(self.conv(s, p + ".conv2"))

    def se_res2net(self, x, p, dilation):                             # :231-238
        out = self.tdnn(x, p + ".tdnn1")
        out = self.res2net(out, p + ".res2net_block", dilation)
        out = self.tdnn(out, p + ".tdnn2")
        return self.se(out, p + ".se_block") + x

    def asp(self, x, p):                                              # :257-281, globalContext
        m = x.mean(dim=0, keepdim=True)
        sd = torch.sqrt(x.var(dim=0, unbiased=False, keepdim=True) + 1e-9)
        a = torch.cat([x, m.expand_as(x), sd.expand_as(x)], dim=-1)
        a = torch.softmax(self.conv(torch.tanh(self.tdnn(a, p + ".tdnn")), p + ".conv"), dim=0)
        mean = (a * x).sum(dim=0)
        var = (a * (x * x)).sum(dim=0) - mean * mean
        return torch.cat([mean, torch.sqrt(torch.clamp(var, min=1e-9))])

    def stages(self, feat):
        c, e = self.cfg, "embedding_model."
        x = torch.as_tensor(feat).to(self.dtype)
        out = {2: self.tdnn(x, e + "block0")}                         # (block0 and mfa run at dilation 1, :29-34, 59-64)
        h = out[2]
        for i in (1, 2, 3):
            h = self.se_res2net(h, f"{e}block{i}", c.dilations[i])
            out[2 + i] = h
        out[6] = self.tdnn(torch.cat([out[3], out[4], out[5]], dim=-1), e + "mfa")
        out[7] = self.asp(out[6], e + "asp")
        out[8] = self.conv(self.bn(out[7][None], e + "asp_bn"), e + "fc")[0]
        z = self.bn(F.leaky_relu(out[8], 0.01), "classifier.norm")    # EcapaClassifier (EcapaTdnnLayers.swift:63-77)
        W = self.W
        z = F.linear(z, W["classifier.DNN.block_0.linear.w.weight"], W["classifier.DNN.block_0.linear.w.bias"])
        z = self.bn(F.leaky_relu(z, 0.01), "classifier.DNN.block_0.norm")
        z = F.linear(z, W["classifier.out.w.weight"], W["classifier.out.w.bias"])
        out[9] = torch.log_softmax(z, dim=-1)
        return out

    def log_probs(self, wave):
        """callAsFunction on compute(audio:) (:42-46, 57-58)"""
        return self.stages(sentence_mean_normalize(mel_db(wave, self.cfg.n_mels, self.dtype)))[9]


def top_k(log_probs, k):
    """predict's ranking (:59-73): descending probability; (indices, probabilities) of the first min(k, classes)"""
    p = torch.exp(torch.as_tensor(log_probs))
    order = torch.argsort(p, descending=True, stable=True)[: min(k, p.numel())]
    return order.numpy(), p[order].numpy()
