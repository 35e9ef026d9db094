"""A numpy specification of SenseVoice (SenseVoiceModel.swift, SenseVoiceAudio.swift, DSP.swift melFilters / hammingWindow /
hanningWindow), stage by stage: front end, LFR / CMVN, intake, a layer, the encoder, head, log-softmax, greedy CTC, rich info.  Every
function takes acc = np.float64 or np.float32: the arithmetic runs in that type.  test_sensevoice_cpu.py holds it to torch.nn and
numpy / scipy; test_gpu_sensevoice.py holds the device to it."""
import numpy as np
import scipy.fft

import mlx_audio_swift_amd as mas

DECISION_SEED = 11
LN_EPS = 1e-5

CASES = {
    #      output heads linear blocks tp kernel shift vocab mels lfr_m lfr_n window
    "A": (64, 2, 128, 3, 2, 5, 0, 32, 80, 7, 6, "hamming"),
    "B": (48, 3, 80, 2, 1, 11, 2, 300, 40, 5, 3, "hann"),
    "F": (8, 2, 16, 1, 0, 5, 0, 6, 80, 7, 6, "hamming"),
    "P": (512, 4, 2048, 2, 1, 11, 0, 25055, 80, 7, 6, "hamming"),
}


def case_config(name, **workspace):
    D, H, Fd, nb, tp, k, sh, V, nm, m, n, win = CASES[name]
    ws = dict(max_batch=8, max_seconds=4, head_rows=2048)
    ws.update(workspace)
    return mas.SenseVoiceConfig(vocab_size=V, input_size=nm * m,
                                encoder_conf=mas.SenseVoiceEncoderConfig(output_size=D, attention_heads=H, linear_units=Fd, num_blocks=nb,
                                                                         tp_blocks=tp, kernel_size=k, sanm_shift=sh),
                                frontend_conf=mas.SenseVoiceFrontendConfig(window=win, n_mels=nm, lfr_m=m, lfr_n=n), **ws)


def make_weights(cfg, seed, head_gain=4.0, blank_bias=0.0):
    """Sanitized float32 weights.  Scales: unit-variance activations through the layers (Linear ~ U(+-sqrt(3 / in))), LayerNorm weights
    near 1, and a head of gain `head_gain` so that the top-2 margin of a frame is far above the float32 error (the decision seeds)."""
    g = np.random.default_rng(seed)
    W = {}
    for k, shape in mas.sensevoice_expected_shapes(cfg).items():
        if k.endswith("norm1.weight") or k.endswith("norm2.weight") or k.endswith("_norm.weight"):
            v = 1.0 + 0.1 * g.uniform(-1, 1, shape)
        elif k.endswith(".bias"):
            v = 0.05 * g.uniform(-1, 1, shape)
        elif k.endswith("fsmn_block.weight"):
            v = 0.5 * np.sqrt(3.0 / shape[1]) * g.uniform(-1, 1, shape)
        elif k == "embed.weight":
            v = 0.5 * g.uniform(-1, 1, shape)
        else:
            gain = head_gain if k == "ctc_lo.weight" else (0.5 if ("linear_out" in k or "w_2" in k) else 1.0)
            v = gain * np.sqrt(3.0 / shape[1]) * g.uniform(-1, 1, shape)
        W[k] = v.astype(np.float32)
    if blank_bias:
        W["ctc_lo.bias"][0] += np.float32(blank_bias)
    return W


def make_cmvn(cfg, seed):
    g = np.random.default_rng(seed + 1000)
    return ((-8.0 + g.uniform(-1, 1, cfg.input_size)).astype(np.float32), (0.2 + 0.05 * g.uniform(-1, 1, cfg.input_size)).astype(np.float32))


def tone_row(seed, n, amp=0.3):
    """n samples of a few drifting tones plus noise, peak below 1."""
    if n == 0:
        return np.zeros(0, np.float32)
    g = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    x = np.zeros(n)
    for _ in range(4):
        f0, f1 = g.uniform(100, 3500, 2)
        x += g.uniform(0.2, 1.0) * np.sin(2 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / max(t[-1], 1e-3)) + g.uniform(0, 6.28))
    x = x / max(np.abs(x).max(), 1e-9) * amp + 0.01 * g.standard_normal(n)
    return x.astype(np.float32)


def frames_of(n, win=400, hop=160):
    return 0 if n < win else 1 + (n - win) // hop


def rows_of(F, lfr_n=6):
    return 4 + -(-F // lfr_n)


def samples_for_frames(F, win=400, hop=160):
    return 0 if F <= 0 else win + (F - 1) * hop


# ---------------------------------------------------------------------------------------------- front end
def window(name, n, acc):
    i = np.arange(n, dtype=acc)
    c = np.cos(acc(2) * acc(np.pi) * i / acc(n - 1))
    return (acc(0.5) * (acc(1) - c) if "hann" in name.lower() else acc(0.54) - acc(0.46) * c).astype(acc)


def mel_filters(sample_rate, n_fft, n_mels, acc, f_min=20.0):
    """DSP.melFilters(htk, norm nil): triangles in Hz between the mel-spaced points, [n_fft / 2 + 1, n_mels]."""
    hz2mel = lambda f: acc(2595) * np.log10(acc(1) + f / acc(700))
    mel2hz = lambda m: acc(700) * (np.power(acc(10), m / acc(2595)) - acc(1))
    freqs = np.arange(n_fft // 2 + 1, dtype=acc) * acc(sample_rate) / acc(n_fft)
    m0, m1 = hz2mel(acc(f_min)), hz2mel(acc(sample_rate) / acc(2))
    pts = mel2hz(m0 + np.arange(n_mels + 2, dtype=acc) * (m1 - m0) / acc(n_mels + 1)).astype(acc)
    fb = np.zeros((len(freqs), n_mels), acc)
    for j in range(n_mels):
        lo, ce, hi = pts[j], pts[j + 1], pts[j + 2]
        up = (freqs >= lo) & (freqs < ce)
        dn = (freqs >= ce) & (freqs <= hi)
        fb[up, j] = (freqs[up] - lo) / (ce - lo)
        fb[dn, j] = (hi - freqs[dn]) / (hi - ce)
    return fb


def fbank(x, cfg, acc=np.float64):
    """computeFbank (:6-39, :105-152) of one waveform -> [F, n_mels]."""
    f = cfg.frontend_conf
    win, hop = f.fs * f.frame_length // 1000, f.fs * f.frame_shift // 1000
    x = np.asarray(x, np.float32)
    if x.ndim > 1:
        x = x.mean(axis=-1, dtype=np.float32)
    x = x.reshape(-1)
    F = frames_of(len(x), win, hop)
    if F == 0:
        return np.zeros((0, f.n_mels), acc)
    a = x.astype(acc)
    if np.abs(x).max() <= 1.0:
        a = a * acc(32768)
    fr = np.stack([a[i * hop: i * hop + win] for i in range(F)])
    fr = fr - fr.mean(axis=1, keepdims=True, dtype=acc)
    fr = np.concatenate([fr[:, :1] - acc(0.97) * fr[:, :1], fr[:, 1:] - acc(0.97) * fr[:, :-1]], axis=1)
    fr = fr * window(f.window, win, acc)
    nfft = 1
    while nfft < win:
        nfft *= 2
    spec = scipy.fft.rfft(fr, n=nfft, axis=1)                          # (single precision for float32 input)
    power = (np.abs(spec) ** 2).astype(acc)
    return np.log(np.maximum(power @ mel_filters(f.fs, nfft, f.n_mels, acc), acc(1e-10))).astype(acc)


def lfr_literal(feats, m, n):
    """applyLFR (:41-72), literally: left pad with the first frame, stack, pad the tail with the last frame."""
    T = feats.shape[0]
    rows = -(-T // n)
    lp = max(0, (m - 1) // 2)
    padded = np.concatenate([np.repeat(feats[:1], lp, axis=0), feats], axis=0) if lp > 0 and T > 0 else feats
    PT = padded.shape[0]
    out = []
    for i in range(rows):
        s, e = i * n, i * n + m
        if e <= PT:
            out.append(padded[s:e].reshape(-1))
        else:
            out.append(np.concatenate([padded[s:PT], np.repeat(padded[PT - 1:PT], e - PT, axis=0)], axis=0).reshape(-1))
    return np.stack(out) if out else np.zeros((0, m * feats.shape[1]), feats.dtype)


def lfr_clamp(feats, m, n):
    """The clamp form the engine computes: row r, slot i = frame clamp(r n + i - (m - 1) / 2, 0, T - 1)."""
    T = feats.shape[0]
    rows = -(-T // n)
    if rows == 0:
        return np.zeros((0, m * feats.shape[1]), feats.dtype)
    idx = np.clip(np.arange(rows)[:, None] * n + np.arange(m)[None] - (m - 1) // 2, 0, T - 1)
    return feats[idx].reshape(rows, -1)


def cmvn_apply(feats, cmvn, acc):
    return feats if cmvn is None else ((feats.astype(acc) + cmvn[0].astype(acc)) * cmvn[1].astype(acc)).astype(acc)


def position_table(T, width, acc):
    """SenseVoiceSinusoidalPositionEncoder (:8-31) for positions 1..T over `width` columns."""
    half = max(width // 2, 1)
    inc = acc(np.log(10000.0) / max(half - 1, 1))
    inv = np.exp(np.arange(half, dtype=acc) * -inc)
    ang = np.arange(1, T + 1, dtype=acc)[:, None] * inv[None]
    enc = np.concatenate([np.sin(ang), np.cos(ang)], axis=1).astype(acc)
    if enc.shape[1] > width:
        enc = enc[:, :width]
    elif enc.shape[1] < width:
        enc = np.concatenate([enc, np.zeros((T, width - enc.shape[1]), acc)], axis=1)
    return enc


def layer_norm(x, w, b, acc):
    x = x.astype(acc)
    mu = x.mean(axis=-1, keepdims=True, dtype=acc)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True, dtype=acc)
    return ((x - mu) / np.sqrt(var + acc(LN_EPS)) * w.astype(acc) + b.astype(acc)).astype(acc)


def fsmn_memory(v, w, left, acc):
    """forwardFSMN (:89-96), literally: pad (left, k - 1 - left) zero rows, depthwise conv, + v.  v [T, D], w [D, k, 1]."""
    T, D = v.shape
    k = w.shape[1]
    padded = np.concatenate([np.zeros((left, D), acc), v.astype(acc), np.zeros((k - 1 - left, D), acc)], axis=0)
    taps = w[:, :, 0].astype(acc)                                     # [D, k]
    mem = np.zeros((T, D), acc)
    for j in range(k):
        mem += padded[j: j + T] * taps[:, j][None]
    return (mem + v.astype(acc)).astype(acc)


class SenseVoiceRef:
    def __init__(self, cfg, W, cmvn=None, acc=np.float64):
        self.cfg, self.cmvn, self.acc = cfg, cmvn, acc
        self.W = {k: np.asarray(v).astype(acc) for k, v in W.items()}
        self.prefixes = mas.sensevoice_layer_prefixes(cfg)
        e = cfg.encoder_conf
        self.N1 = 1 + max(e.num_blocks - 1, 0)
        self.left = (e.kernel_size - 1) // 2 + max(e.sanm_shift, 0)
        self.stages = len(self.prefixes) + 2                          # layers, after_norm, tp_norm

    def lin(self, p, x):
        return (x.astype(self.acc) @ self.W[p + ".weight"].T + self.W[p + ".bias"]).astype(self.acc)

    def features(self, x):
        f = self.cfg.frontend_conf
        return cmvn_apply(lfr_clamp(fbank(x, self.cfg, self.acc), f.lfr_m, f.lfr_n), self.cmvn, self.acc)

    def features_from_fbank(self, fb):
        f = self.cfg.frontend_conf
        return cmvn_apply(lfr_clamp(fb.astype(self.acc), f.lfr_m, f.lfr_n), self.cmvn, self.acc)

    def intake(self, feats, lid=0, textnorm=15):
        acc, E = self.acc, self.W["embed.weight"]
        seq = np.concatenate([E[[lid, 1, 2, textnorm]], feats.astype(acc).reshape(-1, self.cfg.input_size)], axis=0)
        seq = seq * acc(np.sqrt(np.float64(self.cfg.encoder_conf.output_size)))
        return (seq + position_table(seq.shape[0], self.cfg.input_size, acc)).astype(acc)

    def attention(self, q, k, v):
        acc, H = self.acc, self.cfg.encoder_conf.attention_heads
        T, D = q.shape
        dk = D // H
        out = np.zeros((T, D), acc)
        for h in range(H):
            s = slice(h * dk, (h + 1) * dk)
            sc = (q[:, s] * acc(1.0 / np.sqrt(np.float64(dk)))) @ k[:, s].T
            sc = sc - sc.max(axis=1, keepdims=True)
            p = np.exp(sc)
            out[:, s] = (p / p.sum(axis=1, keepdims=True, dtype=acc)) @ v[:, s]
        return out.astype(acc)

    def layer(self, i, x):
        q, acc, e = self.prefixes[i], self.acc, self.cfg.encoder_conf
        x = x.astype(acc)
        y = layer_norm(x, self.W[q + ".norm1.weight"], self.W[q + ".norm1.bias"], acc) if e.normalize_before else x
        qkv = self.lin(q + ".self_attn.linear_q_k_v", y)
        D = e.output_size
        qq, kk, vv = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
        att = self.lin(q + ".self_attn.linear_out", self.attention(qq, kk, vv)) + fsmn_memory(vv, self.W[q + ".self_attn.fsmn_block.weight"], self.left, acc)
        y = x + att if i > 0 else att
        z = layer_norm(y, self.W[q + ".norm2.weight"], self.W[q + ".norm2.bias"], acc) if e.normalize_before else y
        return (y + self.lin(q + ".feed_forward.w_2", np.maximum(self.lin(q + ".feed_forward.w_1", z), 0))).astype(acc)

    def step(self, s, prev):
        """Encoder stage s (0-based in the order the stages run) on the previous stage's output (stage 0: on the intake)."""
        if s == self.N1:
            return layer_norm(prev, self.W["encoder.after_norm.weight"], self.W["encoder.after_norm.bias"], self.acc)
        if s == self.stages - 1:
            return layer_norm(prev, self.W["encoder.tp_norm.weight"], self.W["encoder.tp_norm.bias"], self.acc)
        return self.layer(s if s < self.N1 else s - 1, prev)

    def encoder(self, x0):
        h = x0
        for s in range(self.stages):
            h = self.step(s, h)
        return h

    def logits(self, enc):
        return self.lin("ctc_lo", enc)

    def log_probs_from(self, enc):
        z = self.logits(enc)
        z = z - z.max(axis=1, keepdims=True)
        return (z - np.log(np.exp(z).sum(axis=1, keepdims=True, dtype=self.acc))).astype(self.acc)

    def log_probs(self, x, lid=0, textnorm=15):
        return self.log_probs_from(self.encoder(self.intake(self.features(x), lid, textnorm)))


def greedy_ctc(pred, blank=0):
    """greedyCTCDecode (:392-405) on the arg-max ids of frames 4..: dedupe, then drop the blank."""
    out, prev = [], None
    for t in pred:
        if t != prev:
            out.append(int(t))
            prev = t
    return [t for t in out if t != blank]


def rich_ids(pred):
    return [int(pred[0]), int(pred[1]), int(pred[2])]
