"""CPU restatement of MossFormer2-SE (Sources/MLXAudioSTS/Models/MossFormer2SE: MossFormer2Model.swift, MossFormer2Layers.swift,
MossFormer2DSP.swift; melFilters of MLXAudioCore/DSP.swift), written from the Swift: torch, float32 or float64, one row at a time.
test_mossformer2_cpu.py holds it to numpy / scipy and torch.nn; test_gpu_mossformer2.py holds the device to it.

Stages are numbered as mis_mossformer2_tap numbers them.  `step(stage, get)` computes one stage from the stage(s) before it, which
`get(stage)` returns for the row ([T, width] tensors) - the GPU test passes the device's own taps.

Two definitions fix what the Swift leaves to its runtime, and both dtypes share them: the window and the mel filters are the float32
values the reference's own float32 arithmetic gives; an angle (position x inverse frequency, for the sinusoidal embedding and for
RoPE) is the float32 product, as MLX forms it, and its sine / cosine are evaluated in the working dtype.  RoPE's inverse frequencies
are 10000^(-2 i / 32) rounded to float32."""
import math

import numpy as np
import torch

import mlx_audio_swift_amd as mas

GROUP, QK, INNER, FF_TAPS, FSMN_TAPS, ROPE_DIMS = 256, 128, 256, 17, 39, 32
PREFIX = "model.mossformer."
SEED = 11
INNER_STAGES = 13


def case_config(name: str, num_blocks: int = 2, **workspace) -> mas.MossFormer2SEConfig:
    """S: no free width is a multiple of a tile, fft_len 320 is no power of two, the fbank FFT has 512 points.  P: the published shape."""
    workspace.setdefault("max_batch", 8)
    if name == "S":
        workspace.setdefault("max_seconds", 2.5)
        return mas.MossFormer2SEConfig(sample_rate=16000, win_len=320, win_inc=64, fft_len=320, num_mels=20, in_channels=60, out_channels=96,
                                       out_channels_final=161, num_blocks=num_blocks, **workspace)
    workspace.setdefault("max_seconds", 5.0)
    return mas.MossFormer2SEConfig(num_blocks=num_blocks, **workspace)


def frames_of(cfg, n: int) -> int:
    return 0 if n < cfg.win_len else 1 + (n - cfg.win_len) // cfg.win_inc


def out_len(cfg, T: int) -> int:
    return (T - 1) * cfg.win_inc + min(cfg.win_len, cfg.fft_len) if T else 0


ROW_FRAMES = (0, 1, 2, 255, 256, 257, 600, 40)


def case_rows(cfg) -> list:
    """Noise of differing amplitude with 0 (win_len - 1 samples), 1, 2, 255, 256, 257 and 600 frames, and an all-zero row of 40."""
    g = torch.Generator().manual_seed(5)
    rows = []
    for i, T in enumerate(ROW_FRAMES):
        n = cfg.win_len - 1 if T == 0 else cfg.win_len + (T - 1) * cfg.win_inc + (7 * i) % cfg.win_inc
        amp = 0.0 if i == 7 else 0.02 * (1 + i)
        rows.append((amp * torch.randn(n, generator=g)).numpy().astype(np.float32))
    return rows


def make_weights(cfg, seed: int = SEED) -> dict:
    """Sanitized names -> float32 tensors: every key of mossformer2_expected_shapes.  The scales keep the activations of 24 blocks of
    order one, let about half of the quadratic scores pass the ReLU in every layer, and leave both attention terms visible."""
    g = torch.Generator().manual_seed(seed)
    shapes = mas.mossformer2_expected_shapes(cfg)
    D = cfg.out_channels

    def u(shape, a):
        return (torch.rand(shape, generator=g) * 2 - 1) * a

    W = {}
    for k, shape in shapes.items():
        n = k[len(PREFIX):]
        if n == "pos_enc.inv_freq":                                  # ScaledSinuEmbedding.init, float32 as the reference forms it
            pos = np.arange(0, D, 2, dtype=np.float32)
            W[k] = torch.from_numpy((np.float32(1.0) / np.power(np.float32(10000.0), pos / np.float32(D))).astype(np.float32))
        elif n == "pos_enc.scale":
            W[k] = torch.tensor([0.9])
        elif n.endswith("norm.g"):
            W[k] = 1.0 + u((1,), 0.1)
        elif n.endswith("prelu.weight"):
            W[k] = torch.tensor(0.25) + u((), 0.05)
        elif n.endswith("qk_offset_scale.gamma"):
            sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
            mag = 0.5 + torch.rand(shape, generator=g)
            # the quadratic heads live on the first 16 of the 32 rotated dims (RoPE angles of 1 .. 0.018 rad a frame), so a score turns
            # with the distance between query and key and about half of a group's scores pass the ReLU at any depth; on the other dims a
            # score would carry a constant sum(gamma_q gamma_k mean^2) that grows with the residual stream and parks a whole layer at 0 or
            # 100 %.  The linear heads are scaled so that both attention terms stay within two orders of magnitude of each other.
            quad = torch.cat([torch.full((16,), 4.5), torch.full((shape[1] - 16,), 0.2)])
            mag[0] *= quad; mag[2] *= quad
            mag[1] *= 0.6; mag[3] *= 0.6
            W[k] = sign * mag
        elif n.endswith("qk_offset_scale.beta"):
            W[k] = u(shape, 0.2)
        elif "conv_module.weight" in n or n.endswith("fsmn.conv1.weight"):
            W[k] = u(shape, 0.5 * math.sqrt(3.0 / shape[1]))
        elif n.endswith(".bias") and ("norm" in n.split(".")[-2]):
            W[k] = u(shape, 0.05)
        elif n.endswith(".weight") and ("norm" in n.split(".")[-2]):
            W[k] = 1.0 + u(shape, 0.1)
        elif n.endswith(".bias"):
            W[k] = u(shape, 0.05)
        else:                                                         # Linear [out, in] / Conv1d [out, 1, in]
            gain = 0.5 if n.endswith("conv2.weight") else 1.0
            W[k] = u(shape, gain * math.sqrt(3.0 / shape[-1]))
    return {k: v.to(torch.float32).contiguous() for k, v in W.items()}


# ------------------------------------------------------------------------------------------------------------ tables
def window_f32(cfg) -> np.ndarray:
    """hammingWindow / hannWindow(periodic: false) in the reference's float32 arithmetic; the cosine of the float32 phase is taken in
    double and rounded."""
    n = cfg.win_len
    phase = (np.float32(2.0) * np.float32(np.pi) * np.arange(n, dtype=np.float32)) / np.float32(n - 1)
    c = np.cos(phase.astype(np.float64)).astype(np.float32)
    if "hann" in cfg.win_type.lower():
        return (np.float32(0.5) - np.float32(0.5) * c).astype(np.float32)
    return (np.float32(0.54) - np.float32(0.46) * c).astype(np.float32)


def nfft_of(cfg) -> int:
    n = 1
    while n < cfg.win_len:
        n <<= 1
    return n


def mel_filters_f32(cfg) -> np.ndarray:
    """melFilters(sampleRate, nFft, nMels, fMin: 20, norm: nil, .htk) in float32: [nFft / 2 + 1, nMels], triangles in Hz."""
    f32 = np.float32
    sr, nfft, nm = f32(cfg.sample_rate), nfft_of(cfg), cfg.num_mels
    freqs = (np.arange(nfft // 2 + 1, dtype=np.float32) * sr / f32(nfft)).astype(np.float32)
    h2m = lambda f: (f32(2595.0) * np.log10(f32(1.0) + f / f32(700.0), dtype=np.float32)).astype(np.float32)
    m2h = lambda m: (f32(700.0) * (np.power(f32(10.0), m / f32(2595.0), dtype=np.float32) - f32(1.0))).astype(np.float32)
    mmin, mmax = h2m(f32(20.0)), h2m(sr / f32(2.0))
    pts = (mmin + np.arange(nm + 2, dtype=np.float32) * (mmax - mmin) / f32(nm + 1)).astype(np.float32)
    fp = m2h(pts)
    fb = np.zeros((len(freqs), nm), np.float32)
    for j in range(nm):
        lo, ce, hi = fp[j], fp[j + 1], fp[j + 2]
        up = (freqs >= lo) & (freqs < ce)
        dn = (freqs >= ce) & (freqs <= hi)
        fb[up, j] = (freqs[up] - lo) / (ce - lo)
        fb[dn, j] = (hi - freqs[dn]) / (hi - ce)
    return fb


def angles(T: int, inv_freq_f32: np.ndarray) -> np.ndarray:
    """float32(t) x inv_freq, rounded to float32: [T, len(inv_freq)]."""
    return (np.arange(T, dtype=np.float32)[:, None] * inv_freq_f32.astype(np.float32)[None, :]).astype(np.float32)


def rope_inv_freq() -> np.ndarray:
    return np.power(10000.0, -2.0 * np.arange(ROPE_DIMS // 2, dtype=np.float64) / ROPE_DIMS).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ the model
class MossFormer2Ref:
    def __init__(self, cfg, weights: dict, dtype=torch.float64):
        self.cfg, self.dt = cfg, dtype
        self.W = {k[len(PREFIX):]: v.to(dtype) for k, v in weights.items()}
        self.NB, self.D = cfg.num_blocks, cfg.out_channels
        self.base = 4 + 2 * self.NB
        self.win = torch.from_numpy(window_f32(cfg)).to(dtype)
        self.fb = torch.from_numpy(mel_filters_f32(cfg)).to(dtype)
        self.Wn = min(cfg.win_len, cfg.fft_len)

    # -- front end ------------------------------------------------------------------------------------
    def frames(self, x) -> torch.Tensor:
        """[T, win_len] frames of the x 32768 waveform."""
        c = self.cfg
        a = torch.as_tensor(np.asarray(x, np.float32)).to(self.dt) * 32768.0
        T = frames_of(c, len(a))
        if T == 0:
            return torch.zeros(0, c.win_len, dtype=self.dt)
        return a.unfold(0, c.win_len, c.win_inc)[:T]

    def fbank(self, x) -> torch.Tensor:
        c = self.cfg
        fr = self.frames(x)
        if fr.shape[0] == 0:
            return torch.zeros(0, c.num_mels, dtype=self.dt)
        fr = fr - fr.mean(dim=1, keepdim=True)
        pre = torch.tensor(np.float32(c.preemphasis), dtype=self.dt)
        fr = torch.cat([fr[:, :1] - pre * fr[:, :1], fr[:, 1:] - pre * fr[:, :-1]], dim=1) * self.win
        power = torch.fft.rfft(fr, n=nfft_of(c), dim=1).abs() ** 2
        return torch.log(torch.clamp(power @ self.fb, min=float(np.float32(1e-10))))

    @staticmethod
    def deltas(f: torch.Tensor) -> torch.Tensor:
        """computeDeltasKaldi over time: [-2, -1, 0, 1, 2] / 10 with edge padding; f is [T, C]."""
        T = f.shape[0]
        idx = torch.arange(T)
        out = torch.zeros_like(f)
        for k in (1, 2):                                              # the filter is odd: k / 10 (x[t + k] - x[t - k])
            out = out + (k / 10.0) * (f[(idx + k).clamp(0, T - 1)] - f[(idx - k).clamp(0, T - 1)])
        return out

    def features(self, x) -> torch.Tensor:
        f = self.fbank(x)
        if f.shape[0] == 0:
            return torch.zeros(0, 3 * self.cfg.num_mels, dtype=self.dt)
        d = self.deltas(f)
        return torch.cat([f, d, self.deltas(d)], dim=1)

    # -- layers ---------------------------------------------------------------------------------------
    def lin(self, p, x, bias=True):
        w = self.W[p + ".weight"]
        y = x @ w.reshape(w.shape[0], -1).t()
        return y + self.W[p + ".bias"] if bias else y

    def dwres(self, name, y):
        """y + depthwise conv over time with zero padding, weight [C, K, 1(, 1)]."""
        w = self.W[name]
        w = w.reshape(w.shape[0], w.shape[1])
        K = w.shape[1]
        pad = (K - 1) // 2
        yp = torch.nn.functional.pad(y, (0, 0, pad, pad))
        out = y.clone()
        for j in range(K):
            out = out + yp[j: j + y.shape[0]] * w[:, j]
        return out

    def scalenorm(self, p, x):
        norm = torch.sqrt((x * x).sum(-1, keepdim=True)) * (x.shape[-1] ** -0.5)
        return x * (self.W[p + ".g"] / torch.clamp(norm, min=1e-8))

    @staticmethod
    def layernorm(x, w, b, eps):
        m = x.mean(-1, keepdim=True)
        v = ((x - m) ** 2).mean(-1, keepdim=True)
        return (x - m) / torch.sqrt(v + eps) * w + b

    def ff_pre(self, p, x, scale_norm):
        """FFConvM up to the SiLU."""
        n = self.scalenorm(p + ".norm", x) if scale_norm else self.layernorm(x, self.W[p + ".norm.weight"], self.W[p + ".norm.bias"], 1e-5)
        y = self.lin(p + ".linear", n)
        return y * torch.sigmoid(y)

    def shift(self, x):
        if x.shape[0] <= 1:
            return x
        h = x.shape[1] // 2
        return torch.cat([torch.cat([torch.zeros(1, h, dtype=x.dtype), x[:-1, :h]], 0), x[:, h:]], 1)

    def L(self, i):
        return f"mdl.intra_mdl.mossformerM.layers.{i}"

    def Fs(self, i):
        return f"mdl.intra_mdl.mossformerM.fsmn.{i}"

    def hq(self, i, x):
        s = self.shift(x)
        return torch.cat([self.ff_pre(self.L(i) + ".to_hidden", s, True), self.ff_pre(self.L(i) + ".to_qk", s, True)], 1)

    def vu(self, i, hq):
        D = self.D
        return self.dwres(self.L(i) + ".to_hidden.conv_module.weight", hq[:, : 4 * D])

    def qk4(self, i, hq):
        """[T, 4 x 128]: quadQ | linQ | quadK | linK after OffsetScale and RoPE (traditional, the first 32 dims)."""
        qk = self.dwres(self.L(i) + ".to_qk.conv_module.weight", hq[:, 4 * self.D:])
        T = qk.shape[0]
        heads = qk[:, None, :] * self.W[self.L(i) + ".qk_offset_scale.gamma"] + self.W[self.L(i) + ".qk_offset_scale.beta"]
        th = torch.from_numpy(angles(T, rope_inv_freq())).to(self.dt)
        cs, sn = torch.cos(th)[:, None, :], torch.sin(th)[:, None, :]
        a, b = heads[:, :, 0:ROPE_DIMS:2], heads[:, :, 1:ROPE_DIMS:2]
        rot = torch.stack([a * cs - b * sn, a * sn + b * cs], dim=-1).reshape(T, 4, ROPE_DIMS)
        return torch.cat([rot, heads[:, :, ROPE_DIMS:]], dim=-1).reshape(T, 4 * QK)

    def attention(self, qk4, vu, parts=False):
        """calAttention + the gate: [T, 2 D]."""
        T, D2 = vu.shape[0], vu.shape[1] // 2
        q4 = qk4.reshape(T, 4, QK)
        quadq, linq, quadk, link = q4[:, 0], q4[:, 1], q4[:, 2], q4[:, 3]
        pad = (GROUP - T % GROUP) % GROUP
        P = lambda z: torch.nn.functional.pad(z, (0, 0, 0, pad))
        G = (T + pad) // GROUP
        qg, kg, vg = P(quadq).reshape(G, GROUP, QK), P(quadk).reshape(G, GROUP, QK), P(vu).reshape(G, GROUP, 2 * D2)
        sim = qg @ kg.transpose(1, 2) / GROUP
        attn = torch.relu(sim) ** 2
        quad = (attn @ vg).reshape(G * GROUP, 2 * D2)[:T]
        lin = linq @ (link.t() @ vu / T)
        att = quad + lin
        v, u_ = vu[:, :D2], vu[:, D2:]
        out = (att[:, D2:] * v) * torch.sigmoid(att[:, :D2] * u_)
        if parts:
            live = torch.ones(T + pad, dtype=torch.bool)
            live[T:] = False
            m = live.reshape(G, GROUP)[:, :, None] & live.reshape(G, GROUP)[:, None, :]
            return out, quad, lin, float((sim[m] > 0).double().mean())
        return out

    def to_out_pre(self, i, att):
        return self.ff_pre(self.L(i) + ".to_out", att, True)

    def flash(self, i, x):
        hq = self.hq(i, x)
        y = self.to_out_pre(i, self.attention(self.qk4(i, hq), self.vu(i, hq)))
        return x + self.dwres(self.L(i) + ".to_out.conv_module.weight", y)

    def prelu(self, name, x):
        a = self.W[name]
        return torch.clamp(x, min=0) + a * torch.clamp(x, max=0)

    def c1(self, i, x):
        return self.prelu(self.Fs(i) + ".prelu.weight", self.lin(self.Fs(i) + ".conv1", x))

    def cln(self, p, x):
        return self.layernorm(x, self.W[p + ".weight"], self.W[p + ".bias"], 1e-8)

    def uv(self, i, n1):
        g = self.Fs(i) + ".gated_fsmn"
        return torch.cat([self.ff_pre(g + ".to_u", n1, False), self.ff_pre(g + ".to_v", n1, False)], 1)

    def uv2(self, i, uv):
        g = self.Fs(i) + ".gated_fsmn"
        return torch.cat([self.dwres(g + ".to_u.conv_module.weight", uv[:, :INNER]), self.dwres(g + ".to_v.conv_module.weight", uv[:, INNER:])], 1)

    def f1(self, i, uv2):
        return torch.relu(self.lin(self.Fs(i) + ".gated_fsmn.fsmn.linear", uv2[:, :INNER]))

    def p1(self, i, f1):
        return self.lin(self.Fs(i) + ".gated_fsmn.fsmn.project", f1, bias=False)

    def gate(self, i, p1, uv2, n1):
        xu = uv2[:, :INNER] + self.dwres(self.Fs(i) + ".gated_fsmn.fsmn.conv1.weight", p1)
        return uv2[:, INNER:] * xu + n1

    def fsmn_block(self, i, x):
        n1 = self.cln(self.Fs(i) + ".norm1", self.c1(i, x))
        uv2 = self.uv2(i, self.uv(i, n1))
        g = self.gate(i, self.p1(i, self.f1(i, uv2)), uv2, n1)
        return self.lin(self.Fs(i) + ".conv2", self.cln(self.Fs(i) + ".norm2", g)) + x

    def gln(self, f):
        m = f.mean()
        v = ((f - m) ** 2).mean()
        return self.W["norm.weight"][:, 0] * ((f - m) / torch.sqrt(v + 1e-8)) + self.W["norm.bias"][:, 0]

    def positions(self, T):
        th = torch.from_numpy(angles(T, self.W["pos_enc.inv_freq"].to(torch.float32).numpy())).to(self.dt)
        return torch.cat([torch.sin(th), torch.cos(th)], 1) * self.W["pos_enc.scale"]

    def encode(self, xn):
        return self.lin("conv1d_encoder", xn, bias=False) + self.positions(xn.shape[0])

    def tail(self, y, x0):
        z = self.layernorm(y, self.W["mdl.intra_mdl.norm.weight"], self.W["mdl.intra_mdl.norm.bias"], 1e-8)
        z = self.layernorm(z, self.W["mdl.intra_norm.weight"], self.W["mdl.intra_norm.bias"], 1e-8)
        return self.prelu("prelu.weight", z + x0)

    def conv_out(self, t):
        """Speaker 0: the first out_channels outputs of conv1d_out."""
        D = self.D
        return t @ self.W["conv1d_out.weight"].reshape(2 * D, D)[:D].t() + self.W["conv1d_out.bias"][:D]

    def og(self, co):
        """tanh(output) | sigmoid(output_gate)."""
        return torch.cat([torch.tanh(self.lin("output", co)), torch.sigmoid(self.lin("output_gate", co))], 1)

    def decode(self, og):
        D = self.D
        return torch.relu(self.lin("conv1_decoder", og[:, :D] * og[:, D:], bias=False))

    # -- stages ---------------------------------------------------------------------------------------
    def step(self, stage: int, get):
        """Stage `stage` of one row from the stages before it; get(s) returns stage s of the row."""
        NB, base, Lb = self.NB, self.base, self.NB - 1
        if stage == 2:
            return self.gln(get(1))
        if stage == 3:
            return self.encode(get(2))
        if stage < base:
            i, fs = (stage - 4) // 2, (stage - 4) % 2
            return self.fsmn_block(i, get(stage - 1)) if fs else self.flash(i, get(stage - 1))
        if stage == base:
            return self.tail(get(base - 1), get(3))
        if stage == base + 1:
            return self.conv_out(get(base))
        if stage == base + 2:
            return self.og(get(base + 1))
        if stage == base + 3:
            return self.decode(get(base + 2))
        k, i0 = stage - base - 7, base + 7
        x, xa = (lambda: get(3 + 2 * Lb)), (lambda: get(4 + 2 * Lb))
        if k == 0: return self.hq(Lb, x())
        if k == 1: return self.vu(Lb, get(i0))
        if k == 2: return self.qk4(Lb, get(i0))
        if k == 3: return self.attention(get(i0 + 2), get(i0 + 1))
        if k == 4: return self.to_out_pre(Lb, get(i0 + 3))
        if k == 5: return self.c1(Lb, xa())
        if k == 6: return self.cln(self.Fs(Lb) + ".norm1", get(i0 + 5))
        if k == 7: return self.uv(Lb, get(i0 + 6))
        if k == 8: return self.uv2(Lb, get(i0 + 7))
        if k == 9: return self.f1(Lb, get(i0 + 8))
        if k == 10: return self.p1(Lb, get(i0 + 9))
        if k == 11: return self.gate(Lb, get(i0 + 10), get(i0 + 8), get(i0 + 6))
        if k == 12: return self.cln(self.Fs(Lb) + ".norm2", get(i0 + 11))
        raise ValueError(stage)

    def mask_from_features(self, f, want_max=False):
        """The whole network on features [T, in_channels] -> mask [T, out_channels_final] (and the largest activation seen)."""
        x0 = self.encode(self.gln(f))
        x, big = x0, float(x0.abs().max())
        for i in range(self.NB):
            x = self.flash(i, x); big = max(big, float(x.abs().max()))
            x = self.fsmn_block(i, x); big = max(big, float(x.abs().max()))
        m = self.decode(self.og(self.conv_out(self.tail(x, x0))))
        return (m, big) if want_max else m

    # -- synthesis ------------------------------------------------------------------------------------
    def stft(self, x) -> torch.Tensor:
        """[T, 2 F]: real | imaginary parts of the first T frames' fft_len-point transform."""
        c = self.cfg
        fr = self.frames(x)[:, : self.Wn] * self.win[: self.Wn]
        s = torch.fft.rfft(fr, n=c.fft_len, dim=1)
        return torch.cat([s.real, s.imag], 1)

    def istft_frames(self, spec, mask) -> torch.Tensor:
        """(spectrum x mask) -> irfft -> x window: [T, W]."""
        F = spec.shape[1] // 2
        z = torch.complex(spec[:, :F] * mask, spec[:, F:] * mask)
        return torch.fft.irfft(z, n=self.cfg.fft_len, dim=1)[:, : self.Wn] * self.win[: self.Wn]

    def overlap_add(self, fr) -> torch.Tensor:
        c, T, W = self.cfg, fr.shape[0], self.Wn
        out = torch.zeros(out_len(c, T), dtype=self.dt)
        ws = torch.zeros_like(out)
        w2 = self.win[:W] ** 2
        for t in range(T):
            out[t * c.win_inc: t * c.win_inc + W] += fr[t]
            ws[t * c.win_inc: t * c.win_inc + W] += w2
        return out / torch.clamp(ws, min=1e-8) / 32768.0

    def synthesize(self, x, mask) -> torch.Tensor:
        return self.overlap_add(self.istft_frames(self.stft(x), mask))

    def enhance_from(self, x, features) -> tuple:
        """(mask, waveform) of a row whose features are given (the device's own, in the chained test)."""
        m = self.mask_from_features(features)
        return m, self.synthesize(x, m)

    def enhance(self, x) -> torch.Tensor:
        if frames_of(self.cfg, len(x)) == 0:
            return torch.zeros(0, dtype=self.dt)
        return self.enhance_from(x, self.features(x))[1]
