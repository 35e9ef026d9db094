"""EnCodec encode path, numpy specification in float64 (and a float32 twin, used ONLY to measure the specification's own
float32-to-float64 distance).  Test infrastructure.

Follows Sources/MLXAudioCodecs/Encodec/: Encodec.encodeFrame / encode (Encodec.swift:212-291: masked input, mono mean, scale =
sqrt(mean_t mono^2) + 1e-8; the chunk walk `while offset < L - (chunk - stride)`), EncodecEncoder (:17-89), EncodecConv1d with
getExtraPaddingForConv1d and the reflect rule min(left - i, T - 1) / max(T - 2 - i, 0) (EncodecLayers.swift:92-211),
EncodecResnetBlock, EncodecLSTMBlock, EncodecResidualVectorQuantizer.encode (EncodecQuantization.swift:22-32,100-114: arg-max of
-(|r|^2 - 2 r.e + |e|^2), first maximum on ties; r -= E[code]).  Layout [B, C, T].

Planted faults (tests/test_encodec_encode_cpu.py shows each one changes the expected outputs): fault = "extra0" (extra padding 0),
"reflect_swap" (left / right reflect rules swapped), "tie_high" (ties to the higher index), "no_update" (residual not updated).

THE FLOAT32 SEARCH BOUND (rvq_bound).  A float32 search scores entry e of frame residual r as fl(2 fl(r.e) - fl(|e|^2)); r and e are
float32 numbers, so the inputs are exact.  With u = 2^-24: a float32 dot product of D terms, summed in any order (fused or not), is
off by at most gamma_D sum|r_i e_i| <= gamma_D |r||e|, gamma_D = D u / (1 - D u); |e|^2 likewise by gamma_D |e|^2; the doubling is
exact and the final subtraction adds u (2|r||e| + |e|^2)(1 + gamma_D).  In all the score is off by at most
(D + 2) u (2|r||e| + |e|^2) <= (D + 2) u (|r| + |e|)^2 (D u << 1 absorbs the second-order terms).  The search takes entry c over the
true nearest m only if its computed score is no smaller, so the float64 distances obey
    |r - e_c|^2 - |r - e_m|^2 <= err_c + err_m <= 2 (D + 2) 2^-24 (|r| + max_e |e|)^2 = rvq_bound(r, E).
The same figure decides the exempt entries of the end-to-end comparison: where the specification's own top-2 gap is under it, a
correct float32 search may return either entry."""
from __future__ import annotations

import math
from dataclasses import replace

import numpy as np

from oracle import encodec as oe
from oracle import synth

U24 = 2.0 ** -24


def rvq_bound(r_norm, e_norm_max, D):
    return 2.0 * (D + 2) * U24 * (r_norm + e_norm_max) ** 2


def num_quantizers_for_bandwidth(cfg, bandwidth):
    """getNumQuantizersForBandwidth (EncodecQuantization.swift:90-97)"""
    frame_rate = int(math.ceil(cfg.sampling_rate / cfg.hop_length))
    n = cfg.num_quantizers
    if bandwidth is not None and bandwidth > 0.0:
        n = max(1, int(math.floor(np.float32(bandwidth) * np.float32(1000) / (np.float32(math.log2(cfg.codebook_size)) * np.float32(frame_rate)))))
    return n


def num_frames(cfg, L):
    for r in reversed(cfg.upsampling_ratios):
        L = -(-L // r)
    return L


def make_synthetic_encoder_weights(cfg, seed: int = 515) -> dict:
    """encoder.layers.* of EncodecEncoder (numbering of Encodec.swift:17-72), in the style of oracle.encodec.make_synthetic_weights"""
    W, key = {}, [seed * 100000]

    def t(shape, amp):
        key[0] += 1
        return synth.synth_tensor(key[0], shape, amp)

    def conv(p, co, k, ci, gain=1.0):
        W[p + ".conv.weight"] = t((co, k, ci), gain * math.sqrt(3.0 / (k * ci)))
        W[p + ".conv.bias"] = t((co,), 0.05)
        if cfg.norm_type == "time_group_norm":
            W[p + ".norm.weight"] = (1.0 + t((co,), 0.3)).astype(np.float32)
            W[p + ".norm.bias"] = t((co,), 0.1)

    dim = cfg.num_filters
    conv("encoder.layers.0", dim, cfg.kernel_size, cfg.audio_channels, gain=2.0)
    li = 1
    for ratio in reversed(cfg.upsampling_ratios):
        for _ in range(cfg.num_residual_layers):
            p = f"encoder.layers.{li}"
            conv(p + ".block.1", dim // cfg.compress, cfg.residual_kernel_size, dim)
            conv(p + ".block.3", dim, 1, dim // cfg.compress, gain=0.5)
            if cfg.use_conv_shortcut:
                conv(p + ".shortcut", dim, 1, dim)
            li += 1
        conv(f"encoder.layers.{li + 1}", 2 * dim, 2 * ratio, dim, gain=1.5)
        li += 2
        dim *= 2
    for j in range(cfg.num_lstm_layers):
        p = f"encoder.layers.{li}.lstm.{j}"
        W[p + ".Wx"] = t((4 * dim, dim), math.sqrt(3.0 / dim))
        W[p + ".Wh"] = t((4 * dim, dim), math.sqrt(3.0 / dim))
        W[p + ".bias"] = t((4 * dim,), 0.1)
    conv(f"encoder.layers.{li + 2}", cfg.hidden_size, cfg.last_kernel_size, dim, gain=1.5)
    return W


def make_synthetic_weights(cfg, seed: int = 909) -> dict:
    """decoder and codebooks of oracle.encodec + the encoder"""
    W = dict(oe.make_synthetic_weights(cfg, seed))
    W.update(make_synthetic_encoder_weights(cfg, seed + 1))
    return W


def elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


class EncodeRef:
    def __init__(self, cfg, weights: dict, dtype=np.float64, normalize: bool = False, chunk_length=None, chunk_stride=None, fault: str | None = None):
        self.cfg, self.dt, self.normalize, self.fault = cfg, dtype, normalize, fault
        self.chunk_length, self.chunk_stride = chunk_length, chunk_stride
        self.w = {k: np.asarray(v, np.float32).astype(dtype) for k, v in weights.items()}

    # ---- layers
    def pad1d(self, x, left, right):
        if self.cfg.pad_mode != "reflect":
            return np.pad(x, ((0, 0), (0, 0), (left, right)))
        n = x.shape[-1]
        li = [min(left - i, n - 1) for i in range(left)]
        ri = [max(n - 2 - i, 0) for i in range(right)]
        if self.fault == "reflect_swap":
            li, ri = [max(n - 2 - i, 0) for i in range(left)], [min(right - i, n - 1) for i in range(right)]
        return np.concatenate([x[..., li], x, x[..., ri]], -1)

    def norm(self, p, h):
        if self.cfg.norm_type != "time_group_norm":
            return h
        mu = h.mean(axis=(1, 2), keepdims=True)
        var = ((h - mu) ** 2).mean(axis=(1, 2), keepdims=True)
        return (h - mu) / np.sqrt(var + self.dt(1e-5)) * self.w[p + ".norm.weight"][None, :, None] + self.w[p + ".norm.bias"][None, :, None]

    def conv(self, p, x, k, stride=1, dilation=1):
        keff, ptotal, n = (k - 1) * dilation + 1, k - stride, x.shape[-1]
        nfr = (n - keff + ptotal) / stride + 1
        extra = max(0, (int(math.ceil(nfr)) - 1) * stride + keff - ptotal - n)
        if self.fault == "extra0":
            extra = 0
        if self.cfg.use_causal_conv:
            xp = self.pad1d(x, ptotal, extra)
        else:
            xp = self.pad1d(x, ptotal - ptotal // 2, ptotal // 2 + extra)
        F = (xp.shape[-1] - keff) // stride + 1
        cols = np.stack([xp[:, :, j * dilation: j * dilation + (F - 1) * stride + 1: stride] for j in range(k)])     # [k, B, C, F]
        y = np.einsum("ojc,jbcf->bof", self.w[p + ".conv.weight"], cols) + self.w[p + ".conv.bias"][None, :, None]
        return self.norm(p, y.astype(self.dt))

    def resnet(self, p, h, j):
        cfg = self.cfg
        t = self.conv(p + ".block.1", elu(h), cfg.residual_kernel_size, dilation=cfg.dilation_growth_rate ** j)
        t = self.conv(p + ".block.3", elu(t), 1)
        return (self.conv(p + ".shortcut", h, 1) if cfg.use_conv_shortcut else h) + t

    def lstm_block(self, p, h):
        y = np.swapaxes(h, 1, 2)                                        # [B, T, C]
        r = y
        for j in range(self.cfg.num_lstm_layers):
            Wx, Wh, b = (self.w[f"{p}.lstm.{j}.{n}"] for n in ("Wx", "Wh", "bias"))
            H = Wh.shape[1]
            xp = r @ Wx.T + b
            hs, c, out = None, np.zeros((r.shape[0], H), self.dt), []
            for t in range(r.shape[1]):
                g = xp[:, t] + (hs @ Wh.T if hs is not None else 0.0)
                i, f, gg, o = sigmoid(g[:, :H]), sigmoid(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), sigmoid(g[:, 3 * H:])
                c = f * c + i * gg
                hs = o * np.tanh(c)
                out.append(hs)
            r = np.stack(out, 1).astype(self.dt)
        return np.swapaxes(r + y, 1, 2)

    # ---- stages: ("norm", "conv0", "down0".., "lstm", "emb"); stage(name, x) maps the previous stage's output to this one's
    def stage_names(self):
        return ["norm", "conv0"] + [f"down{i}" for i in range(len(self.cfg.upsampling_ratios))] + ["lstm", "emb"]

    def _layer_index(self, name):
        cfg = self.cfg
        per = cfg.num_residual_layers + 2
        n = len(cfg.upsampling_ratios)
        if name.startswith("down"):
            return 1 + int(name[4:]) * per
        return 1 + n * per + (0 if name == "lstm" else 2)

    def normalise(self, x, mask=None):
        """x [B, C, L], mask [B, L] -> (values, scale [B]) (Encodec.swift:227-233); identity and None without normalize"""
        x = np.asarray(x).astype(self.dt)
        if not self.normalize:
            return x, None
        if mask is not None:
            x = x * np.asarray(mask).astype(self.dt)[:, None, :]
        mono = x.sum(axis=1, keepdims=True) / self.dt(x.shape[1])
        scale = np.sqrt((mono ** 2).mean(axis=2, keepdims=True)) + self.dt(1e-8)
        return (x / scale).astype(self.dt), scale[:, 0, 0].astype(self.dt)

    def stage(self, name, x, mask=None):
        cfg = self.cfg
        x = np.asarray(x).astype(self.dt)
        if name == "norm":
            return self.normalise(x, mask)[0]
        if name == "conv0":
            return self.conv("encoder.layers.0", x, cfg.kernel_size)
        li = self._layer_index(name)
        if name.startswith("down"):
            ratio = list(reversed(cfg.upsampling_ratios))[int(name[4:])]
            for j in range(cfg.num_residual_layers):
                x = self.resnet(f"encoder.layers.{li + j}", x, j)
            return self.conv(f"encoder.layers.{li + cfg.num_residual_layers + 1}", elu(x), 2 * ratio, stride=ratio)
        if name == "lstm":
            return self.lstm_block(f"encoder.layers.{li}", x)
        return self.conv(f"encoder.layers.{li}", elu(x), cfg.last_kernel_size)

    def encoder(self, x, mask=None):
        """[B, C, L] -> embeddings [B, hidden, F]"""
        for name in self.stage_names():
            x = self.stage(name, x, mask)
        return x

    # ---- residual VQ
    def codebook(self, q):
        return self.w[f"quantizer.layers.{q}.codebook.embed"]

    def rvq(self, emb, n_q):
        """emb [B, D, F] -> codes int64 [B, n_q, F], residuals [n_q + 1, B, D, F], gaps [B, n_q, F] (top-2 score gap = distance gap),
        bounds [B, n_q, F] (rvq_bound of that residual)"""
        r = np.swapaxes(np.asarray(emb).astype(self.dt), 1, 2).copy()        # [B, F, D]
        B, F, D = r.shape
        codes, res, gaps, bounds = [], [np.swapaxes(r, 1, 2).copy()], [], []
        for q in range(n_q):
            E = self.codebook(q)
            score = -((r ** 2).sum(-1, keepdims=True) - 2 * (r @ E.T) + (E ** 2).sum(-1)[None, None, :])     # [B, F, CB]
            if self.fault == "tie_high":
                idx = score.shape[-1] - 1 - np.argmax(score[..., ::-1], -1)
            else:
                idx = np.argmax(score, -1)                                   # first maximum
            top = np.sort(score, -1)
            gaps.append(top[..., -1] - top[..., -2] if score.shape[-1] > 1 else np.full(idx.shape, np.inf))
            bounds.append(rvq_bound(np.sqrt((r.astype(np.float64) ** 2).sum(-1)), float(np.sqrt((E.astype(np.float64) ** 2).sum(-1)).max()), D))
            if self.fault != "no_update":
                r = (r - E[idx]).astype(self.dt)
            codes.append(idx)
            res.append(np.swapaxes(r, 1, 2).copy())
        return np.stack(codes, 1), np.stack(res), np.stack(gaps, 1), np.stack(bounds, 1)

    # ---- Encodec.encode (Encodec.swift:248-291): input_values [B, L, C]
    def chunk_offsets(self, L):
        chunk = self.chunk_length if self.chunk_length is not None else L
        stride = self.chunk_stride if self.chunk_stride is not None else L
        step, offs, off = chunk - stride, [], 0
        while off < L - step:
            offs.append(off)
            off += stride
        return offs, chunk

    def encode(self, input_values, padding_mask=None, bandwidth=None):
        x = np.asarray(input_values)
        if x.ndim == 2:
            x = x[:, :, None]
        B, L, _ = x.shape
        mask = np.ones((B, L), bool) if padding_mask is None else np.asarray(padding_mask).astype(bool)
        bw = self.cfg.target_bandwidths[0] if bandwidth is None else bandwidth
        n_q = num_quantizers_for_bandwidth(self.cfg, bw)
        offs, chunk = self.chunk_offsets(L)
        codes, scales = [], []
        for o in offs:
            fr, m = np.swapaxes(x[:, o:o + chunk], 1, 2), mask[:, o:o + chunk]
            vals, sc = self.normalise(fr, m)
            y = vals
            for name in self.stage_names()[1:]:
                y = self.stage(name, y)
            codes.append(self.rvq(y, n_q)[0])
            scales.append(sc)
        return np.stack(codes), scales


# ---- the shared end-to-end cases of the CPU and GPU tests (committed seeds)
# oracle.encodec.TINY / TINY_48K with a bandwidth table whose first two entries select 1 and all 3 quantizers: the layer count comes from
# the largest bandwidth at 10 bits a code (EncodecQuantization.swift:81-82), the selection from log2(codebook_size) = 5 bits (:90-97),
# so 3.0 itself asks for 6 quantizers of 3 - an error here, a crash in the reference
BANDWIDTHS = (0.5, 1.5, 3.0)
WIDE = oe.EncodecConfig(num_filters=32, codebook_size=48, codebook_dim=32, hidden_size=32, upsampling_ratios=(3, 2, 2),
                        target_bandwidths=(0.5, 1.7, 3.0), sampling_rate=1200)       # log2(48) = 5.58 bits: 1.7 selects all 3
CONFIGS = {"tiny": replace(oe.TINY, target_bandwidths=BANDWIDTHS), "tiny_48k": replace(oe.TINY_48K, target_bandwidths=BANDWIDTHS), "wide": WIDE}
EXEMPT_CAP = 0.10


def is_normalize(name):
    return name == "tiny_48k"


def row_lengths(cfg):
    hop = cfg.hop_length
    return [9 * hop, hop, 7 * hop - 3, 1]


def audio_rows(cfg, L, rows, seed):
    """[rows, L, channels] float32: band-limited noise with a per-row level"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, L, cfg.audio_channels))
    lvl = 0.1 * (1.0 + np.arange(rows))[:, None, None]
    return (lvl * x).astype(np.float32)


def exempt_mask(gaps, bounds):
    """[B, n_q, F] bool: a frame is exempt from the first quantizer whose top-2 gap falls under the bound"""
    near = gaps < bounds
    return np.cumsum(near, axis=1) > 0
