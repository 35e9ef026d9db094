"""Mimi decoder and per-frame streaming decoder: CPU restatement of the reference, for the tests.  The device side is
csrc/mimi.hip; the encoder half is oracle/mimi_encoder.py (reused read-only, with its synthetic-weight conventions).

Follows Mimi.decode (Sources/MLXAudioCodecs/Mimi/Mimi.swift:178-186) and MimiStreamingDecoder.decodeFrames (:207-232, one decodeStep
:196-204 per frame): SplitResidualVectorQuantizer.decode (Quantization.swift: codebook = embedding_sum / max(cluster_usage, 1e-5),
codebook 0 behind rvq_first.output_proj, the sum of the others behind rvq_rest.output_proj), ConvTrUpsample1d (Conv.swift:349-362,
depthwise transposed conv k = 2s, no bias, causal right trim), the decoder transformer (Transformer.swift:110-314: LayerNorm eps 1e-5,
fused in_proj, interleaved RoPE at the cache offset, the cache trim to t + min(context, kLen - t) keys, MLX's bottom-right causal mask,
layer scale, exact-GELU MLP) and SeanetDecoder (Seanet.swift:259-356).  The stream restates the step functions literally:
StreamableConv1d.step (Conv.swift:225-262: left zero pad on the first call, carried tail) and StreamableConvTranspose1d.step
(:305-330: overlap-add of the carried tail after subtracting the bias).  Layout [B, C, T]; conv weights [out, k, in] (MLX)."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as TF

from oracle import mimi_encoder as om

F = np.float32


@dataclass
class MimiRefConfig:                              # mimi_202407 (Mimi.swift:47-99)
    dimension: int = 512
    n_filters: int = 64
    n_residual_layers: int = 1
    ratios: tuple = (8, 6, 5, 4)
    kernel_size: int = 7
    residual_kernel_size: int = 3
    last_kernel_size: int = 3
    dilation_base: int = 2
    compress: int = 2
    num_layers: int = 8
    num_heads: int = 8
    dim_feedforward: int = 2048
    context: int = 250
    max_period: float = 10000.0
    num_quantizers: int = 32
    bins: int = 2048
    quantizer_dim: int = 256
    sample_rate: int = 24000
    frame_rate: float = 12.5

    @property
    def stride(self) -> int:                      # Mimi.swift:125-126
        return int(self.sample_rate / float(np.prod(self.ratios)) / self.frame_rate)

    @property
    def samples_per_frame(self) -> int:
        return self.stride * int(np.prod(self.ratios))

    def encoder_config(self) -> om.MimiEncoderConfig:
        return om.MimiEncoderConfig(num_filters=self.n_filters, kernel_size=self.kernel_size, last_kernel_size=self.last_kernel_size,
                                    residual_kernel_size=self.residual_kernel_size, num_residual_layers=self.n_residual_layers,
                                    dilation_growth_rate=self.dilation_base, compress=self.compress, upsampling_ratios=tuple(self.ratios),
                                    hidden_size=self.dimension, num_hidden_layers=self.num_layers, num_attention_heads=self.num_heads,
                                    intermediate_size=self.dim_feedforward, rope_theta=self.max_period, sliding_window=self.context,
                                    sampling_rate=self.sample_rate, frame_rate=self.frame_rate, codebook_dim=self.quantizer_dim,
                                    codebook_size=self.bins, num_quantizers=self.num_quantizers, valid_num_quantizers=self.num_quantizers)


MIMI = MimiRefConfig()
TINY = MimiRefConfig(dimension=32, n_filters=4, ratios=(3, 2), num_layers=2, num_heads=2, dim_feedforward=64, num_quantizers=8, bins=64,
                     quantizer_dim=8, sample_rate=240, frame_rate=20.0)


def make_synthetic_weights(cfg: MimiRefConfig, seed: int = 77) -> dict:
    """Post-sanitize MLX names: the encoder half of oracle/mimi_encoder.make_synthetic_weights (quantizer codebooks included), plus the
    decoder half drawn from the same generator on a disjoint key range."""
    from oracle import synth
    W = om.make_synthetic_weights(cfg.encoder_config(), seed=seed)
    key = [seed * 100000 + 50000]

    def t(shape, amp):
        key[0] += 1
        return synth.synth_tensor(key[0], shape, amp)

    def conv(p, co, k, ci, gain=1.0):
        W[p + ".weight"] = t((co, k, ci), gain * math.sqrt(3.0 / (k * ci)))
        W[p + ".bias"] = t((co,), 0.05)
    D, qd = cfg.dimension, cfg.quantizer_dim
    for grp in ("rvq_first", "rvq_rest"):
        W[f"quantizer.{grp}.output_proj.weight"] = t((D, 1, qd), math.sqrt(3.0 / qd))
    s = cfg.stride
    W["upsample.convtr.convtr.convtr.weight"] = t((D, 2 * s, 1), 0.8)
    for li in range(cfg.num_layers):
        p = f"decoder_transformer.transformer.layers.{li}"
        for n in ("norm1", "norm2"):
            W[f"{p}.{n}.weight"] = (1.0 + t((D,), 0.2)).astype(F)
            W[f"{p}.{n}.bias"] = t((D,), 0.1)
        W[p + ".self_attn.in_proj.weight"] = t((3 * D, D), math.sqrt(3.0 / D))
        W[p + ".self_attn.out_proj.weight"] = t((D, D), math.sqrt(3.0 / D))
        W[p + ".gating.linear1.weight"] = t((cfg.dim_feedforward, D), math.sqrt(3.0 / D))
        W[p + ".gating.linear2.weight"] = t((D, cfg.dim_feedforward), math.sqrt(3.0 / cfg.dim_feedforward))
        W[p + ".layer_scale_1.scale"] = (0.3 + t((D,), 0.1)).astype(F)
        W[p + ".layer_scale_2.scale"] = (0.3 + t((D,), 0.1)).astype(F)
    mult = 1 << len(cfg.ratios)
    conv("decoder.init_conv1d.conv.conv", mult * cfg.n_filters, cfg.kernel_size, D, gain=1.3)
    for li, r in enumerate(cfg.ratios):
        p = f"decoder.layers.{li}"
        cin = mult * cfg.n_filters
        cout = cin // 2
        conv(p + ".upsample.convtr.convtr", cout, 2 * r, cin, gain=1.3 * math.sqrt(r))
        for ri in range(cfg.n_residual_layers):
            q = f"{p}.residuals.{ri}"
            conv(q + ".block.0.conv.conv", cout // cfg.compress, cfg.residual_kernel_size, cout, gain=1.3)
            conv(q + ".block.1.conv.conv", cout, 1, cout // cfg.compress, gain=0.7)
        mult //= 2
    conv("decoder.final_conv1d.conv.conv", 1, cfg.last_kernel_size, cfg.n_filters, gain=1.0)
    return W


def synthetic_codes(cfg: MimiRefConfig, batch: int, n_q: int, T: int, seed: int = 5) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, cfg.bins, size=(batch, n_q, T)).astype(np.int32)


class _ConvStep:                                  # StreamableConv1d.step, stride 1 (Conv.swift:225-262)
    def __init__(self):
        self.prev, self.padded = None, False

    def __call__(self, x, w, b, k, dil):
        keff = (k - 1) * dil + 1
        if not self.padded:
            self.padded = True
            x = TF.pad(x, (keff - 1, 0))
        if self.prev is not None:
            x = torch.cat([self.prev, x], dim=2)
        nframes = max(x.shape[2] + 1 - keff, 0)
        if nframes == 0:
            self.prev = x
            return x[:, :0]
        self.prev = x[:, :, nframes:]
        return TF.conv1d(x[:, :, :nframes - 1 + keff], w, b, dilation=dil)


class _ConvTrStep:                                # StreamableConvTranspose1d.step (Conv.swift:305-330)
    def __init__(self):
        self.prev = None

    def __call__(self, x, w, b, stride, k, groups=1):
        y = TF.conv_transpose1d(x, w, b, stride=stride, groups=groups)
        if self.prev is not None:
            prev = self.prev if b is None else self.prev - b[None, :, None]
            pt = prev.shape[2]
            y = torch.cat([y[:, :, :pt] + prev, y[:, :, pt:]], dim=2)
        ot, invalid = y.shape[2], k - stride
        self.prev = y[:, :, ot - invalid:]
        return y[:, :, :ot - invalid]


class MimiDecoderRef:
    def __init__(self, cfg: MimiRefConfig, weights: dict):
        self.cfg = cfg
        self.w = {k: torch.as_tensor(np.asarray(v, F)) for k, v in weights.items()}
        self._pt = {}

    def _conv_w(self, p):                         # [out, k, in] -> PyTorch [out, in, k]
        return self.w[p + ".weight"].permute(0, 2, 1).contiguous()

    def _convtr_w(self, p):                       # [out, k, in / groups] -> PyTorch [in, out / groups, k]
        w = self.w[p + ".weight"]
        return w.permute(0, 2, 1).contiguous() if w.shape[2] == 1 else w.permute(2, 0, 1).contiguous()

    # -- SplitResidualVectorQuantizer.decode
    def rvq_decode(self, codes):
        codes = torch.as_tensor(np.asarray(codes, np.int64))
        n_q = codes.shape[1]
        assert 2 <= n_q <= self.cfg.num_quantizers

        def emb(grp, i):
            q = f"quantizer.{grp}.vq.layers.{i}.codebook"
            return self.w[q + ".embedding_sum"] / torch.clamp(self.w[q + ".cluster_usage"], min=1e-5)[:, None]
        first = emb("rvq_first", 0)[codes[:, 0]]                                          # [B, T, d]
        rest = sum(emb("rvq_rest", i - 1)[codes[:, i]] for i in range(1, n_q))
        out = []
        for grp, z in (("rvq_first", first), ("rvq_rest", rest)):
            out.append(TF.conv1d(z.transpose(1, 2), self._conv_w(f"quantizer.{grp}.output_proj")))
        return out[0] + out[1]

    # -- Attention / TransformerLayer with a KV cache (Transformer.swift:136-314); caches: per layer [K, V] lists or None
    def transformer(self, x, caches, offset):
        cfg = self.cfg
        h = x.transpose(1, 2)
        B, t, D = h.shape
        H, hd = cfg.num_heads, D // cfg.num_heads
        pos = torch.arange(offset, offset + t, dtype=torch.float32)
        inv = 1.0 / (cfg.max_period ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
        ang = pos[:, None] * inv[None, :]
        cos, sin = torch.cos(ang), torch.sin(ang)

        def rope(a):
            a1, a2 = a[..., 0::2], a[..., 1::2]
            return torch.stack([a1 * cos - a2 * sin, a1 * sin + a2 * cos], dim=-1).reshape(a.shape)
        for li in range(cfg.num_layers):
            p = f"decoder_transformer.transformer.layers.{li}"
            n1 = TF.layer_norm(h, (D,), self.w[p + ".norm1.weight"], self.w[p + ".norm1.bias"], 1e-5)
            qkv = (n1 @ self.w[p + ".self_attn.in_proj.weight"].T).reshape(B, t, 3, H, hd)
            q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
            q, k = rope(q), rope(k)
            if caches is not None:
                if caches[li] is not None:
                    k = torch.cat([caches[li][0], k], dim=2)
                    v = torch.cat([caches[li][1], v], dim=2)
                caches[li] = (k, v)
            kl = k.shape[2]
            kt = t + min(cfg.context, kl - t)
            k, v = k[:, :, kl - kt:], v[:, :, kl - kt:]
            # bottom-right causal: query i sees keys j <= kt - t + i
            mask = torch.full((t, kt), float("-inf")).triu(kt - t + 1)
            sc = (q @ k.transpose(-1, -2)) / math.sqrt(hd) + mask
            o = (torch.softmax(sc, dim=-1) @ v).transpose(1, 2).reshape(B, t, D)
            h = h + (o @ self.w[p + ".self_attn.out_proj.weight"].T) * self.w[p + ".layer_scale_1.scale"]
            n2 = TF.layer_norm(h, (D,), self.w[p + ".norm2.weight"], self.w[p + ".norm2.bias"], 1e-5)
            m = TF.gelu(n2 @ self.w[p + ".gating.linear1.weight"].T) @ self.w[p + ".gating.linear2.weight"].T
            h = h + m * self.w[p + ".layer_scale_2.scale"]
        return h.transpose(1, 2)

    def _causal(self, x, p, k, dil=1):
        return TF.conv1d(TF.pad(x, ((k - 1) * dil, 0)), self._conv_w(p), self.w[p + ".bias"], dilation=dil)

    def _convtr(self, x, p, stride, groups=1, bias=True):
        y = TF.conv_transpose1d(x, self._convtr_w(p), self.w[p + ".bias"] if bias else None, stride=stride, groups=groups)
        return y[:, :, : y.shape[2] - stride] if y.shape[2] else y          # k = 2 stride: right trim k - stride

    def decode(self, codes, stop: str | None = None):
        """codes [B, n_q, T] -> pcm [B, 1, T * samples_per_frame] (Mimi.decode).  stop: return an intermediate stage."""
        cfg = self.cfg
        with torch.no_grad():
            x = self.rvq_decode(codes)
            if stop == "rvq":
                return x.numpy()
            x = self._convtr(x, "upsample.convtr.convtr.convtr", cfg.stride, groups=cfg.dimension, bias=False)
            if stop == "upsample":
                return x.numpy()
            x = self.transformer(x, [None] * cfg.num_layers, 0)
            if stop == "transformer":
                return x.numpy()
            x = self._causal(x, "decoder.init_conv1d.conv.conv", cfg.kernel_size)
            if stop == "init":
                return x.numpy()
            for li, r in enumerate(cfg.ratios):
                p = f"decoder.layers.{li}"
                x = self._convtr(TF.elu(x), p + ".upsample.convtr.convtr", r)
                dil = 1
                for ri in range(cfg.n_residual_layers):
                    q = f"{p}.residuals.{ri}"
                    h = self._causal(TF.elu(x), q + ".block.0.conv.conv", cfg.residual_kernel_size, dil)
                    x = x + self._causal(TF.elu(h), q + ".block.1.conv.conv", 1)
                    dil *= cfg.dilation_base
                if stop == f"layer{li}":
                    return x.numpy()
            return self._causal(TF.elu(x), "decoder.final_conv1d.conv.conv", cfg.last_kernel_size).numpy()

    def stream(self, codes) -> np.ndarray:
        """decodeFrames: codes [B, n_q, T] -> pcm [B, 1, T * samples_per_frame], one decodeStep per frame from a reset state."""
        cfg = self.cfg
        nl = len(cfg.ratios)
        up = _ConvTrStep()
        init = _ConvStep()
        cts = [_ConvTrStep() for _ in range(nl)]
        res = [[(_ConvStep(), _ConvStep()) for _ in range(cfg.n_residual_layers)] for _ in range(nl)]
        fin = _ConvStep()
        caches = [None] * cfg.num_layers
        codes = np.asarray(codes)
        out = []
        with torch.no_grad():
            for f in range(codes.shape[2]):
                x = self.rvq_decode(codes[:, :, f:f + 1])
                x = up(x, self._convtr_w("upsample.convtr.convtr.convtr"), None, cfg.stride, 2 * cfg.stride, groups=cfg.dimension)
                x = self.transformer(x, caches, f * cfg.stride)
                p = "decoder.init_conv1d.conv.conv"
                x = init(x, self._conv_w(p), self.w[p + ".bias"], cfg.kernel_size, 1)
                for li, r in enumerate(cfg.ratios):
                    p = f"decoder.layers.{li}.upsample.convtr.convtr"
                    x = cts[li](TF.elu(x), self._convtr_w(p), self.w[p + ".bias"], r, 2 * r)
                    dil = 1
                    for ri in range(cfg.n_residual_layers):
                        q = f"decoder.layers.{li}.residuals.{ri}"
                        a, b = res[li][ri]
                        h = a(TF.elu(x), self._conv_w(q + ".block.0.conv.conv"), self.w[q + ".block.0.conv.conv.bias"],
                              cfg.residual_kernel_size, dil)
                        x = x + b(TF.elu(h), self._conv_w(q + ".block.1.conv.conv"), self.w[q + ".block.1.conv.conv.bias"], 1, 1)
                        dil *= cfg.dilation_base
                p = "decoder.final_conv1d.conv.conv"
                out.append(fin(TF.elu(x), self._conv_w(p), self.w[p + ".bias"], cfg.last_kernel_size, 1))
        return torch.cat(out, dim=2).numpy()


def first_divergent_frame(cfg: MimiRefConfig) -> int:
    """The first frame whose step sees fewer keys than the whole-sequence decode: s*f - context > 0."""
    return cfg.context // cfg.stride + 1
