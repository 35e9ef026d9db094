"""SNAC codec, host mirror of `class SNAC: Module, AudioCodecModel`
(Sources/MLXAudioCodecs/SNAC/SNACDecoder.swift:11-205).  All arithmetic runs in libmi_speech.so."""
from __future__ import annotations

import ctypes as C
import json
import os
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._handle import NativeHandle, _tensor_args  # noqa: F401  (other modules import _tensor_args from here)
from .generation import AudioGenerationError, check


@dataclass
class SNACConfig:
    """SNAC/Config.swift:10-37"""
    sampling_rate: int = 24000
    encoder_dim: int = 48
    encoder_rates: list = field(default_factory=lambda: [2, 4, 8, 8])
    latent_dim: int | None = None
    decoder_dim: int = 1024
    decoder_rates: list = field(default_factory=lambda: [8, 8, 4, 2])
    attn_window_size: int | None = None
    codebook_size: int = 4096
    codebook_dim: int = 8
    vq_strides: list = field(default_factory=lambda: [4, 2, 1])
    noise: bool = True
    depthwise: bool = True

    @classmethod
    def from_dict(cls, d: dict) -> "SNACConfig":
        keys = cls.__dataclass_fields__.keys()
        return cls(**{k: d[k] for k in keys if k in d})

    def to_c(self) -> "_lib.SnacConfigC":
        c = _lib.SnacConfigC()
        c.sampling_rate = self.sampling_rate
        c.latent_dim = self.latent_dim or self.encoder_dim * 2 ** len(self.encoder_rates)
        c.decoder_dim = self.decoder_dim
        c.n_decoder_rates = len(self.decoder_rates)
        for i, r in enumerate(self.decoder_rates):
            c.decoder_rates[i] = r
        c.codebook_size, c.codebook_dim = self.codebook_size, self.codebook_dim
        c.n_codebooks = len(self.vq_strides)
        for i, s in enumerate(self.vq_strides):
            c.vq_strides[i] = s
        c.noise = 1 if self.noise else 0
        c.depthwise = 1 if self.depthwise else 0
        c.attn_window_size = self.attn_window_size or 0
        return c


class SNAC(NativeHandle):
    """AudioCodecModel conformance (AudioCodecModel.swift:15-27): codec_sample_rate, encode_audio (SNACDecoder.swift:120-125, on
    mis_snac_encode; a handle loaded without encoder tensors raises audioEncodingFailed), decode_audio."""

    _prefix = "mis_snac"

    def __init__(self, config: SNACConfig, device: int = 0, _handle=None):
        self.config = config
        self.device = device
        self._h = _handle
        if self._h is None:
            self._create(config.to_c(), device)
        self.sampling_rate = config.sampling_rate
        self.hop_length = int(np.prod(config.encoder_rates))

    # -- loading (SNACDecoder.swift:133-189) ---------------------------------------------------
    @classmethod
    def from_model_directory(cls, model_dir: str, device: int = 0) -> "SNAC":
        with open(os.path.join(model_dir, "config.json")) as f:
            cfg = SNACConfig.from_dict(json.load(f))
        h = C.c_void_p()
        check(_lib.lib().mis_snac_load(model_dir.encode(), device, C.byref(h)))
        return cls(cfg, device, _handle=h)

    @classmethod
    def from_pretrained(cls, model_repo: str, device: int = 0) -> "SNAC":
        """fromPretrained (SNACDecoder.swift:133-154).  No network here: the repo id must resolve to a
        local directory (HF snapshot layout or a plain path)."""
        if os.path.isdir(model_repo):
            return cls.from_model_directory(model_repo, device)
        raise AudioGenerationError(1, f"model repo {model_repo!r} is not a local directory (no network access)")

    @classmethod
    def from_weights(cls, config: SNACConfig, weights: dict, device: int = 0) -> "SNAC":
        m = cls(config, device)
        for name, arr in weights.items():
            m.set_tensor(name, arr)                  # "encoder.*" / "*.in_proj.*" enable the encode path when present
        m.finalize()
        return m

    def set_noise(self, null_noise_is_zero: bool, seed: int = 0):
        check(_lib.lib().mis_snac_set_noise(self._h, 1 if null_noise_is_zero else 0, seed))

    # -- AudioCodecModel -----------------------------------------------------------------------
    @property
    def codec_sample_rate(self) -> float:
        return float(self.sampling_rate)

    def num_samples(self, t_coarse: int) -> int:
        return int(_lib.lib().mis_snac_num_samples(self._h, t_coarse))

    def noise_lengths(self, t_coarse: int):
        return [int(_lib.lib().mis_snac_noise_len(self._h, i, t_coarse)) for i in range(len(self.config.decoder_rates))]

    def decode(self, codes, noise=None) -> np.ndarray:
        """SNAC.decode (SNACDecoder.swift:127-131): list of int arrays [B, T_i] -> float32 [B, 1, N].
        noise: None (policy of set_noise) or one [B, T_i] array per decoder block."""
        codes = [np.ascontiguousarray(c, dtype=np.int32) for c in codes]
        if len(codes) != len(self.config.vq_strides):
            raise AudioGenerationError(3, f"expected {len(self.config.vq_strides)} code arrays")
        if any(c.ndim != 2 for c in codes):
            raise AudioGenerationError(3, "codes must be [batch, time]")
        B, t_coarse = codes[0].shape
        s0 = self.config.vq_strides[0]
        for c, s in zip(codes, self.config.vq_strides):
            if c.shape != (B, t_coarse * (s0 // s)):
                raise AudioGenerationError(3, "code array lengths inconsistent with vq_strides")
        N = self.num_samples(t_coarse)
        out = np.zeros((B, 1, N), np.float32)
        if B == 0 or t_coarse == 0:
            return out
        cptr = (C.c_void_p * len(codes))(*[c.ctypes.data for c in codes])
        nptr = None
        keep = None
        if noise is not None:
            keep = [np.ascontiguousarray(n, dtype=np.float32) for n in noise]
            lens = self.noise_lengths(t_coarse)
            for n, L in zip(keep, lens):
                if n.shape != (B, L):
                    raise AudioGenerationError(3, f"noise shape {n.shape} != {(B, L)}")
            nptr = (C.c_void_p * len(keep))(*[n.ctypes.data for n in keep])
        check(_lib.lib().mis_snac_decode(self._h, cptr, B, t_coarse, nptr, out.ctypes.data))
        return out

    def decode_audio(self, codes) -> np.ndarray:           # decodeAudio, SNACDecoder.swift:201-203
        return self.decode(codes)

    def padded_length(self, n_samples: int) -> int:
        return int(_lib.lib().mis_snac_padded_length(self._h, n_samples))

    def encode(self, audio, return_latent: bool = False):
        """SNAC.encode (SNACDecoder.swift:120-125): audio [B, samples] (or [samples]) -> list of int32 codes [B, T_i]."""
        a = np.ascontiguousarray(audio, dtype=np.float32)
        if a.ndim == 1:
            a = a[None]
        if a.ndim == 3 and a.shape[1] == 1:
            a = np.ascontiguousarray(a[:, 0])
        B, n = a.shape
        Tl = self.padded_length(n) // self.hop_length
        outs = [np.zeros((B, Tl // s), np.int32) for s in self.config.vq_strides]
        ptrs = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
        latent = self.config.latent_dim or self.config.encoder_dim * 2 ** len(self.config.encoder_rates)
        z = np.zeros((B, latent, Tl), np.float32) if return_latent else None
        check(_lib.lib().mis_snac_encode(self._h, a.ctypes.data, B, n, ptrs, z.ctypes.data if return_latent else None))
        return (outs, z) if return_latent else outs

    def encode_audio(self, waveform):                      # encodeAudio, SNACDecoder.swift:197-199
        return self.encode(waveform)

    def debug_tap(self, name: str, batch: int) -> np.ndarray:
        """Intermediate [batch, C, T] of the LAST decode: "zq", "stem_dw", "stem_pw", "block<i>"."""
        cap = 1 << 26
        buf = np.zeros(cap, np.float32)
        ch, ln = C.c_int32(), C.c_int64()
        check(_lib.lib().mis_snac_debug_tap(self._h, name.encode(), buf.ctypes.data, cap, C.byref(ch), C.byref(ln)))
        return buf[: batch * ch.value * ln.value].reshape(batch, ch.value, ln.value).copy()


@dataclass
class DescriptDACConfig:
    """DescriptDACConfig (Sources/MLXAudioCodecs/Descript/DescriptDACConfig.swift:3-34)"""
    encoder_dim: int = 64
    encoder_rates: tuple = (2, 4, 5, 8)
    latent_dim: int | None = None
    decoder_dim: int = 1536
    decoder_rates: tuple = (8, 5, 4, 2)
    n_codebooks: int = 12
    codebook_size: int = 1024
    codebook_dim: int = 8
    sample_rate: int = 16000

    @property
    def resolved_latent(self) -> int:
        return self.latent_dim or self.encoder_dim * 2 ** len(self.encoder_rates)

    def to_c(self) -> "_lib.DacConfigC":
        return _lib.DacConfigC(self.resolved_latent, self.decoder_dim, len(self.decoder_rates), (C.c_int32 * 8)(*self.decoder_rates),
                               self.n_codebooks, self.codebook_size, self.codebook_dim, self.sample_rate)


class DescriptDAC(NativeHandle):
    """class DescriptDAC (Descript/DescriptDAC.swift:172-245,334-352): preprocess / encode / encode_audio / decode_from_codes /
    decode_audio.  The encoder needs the checkpoint's encoder.* and in_proj tensors (error 5 otherwise)."""

    _prefix = "mis_dac"

    def __init__(self, config: DescriptDACConfig, device: int = 0):
        self.config = config
        self._create(config.to_c(), device)

    @classmethod
    def from_weights(cls, config, weights: dict, device: int = 0) -> "DescriptDAC":
        m = cls(config, device)
        for k, v in weights.items():
            m.set_tensor(k, v)
        m.finalize()
        return m

    @property
    def codec_sample_rate(self) -> float:
        return float(self.config.sample_rate)

    def num_samples(self, n_frames: int) -> int:
        return int(_lib.lib().mis_dac_num_samples(self._h, n_frames))

    def decode_from_codes(self, codes) -> np.ndarray:
        """codes int [B, n_codebooks, T] -> waveform float32 [B, num_samples(T)]"""
        cd = np.ascontiguousarray(codes, dtype=np.int32)
        B, ncb, T = cd.shape
        if ncb != self.config.n_codebooks:
            raise AudioGenerationError(3, "wrong number of codebooks")
        out = np.zeros((B, self.num_samples(T)), np.float32)
        check(_lib.lib().mis_dac_decode_codes(self._h, cd.ctypes.data, B, T, out.ctypes.data))
        return out

    def debug_tap(self, codes, block: int) -> np.ndarray:
        cd = np.ascontiguousarray(codes, dtype=np.int32)
        B, ncb, T = cd.shape
        cap = B * self.config.decoder_dim * self.num_samples(T)
        buf = np.zeros(cap, np.float32)
        ch = C.c_int32(); ln = C.c_int64()
        check(_lib.lib().mis_dac_debug_tap(self._h, cd.ctypes.data, B, T, block, buf.ctypes.data, cap, C.byref(ch), C.byref(ln)))
        return buf[: B * ch.value * ln.value].reshape(B, ch.value, ln.value).copy()

    @property
    def hop_length(self) -> int:
        return int(np.prod(self.config.encoder_rates))

    def preprocess(self, audio, sample_rate: int | None = None) -> np.ndarray:
        """DescriptDAC.preprocess (:216-228): right-pad [B, n] to a multiple of the hop length"""
        if sample_rate is not None and sample_rate != self.config.sample_rate:
            raise AudioGenerationError(3, f"Sample rate mismatch: {sample_rate} != {self.config.sample_rate}")
        a = np.ascontiguousarray(audio, dtype=np.float32)
        pad = -a.shape[1] % self.hop_length
        return np.pad(a, ((0, 0), (0, pad))) if pad else a

    def encode(self, audio, n_quantizers: int | None = None, return_latent: bool = False):
        """DescriptDAC.encode (:230-233) on preprocess()ed audio [B, n]: codes int32 [B, nq, n / hop] (+ the encoder output
        [B, latent, T] before the RVQ when return_latent).  Un-padded input is padded as preprocess() does."""
        a = np.ascontiguousarray(audio, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] < 1:
            raise AudioGenerationError(3, "audio must be [batch, samples]")
        B, n = a.shape
        nq = self.config.n_codebooks if n_quantizers is None else int(n_quantizers)
        if not 1 <= nq <= self.config.n_codebooks:
            raise AudioGenerationError(3, "n_quantizers out of range")
        T = int(_lib.lib().mis_dac_padded_length(self._h, n)) // self.hop_length
        if T < 1:
            raise AudioGenerationError(5, "this DAC model was loaded without encoder weights")
        codes = np.zeros((B, nq, T), np.int32)
        z = np.zeros((B, self.config.resolved_latent, T), np.float32) if return_latent else None
        check(_lib.lib().mis_dac_encode(self._h, a.ctypes.data, B, n, nq, codes.ctypes.data, z.ctypes.data if return_latent else None))
        return (codes, z) if return_latent else codes

    def encode_audio(self, waveform) -> dict:
        """AudioCodecModel.encodeAudio (:340-345): {"codes", "original_length"}"""
        w = np.ascontiguousarray(waveform, dtype=np.float32)
        return {"codes": self.encode(self.preprocess(w, self.config.sample_rate)), "original_length": int(w.shape[1])}

    def decode_audio(self, encoded: dict) -> np.ndarray:
        """AudioCodecModel.decodeAudio (:347-350): decode and trim to the original length"""
        return self.decode_from_codes(encoded["codes"])[:, : encoded["original_length"]]


@dataclass
class EncodecConfig:
    """EncodecConfig (Sources/MLXAudioCodecs/Encodec/EncodecConfig.swift:64-89)"""
    audio_channels: int = 1
    num_filters: int = 32
    kernel_size: int = 7
    num_residual_layers: int = 1
    dilation_growth_rate: int = 2
    codebook_size: int = 1024
    codebook_dim: int = 128
    hidden_size: int = 128
    num_lstm_layers: int = 2
    residual_kernel_size: int = 3
    use_causal_conv: bool = True
    pad_mode: str = "reflect"
    norm_type: str = "weight_norm"
    last_kernel_size: int = 7
    trim_right_ratio: float = 1.0
    compress: int = 2
    upsampling_ratios: tuple = (8, 5, 4, 2)
    target_bandwidths: tuple = (1.5, 3.0, 6.0, 12.0, 24.0)
    sampling_rate: int = 24000
    chunk_length_s: float | None = None
    overlap: float | None = None
    use_conv_shortcut: bool = True
    normalize: bool = False

    @classmethod
    def from_dict(cls, d: dict) -> "EncodecConfig":
        """config.json keys of EncodecConfig.swift:37-62 (model_type and keys the reference does not decode are ignored)"""
        kw = {k: d[k] for k in cls.__dataclass_fields__ if k in d}
        for k in ("upsampling_ratios", "target_bandwidths"):
            if k in kw:
                kw[k] = tuple(kw[k])
        return cls(**kw)

    @property
    def hop_length(self) -> int:
        return int(np.prod(self.upsampling_ratios))

    @property
    def frame_rate(self) -> int:                  # EncodecQuantization.swift:78-79
        import math
        return int(math.ceil(self.sampling_rate / self.hop_length))

    @property
    def num_quantizers(self) -> int:              # EncodecQuantization.swift:60-64
        return int(1000 * max(self.target_bandwidths) / (self.frame_rate * 10))

    def num_quantizers_for_bandwidth(self, bandwidth: float | None) -> int:
        """getNumQuantizersForBandwidth (EncodecQuantization.swift:90-97), in the reference's float32"""
        n = self.num_quantizers
        if bandwidth is not None and bandwidth > 0.0:
            bw_per_q = np.float32(np.log2(np.float32(self.codebook_size))) * np.float32(self.frame_rate)
            n = max(1, int(np.floor(np.float32(bandwidth) * np.float32(1000) / bw_per_q)))
        return n

    @property
    def chunk_length(self):                       # Encodec.swift:196-201
        return None if self.chunk_length_s is None else int(self.chunk_length_s * self.sampling_rate)

    @property
    def chunk_stride(self):                       # Encodec.swift:203-208
        if self.chunk_length_s is None or self.overlap is None:
            return None
        return max(1, int((1.0 - self.overlap) * self.chunk_length))

    def to_c(self) -> "_lib.EncodecConfigC":
        if self.norm_type not in ("weight_norm", "time_group_norm"):
            raise AudioGenerationError(3, f"unknown Encodec norm_type {self.norm_type!r}")
        return _lib.EncodecConfigC(self.audio_channels, self.num_filters, self.kernel_size, self.num_residual_layers,
                                   self.dilation_growth_rate, self.codebook_size, self.codebook_dim, self.hidden_size,
                                   self.num_lstm_layers, self.residual_kernel_size, 1 if self.use_causal_conv else 0,
                                   1 if self.pad_mode == "reflect" else 0, self.last_kernel_size, self.compress,
                                   1 if self.use_conv_shortcut else 0, float(self.trim_right_ratio), len(self.upsampling_ratios),
                                   (C.c_int32 * 8)(*self.upsampling_ratios), self.num_quantizers, self.sampling_rate,
                                   1 if self.norm_type == "time_group_norm" else 0, 1 if self.normalize else 0)


@dataclass
class EncodecEncodedAudio:
    """EncodecEncodedAudio (Encodec.swift:441-450): decode needs both the codes [chunks, B, n_q, frames] and the per-chunk scales"""
    codes: np.ndarray
    scales: list


def encodec_expected_shapes(config: EncodecConfig, encoder: bool = True) -> dict:
    """Module-tree key -> shape of an EnCodec checkpoint (EncodecEncoder / EncodecDecoder / EncodecResidualVectorQuantizer,
    Encodec.swift:17-167, EncodecQuantization.swift:75-87; key suffixes of EncodecLayers.swift)."""
    cfg, want = config, {}
    gn = cfg.norm_type == "time_group_norm"

    def conv(p, co, k, ci):
        want[p + ".conv.weight"], want[p + ".conv.bias"] = (co, k, ci), (co,)
        if gn:
            want[p + ".norm.weight"], want[p + ".norm.bias"] = (co,), (co,)

    def resnet(p, dim):
        conv(p + ".block.1", dim // cfg.compress, cfg.residual_kernel_size, dim)
        conv(p + ".block.3", dim, 1, dim // cfg.compress)
        if cfg.use_conv_shortcut:
            conv(p + ".shortcut", dim, 1, dim)

    def lstm(p, dim):
        for j in range(cfg.num_lstm_layers):
            want[f"{p}.lstm.{j}.Wx"], want[f"{p}.lstm.{j}.Wh"], want[f"{p}.lstm.{j}.bias"] = (4 * dim, dim), (4 * dim, dim), (4 * dim,)

    for i in range(cfg.num_quantizers):
        want[f"quantizer.layers.{i}.codebook.embed"] = (cfg.codebook_size, cfg.codebook_dim)
    dim = cfg.num_filters << len(cfg.upsampling_ratios)
    conv("decoder.layers.0", dim, cfg.kernel_size, cfg.hidden_size)
    lstm("decoder.layers.1", dim)
    li = 2
    for ratio in cfg.upsampling_ratios:
        conv(f"decoder.layers.{li + 1}", dim // 2, 2 * ratio, dim)
        li, dim = li + 2, dim // 2
        for _ in range(cfg.num_residual_layers):
            resnet(f"decoder.layers.{li}", dim)
            li += 1
    conv(f"decoder.layers.{li + 1}", cfg.audio_channels, cfg.last_kernel_size, dim)
    if encoder:
        dim = cfg.num_filters
        conv("encoder.layers.0", dim, cfg.kernel_size, cfg.audio_channels)
        li = 1
        for ratio in reversed(cfg.upsampling_ratios):
            for _ in range(cfg.num_residual_layers):
                resnet(f"encoder.layers.{li}", dim)
                li += 1
            conv(f"encoder.layers.{li + 1}", 2 * dim, 2 * ratio, dim)
            li, dim = li + 2, 2 * dim
        lstm(f"encoder.layers.{li}", dim)
        conv(f"encoder.layers.{li + 2}", cfg.hidden_size, cfg.last_kernel_size, dim)
    return want


def preprocess_encodec_audio(raw_audio, sampling_rate: int = 24000, chunk_length: int | None = None, chunk_stride: int | None = None):
    """preprocessEncodecAudio (Encodec.swift:478-515): a list of [L] or [L, channels] waveforms -> (inputs float32 [B, max_length,
    channels], masks bool [B, max_length]), right-padded with zeros; with chunking max_length grows by chunk - (max_length % stride)."""
    audio = [np.asarray(x, np.float32) for x in raw_audio]
    audio = [x[:, None] if x.ndim == 1 else x for x in audio]
    max_length = max((x.shape[0] for x in audio), default=0)
    if chunk_length is not None and chunk_stride is not None:
        max_length += chunk_length - (max_length % chunk_stride)
    inputs = np.zeros((len(audio), max_length, audio[0].shape[1] if audio else 1), np.float32)
    masks = np.zeros((len(audio), max_length), bool)
    for i, x in enumerate(audio):
        inputs[i, : x.shape[0]] = x
        masks[i, : x.shape[0]] = True
    return inputs, masks


class Encodec(NativeHandle):
    """class Encodec (Encodec/Encodec.swift:172-465): encode(input_values, padding_mask, bandwidth) / decode(audio_codes, audio_scales)
    and the AudioCodecModel surface encode_audio / decode_audio / reconstruct; the 24 kHz (mono, causal, plain convs) and the 48 kHz
    (stereo, non-causal, GroupNorm, normalize, chunked) model families.  Loaders: from_weights, from_model_directory / from_pretrained
    (config.json + model.safetensors, unknown keys rejected), synthetic.  Encoding needs the checkpoint's encoder.* tensors (error 5
    otherwise)."""

    _prefix = "mis_encodec"

    def __init__(self, config: EncodecConfig, device: int = 0):
        self.config = config
        self._create(config.to_c(), device)

    @classmethod
    def from_weights(cls, config, weights: dict, device: int = 0) -> "Encodec":
        m = cls(config, device)
        for k, v in weights.items():
            m.set_tensor(k, v)
        m.finalize()
        return m

    @classmethod
    def from_model_directory(cls, model_dir: str, device: int = 0) -> "Encodec":
        """fromModelDirectory (Encodec.swift:423-438): config.json + model.safetensors; a key the model does not have is an error
        (verify: .noUnusedKeys).  The encoder tensors may be absent as a whole (a decoder-only export)."""
        path = os.path.join(model_dir, "config.json")
        if not os.path.exists(path):
            raise AudioGenerationError(1, f"Encodec: config.json not found in {model_dir!r}")
        with open(path) as f:
            cfg = EncodecConfig.from_dict(json.load(f))
        wpath = os.path.join(model_dir, "model.safetensors")
        if not os.path.exists(wpath):
            raise AudioGenerationError(1, f"Encodec: model.safetensors not found in {model_dir!r}")
        from safetensors import safe_open
        with safe_open(wpath, framework="pt") as sf:
            weights = {k: sf.get_tensor(k) for k in sf.keys()}
        unused = sorted(set(weights) - set(encodec_expected_shapes(cfg)))
        if unused:
            raise AudioGenerationError(3, f"Encodec checkpoint: unused keys {unused[:4]}")
        return cls.from_weights(cfg, weights, device)

    @classmethod
    def from_pretrained(cls, path_or_repo: str, device: int = 0) -> "Encodec":
        """fromPretrained (Encodec.swift:402-421).  No network here: the repo id must resolve to a local directory."""
        if os.path.isdir(path_or_repo):
            return cls.from_model_directory(path_or_repo, device)
        raise AudioGenerationError(1, f"model repo {path_or_repo!r} is not a local directory (no network access)")

    @classmethod
    def synthetic(cls, config: EncodecConfig, seed: int = 909, device: int = 0) -> "Encodec":
        """A full model (encoder, decoder, codebooks) with mis-synth-v1 weights in checkpoint order (measurement tools)."""
        from .synthetic import encodec_synthetic_weights
        return cls.from_weights(config, encodec_synthetic_weights(config, seed), device)

    @property
    def codec_sample_rate(self) -> float:
        return float(self.config.sampling_rate)

    @property
    def has_encoder(self) -> bool:
        return bool(_lib.lib().mis_encodec_has_encoder(self._h))

    def num_frames(self, length: int) -> int:
        """frames of `length` samples: a ceil per strided conv of the encoder"""
        return int(_lib.lib().mis_encodec_encode_num_frames(self._h, int(length)))

    def encode_rows(self, rows, masks=None, n_q: int | None = None):
        """encodeFrame (Encodec.swift:212-238) of independent rows: rows float32 [R, L, channels], masks bool [R, L] or None ->
        (codes int32 [R, n_q, frames], scales float32 [R] or None without config.normalize).  One device pass."""
        a = np.ascontiguousarray(np.transpose(np.asarray(rows, np.float32), (0, 2, 1)))            # [R, channels, L]
        R, ch, L = a.shape
        if ch != self.config.audio_channels:
            raise AudioGenerationError(3, f"Encodec: {ch} input channels, the model has {self.config.audio_channels}")
        if self.config.chunk_length_s is not None and L / self.config.sampling_rate > 1e-5 + self.config.chunk_length_s:
            raise AudioGenerationError(3, f"Duration of frame ({L / self.config.sampling_rate}) is longer than chunk {self.config.chunk_length_s}")
        nq = self.config.num_quantizers if n_q is None else int(n_q)
        if not 1 <= nq <= self.config.num_quantizers:
            raise AudioGenerationError(3, f"{nq} quantizers asked of a model with {self.config.num_quantizers}")
        m = None if masks is None else np.ascontiguousarray(np.asarray(masks).astype(np.uint8))
        codes = np.zeros((R, nq, self.num_frames(L)), np.int32)
        scales = np.zeros(R, np.float32) if self.config.normalize else None
        check(_lib.lib().mis_encodec_encode_frame(self._h, a.ctypes.data, None if m is None else m.ctypes.data, R, L, nq, codes.ctypes.data,
                                                  None if scales is None else scales.ctypes.data))
        return codes, scales

    def encode(self, input_values, padding_mask=None, bandwidth: float | None = None):
        """encode (Encodec.swift:248-291): input_values [B, L, channels] (or [B, L]) -> (codes int32 [chunks, B, n_q, frames], scales:
        one float32 [B] per chunk, or None without config.normalize).  Chunks are independent, so all of them go through one device pass."""
        cfg = self.config
        bw = cfg.target_bandwidths[0] if bandwidth is None else bandwidth
        if bw not in cfg.target_bandwidths:
            raise AudioGenerationError(3, f"This model doesn't support bandwidth {bw}. Select one of {list(cfg.target_bandwidths)}")
        x = np.asarray(input_values, np.float32)
        if x.ndim == 2:
            x = x[:, :, None]
        if x.ndim != 3:
            raise AudioGenerationError(3, "input_values must be [batch, samples, channels]")
        B, L, ch = x.shape
        if not 1 <= ch <= 2:
            raise AudioGenerationError(3, f"Number of audio channels must be 1 or 2, but got {ch}")
        chunk_len = cfg.chunk_length if cfg.chunk_length is not None else L
        stride = cfg.chunk_stride if cfg.chunk_stride is not None else L
        mask = np.ones((B, L), bool) if padding_mask is None else np.asarray(padding_mask).astype(bool)
        step = chunk_len - stride
        offsets, offset = [], 0
        while offset < L - step:
            offsets.append(offset)
            offset += stride
        if not offsets:
            raise AudioGenerationError(3, "input shorter than one chunk step")
        lens = {min(L, o + chunk_len) - o for o in offsets}
        if len(lens) != 1:                                                    # stacked(encodedFrames) needs equal frame counts
            raise AudioGenerationError(3, "chunks of unequal length: pad the input with preprocess_encodec_audio")
        n = lens.pop()
        rows = np.stack([x[:, o:o + n] for o in offsets]).reshape(len(offsets) * B, n, ch)
        masks = np.stack([mask[:, o:o + n] for o in offsets]).reshape(len(offsets) * B, n)
        codes, scales = self.encode_rows(rows, masks, cfg.num_quantizers_for_bandwidth(bw))
        codes = codes.reshape(len(offsets), B, codes.shape[1], codes.shape[2])
        return codes, [None if scales is None else scales[i * B:(i + 1) * B].copy() for i in range(len(offsets))]

    def encode_audio(self, waveform) -> EncodecEncodedAudio:
        """AudioCodecModel.encodeAudio (Encodec.swift:457-460)"""
        codes, scales = self.encode(waveform)
        return EncodecEncodedAudio(codes, scales)

    def decode_audio(self, encoded: EncodecEncodedAudio) -> np.ndarray:
        """AudioCodecModel.decodeAudio (Encodec.swift:462-464)"""
        return self.decode(encoded.codes, encoded.scales)

    def reconstruct(self, waveform) -> np.ndarray:
        """AudioCodecModel.reconstruct: decode_audio(encode_audio(waveform)), cut to the input's length"""
        n = np.asarray(waveform).shape[1]
        return self.decode_audio(self.encode_audio(waveform))[..., :n]

    def encode_tap(self, rows, stage: int, masks=None) -> np.ndarray:
        """Stage output of the encode chain on rows [R, L, channels] -> [R, C, T'] (mis_debug_encodec_encode_tap)"""
        a = np.ascontiguousarray(np.transpose(np.asarray(rows, np.float32), (0, 2, 1)))
        R, ch, L = a.shape
        m = None if masks is None else np.ascontiguousarray(np.asarray(masks).astype(np.uint8))
        cap = R * max(self.config.num_filters << len(self.config.upsampling_ratios), self.config.hidden_size, ch) * (L + 8)
        buf = np.zeros(cap, np.float32)
        cch = C.c_int32(); ln = C.c_int64()
        check(_lib.lib().mis_debug_encodec_encode_tap(self._h, a.ctypes.data, None if m is None else m.ctypes.data, R, L, 0, stage,
                                                      buf.ctypes.data, cap, None, C.byref(cch), C.byref(ln)))
        return buf[: R * cch.value * ln.value].reshape(R, cch.value, ln.value).copy()

    def rvq_tap(self, embeddings, n_q: int):
        """ONE launch of the residual-VQ search on embeddings [R, D, F] -> (codes int32 [R, n_q, F], residuals float32 [n_q + 1, R, D, F])"""
        e = np.ascontiguousarray(embeddings, dtype=np.float32)
        R, D, F = e.shape
        if D != self.config.codebook_dim:
            raise AudioGenerationError(3, "embeddings must be [rows, codebook_dim, frames]")
        codes = np.zeros((R, n_q, F), np.int32)
        res = np.zeros((n_q + 1, R, D, F), np.float32)
        cch = C.c_int32(); ln = C.c_int64()
        check(_lib.lib().mis_debug_encodec_encode_tap(self._h, e.ctypes.data, None, R, F, n_q, -1, res.ctypes.data, res.size, codes.ctypes.data,
                                                      C.byref(cch), C.byref(ln)))
        return codes, res

    def decode_frame(self, codes, scale=None) -> np.ndarray:
        """decodeFrame (Encodec.swift:295-302): codes int [B, n_q, T] -> [B, T * hop] (mono) or [B, channels, T * hop]"""
        cd = np.ascontiguousarray(codes, dtype=np.int32)
        B, nq, T = cd.shape
        ch = self.config.audio_channels
        out = np.zeros((B, T * self.config.hop_length) if ch == 1 else (B, ch, T * self.config.hop_length), np.float32)
        sc = None if scale is None else np.ascontiguousarray(np.broadcast_to(np.asarray(scale, np.float32).reshape(-1), (B,)))
        check(_lib.lib().mis_encodec_decode_frame(self._h, cd.ctypes.data, B, nq, T, None if sc is None else sc.ctypes.data,
                                                  out.ctypes.data))
        return out

    @staticmethod
    def linear_overlap_add(frames, hop_stride: int) -> np.ndarray:
        """Encodec.linearOverlapAdd (Encodec.swift:304-355); host arithmetic in the reference as well."""
        L = frames[0].shape[1]
        total = hop_stride * (len(frames) - 1) + frames[-1].shape[1]
        tv = (np.arange(L, dtype=np.float32) + np.float32(1)) / np.float32(L + 1)
        wv = (np.float32(0.5) - np.abs(tv - np.float32(0.5))).astype(np.float32)
        out = np.zeros((frames[0].shape[0], total), np.float32)
        sw = np.zeros(total, np.float32)
        off = 0
        for f in frames:
            n = f.shape[1]
            out[:, off:off + n] += wv[:n] * f
            sw[off:off + n] += wv[:n]
            off += hop_stride
        nz = sw != 0
        out[:, nz] /= sw[nz]
        return out

    def _overlap_add(self, frames, hop_stride: int) -> np.ndarray:
        if frames[0].ndim == 2:
            return self.linear_overlap_add(frames, hop_stride)
        B, ch = frames[0].shape[:2]                          # stereo: the time axis is the last one; channels ride along as rows
        out = self.linear_overlap_add([f.reshape(B * ch, f.shape[-1]) for f in frames], hop_stride)
        return out.reshape(B, ch, -1)

    def decode(self, audio_codes, audio_scales=None, padding_mask=None) -> np.ndarray:
        """decode (Encodec.swift:357-398): audio_codes [n_chunks, B, n_q, frames] -> [B, samples]"""
        ac = np.asarray(audio_codes)
        scales = audio_scales if audio_scales is not None else [None] * ac.shape[0]
        if self.config.chunk_length is None:
            if ac.shape[0] != 1:
                raise AudioGenerationError(3, f"Expected one frame, got {ac.shape[0]}")
            out = self.decode_frame(ac[0], scales[0])
        else:
            out = self._overlap_add([self.decode_frame(ac[i], scales[i]) for i in range(ac.shape[0])], self.config.chunk_stride or 1)
        if padding_mask is not None and np.asarray(padding_mask).shape[1] < out.shape[-1]:
            out = out[..., : np.asarray(padding_mask).shape[1]]
        return out

    def debug_tap(self, codes, stage: int) -> np.ndarray:
        cd = np.ascontiguousarray(codes, dtype=np.int32)
        B, nq, T = cd.shape
        cap = B * max(self.config.num_filters << len(self.config.upsampling_ratios), 4) * (T + 8) * self.config.hop_length
        buf = np.zeros(cap, np.float32)
        ch = C.c_int32(); ln = C.c_int64()
        check(_lib.lib().mis_encodec_debug_tap(self._h, cd.ctypes.data, B, nq, T, stage, buf.ctypes.data, cap, C.byref(ch), C.byref(ln)))
        return buf[: B * ch.value * ln.value].reshape(B, ch.value, ln.value).copy()


# ---------------------------------------------------------------------------------------------------------------------------------
# Mimi (Sources/MLXAudioCodecs/Mimi/)
@dataclass
class MimiConfig:
    """MimiConfig with the mimi_202407 defaults (Mimi.swift:47-99)."""
    num_codebooks: int = 32
    channels: int = 1
    sample_rate: int = 24000
    frame_rate: float = 12.5
    dimension: int = 512
    n_filters: int = 64
    n_residual_layers: int = 1
    ratios: list = field(default_factory=lambda: [8, 6, 5, 4])
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
    norm_eps: float = 1e-5
    bins: int = 2048
    quantizer_dim: int = 256

    @property
    def stride(self) -> int:                          # downsampleStride (Mimi.swift:125-126)
        return int(self.sample_rate / float(np.prod(self.ratios)) / self.frame_rate)

    @property
    def samples_per_frame(self) -> int:
        return self.stride * int(np.prod(self.ratios))

    def to_c(self) -> "_lib.MimiConfigC":
        c = _lib.MimiConfigC()
        c.channels, c.sample_rate, c.frame_rate = self.channels, self.sample_rate, self.frame_rate
        c.dimension, c.n_filters, c.n_residual_layers = self.dimension, self.n_filters, self.n_residual_layers
        c.n_ratios = len(self.ratios)
        for i, r in enumerate(self.ratios):
            c.ratios[i] = r
        c.kernel_size, c.residual_kernel_size, c.last_kernel_size = self.kernel_size, self.residual_kernel_size, self.last_kernel_size
        c.dilation_base, c.compress = self.dilation_base, self.compress
        c.num_layers, c.num_heads, c.dim_feedforward, c.context = self.num_layers, self.num_heads, self.dim_feedforward, self.context
        c.max_period, c.norm_eps = self.max_period, self.norm_eps
        c.num_quantizers, c.bins, c.quantizer_dim = self.num_codebooks, self.bins, self.quantizer_dim
        return c


def _swap(v, a: int, b: int):
    return v.transpose(a, b) if hasattr(v, "detach") else np.swapaxes(v, a, b)


def _permute(v, axes):
    return v.permute(*axes) if hasattr(v, "detach") else np.transpose(v, axes)


def mimi_sanitize(key: str, arr):
    """Mimi.sanitize (Mimi.swift:337-415) for one raw Kyutai (PyTorch) tensor -> (post-sanitize key, array in the MLX layout)."""
    k = ".".join(seg[1:] if seg.startswith("_") else seg for seg in key.split("."))
    if k.startswith("encoder.model."):
        k = k.replace("encoder.model.", "encoder.")
    if k.startswith("decoder.model."):
        k = k.replace("decoder.model.", "decoder.")
    if k.endswith(".in_proj_weight"):
        k = k.replace(".in_proj_weight", ".in_proj.weight")
    if k.endswith(".linear1.weight"):
        k = k.replace(".linear1.weight", ".gating.linear1.weight")
    if k.endswith(".linear2.weight"):
        k = k.replace(".linear2.weight", ".gating.linear2.weight")
    for li, di in enumerate((2, 5, 8, 11)):
        k = k.replace(f"decoder.{di}.", f"decoder.layers.{li}.upsample.")
        k = k.replace(f"decoder.{di + 1}.", f"decoder.layers.{li}.residuals.0.")
    for li, ei in enumerate((1, 4, 7, 10)):
        k = k.replace(f"encoder.{ei}.", f"encoder.layers.{li}.residuals.0.")
        k = k.replace(f"encoder.{ei + 2}.", f"encoder.layers.{li}.downsample.")
    k = k.replace("decoder.0.", "decoder.init_conv1d.")
    k = k.replace("decoder.14.", "decoder.final_conv1d.")
    k = k.replace("encoder.0.", "encoder.init_conv1d.")
    k = k.replace("encoder.14.", "encoder.final_conv1d.")
    k = k.replace(".block.1.", ".block.0.")
    k = k.replace(".block.3.", ".block.1.")
    v = arr
    if (k.endswith(".conv.weight") or k.endswith(".output_proj.weight") or k.endswith(".input_proj.weight")) and v.ndim >= 2:
        v = _swap(v, v.ndim - 1, v.ndim - 2)
    if k.endswith(".convtr.weight") and v.ndim == 3:
        v = _swap(v, 1, 2) if v.shape[1] == 1 else _permute(v, (1, 2, 0))   # depthwise [C, 1, k] -> [C, k, 1]; [in, out, k] -> [out, k, in]
    return k, v


class Mimi(NativeHandle):
    """extension Mimi: AudioCodecModel (Mimi.swift:426-437): codec_sample_rate, frame_rate, encode / encode_audio, decode /
    decode_audio; loaders from_weights (post-sanitize names), from_model_directory / from_pretrained (raw Kyutai safetensors through
    mimi_sanitize; local directories only) and synthetic.  Weights are computed in float32 whatever their stored dtype."""

    _prefix = "mis_mimi"

    def __init__(self, config: MimiConfig | None = None, device: int = 0):
        self.config = config or MimiConfig()
        self._create(self.config.to_c(), device)

    # -- loading -----------------------------------------------------------------------------------
    @classmethod
    def from_weights(cls, config: MimiConfig, weights: dict, device: int = 0) -> "Mimi":
        m = cls(config, device)
        for k, v in weights.items():
            m.set_tensor(k, v)
        m.finalize()
        return m

    @classmethod
    def from_model_directory(cls, model_dir: str, config: MimiConfig | None = None, device: int = 0) -> "Mimi":
        """Every *.safetensors of the directory (name order; the reference reads tokenizer-e351c8d8-checkpoint125.safetensors) through
        mimi_sanitize."""
        from .qwen3tts import read_safetensors
        files = sorted(f for f in os.listdir(model_dir) if f.endswith(".safetensors"))
        if not files:
            raise AudioGenerationError(1, f"no .safetensors file in {model_dir!r}")
        m = cls(config, device)
        for fn in files:
            for k, v in read_safetensors(os.path.join(model_dir, fn)).items():
                if isinstance(v, np.ndarray):
                    continue                                             # integer bookkeeping tensors
                m.set_tensor(*mimi_sanitize(k, v))
        m.finalize()
        return m

    @classmethod
    def from_pretrained(cls, repo_id: str, config: MimiConfig | None = None, device: int = 0) -> "Mimi":
        """fromPretrained (Mimi.swift:235-335): a local directory only (no network access)."""
        if os.path.isdir(repo_id):
            return cls.from_model_directory(repo_id, config, device)
        raise AudioGenerationError(1, f"model repo {repo_id!r} is not a local directory (no network access)")

    @classmethod
    def synthetic(cls, config: MimiConfig | None = None, seed: int = 77, device: int = 0) -> "Mimi":
        from .synthetic import mimi_synthetic_weights
        config = config or MimiConfig()
        return cls.from_weights(config, mimi_synthetic_weights(config, seed), device)

    # -- AudioCodecModel -----------------------------------------------------------------------------
    @property
    def codec_sample_rate(self) -> float:
        return float(self.config.sample_rate)

    @property
    def frame_rate(self) -> float:
        return float(self.config.frame_rate)

    def num_samples(self, n_frames: int) -> int:
        return int(_lib.lib().mis_mimi_num_samples(self._h, n_frames))

    def decode(self, codes) -> np.ndarray:
        """Mimi.decode: codes [B, n_q, T] (or [n_q, T]) -> pcm float32 [B, 1, T * 1920]."""
        cd = np.ascontiguousarray(np.asarray(codes), dtype=np.int32)
        if cd.ndim == 2:
            cd = cd[None]
        B, nq, T = cd.shape
        out = np.empty((B, 1, self.num_samples(T)), np.float32)
        check(_lib.lib().mis_mimi_decode(self._h, cd.ctypes.data, B, nq, T, out.ctypes.data))
        return out

    def decode_audio(self, codes) -> np.ndarray:
        return self.decode(codes)

    def encode_num_frames(self, n_samples: int) -> int:
        return int(_lib.lib().mis_mimi_encode_num_frames(self._h, n_samples))

    def encode(self, audio, n_q: int | None = None) -> np.ndarray:
        """Mimi.encode: audio [B, 1, n] (or [B, n] / [n]) -> codes int32 [B, n_q, frames]."""
        a = np.ascontiguousarray(np.asarray(audio, np.float32))
        a = a.reshape(1, -1) if a.ndim == 1 else a.reshape(a.shape[0], -1)
        B, n = a.shape
        nq = self.config.num_codebooks if n_q is None else int(n_q)
        out = np.empty((B, nq, self.encode_num_frames(n)), np.int32)
        check(_lib.lib().mis_mimi_encode(self._h, a.ctypes.data, B, n, nq, out.ctypes.data))
        return out

    def encode_audio(self, waveform) -> np.ndarray:
        return self.encode(waveform)

    def debug_tap(self, codes, stage: int) -> np.ndarray:
        cd = np.ascontiguousarray(np.asarray(codes), dtype=np.int32)
        B, nq, T = cd.shape
        cap = B * max(self.config.dim_feedforward, 3 * self.config.dimension, self.config.n_filters << len(self.config.ratios)) * \
            self.num_samples(T)
        buf = np.empty(cap, np.float32)
        ch, ln = C.c_int32(), C.c_int64()
        check(_lib.lib().mis_debug_mimi_decoder_tap(self._h, cd.ctypes.data, B, nq, T, stage, buf.ctypes.data, cap, C.byref(ch), C.byref(ln)))
        return buf[: B * ch.value * ln.value].reshape(B, ch.value, ln.value).copy()


class MimiStreamingDecoder:
    """MimiStreamingDecoder (Mimi.swift:207-232): reset() and decode_frames(codes [B, n_q, T] or [n_q, T]) -> pcm [B, 1, T * 1920]; the
    state of every row is kept across calls, a call of several frames equals the same frames one call at a time."""

    def __init__(self, mimi: Mimi, batch: int = 1):
        self.mimi, self.batch = mimi, batch
        self.reset()

    def reset(self):
        check(_lib.lib().mis_mimi_decode_stream_begin(self.mimi._h, self.batch))

    def decode_frames(self, codes) -> np.ndarray:
        cd = np.ascontiguousarray(np.asarray(codes), dtype=np.int32)
        if cd.ndim == 2:
            cd = cd[None]
        B, nq, T = cd.shape
        if B != self.batch:
            raise AudioGenerationError(3, f"stream has {self.batch} rows, got {B}")
        out = np.empty((B, 1, T * self.mimi.num_samples(1)), np.float32)
        check(_lib.lib().mis_mimi_decode_stream_step(self.mimi._h, cd.ctypes.data, nq, T, out.ctypes.data))
        return out


# ------------------------------------------------------------------------------------------------------------ BigVGAN
@dataclass
class BigVGANConfig:
    """BigVGANConfig (BigVGANConfig.swift:13-65): the eleven fields under their coding keys, resblock as "1" / "2", activation as
    "snake" / "snakebeta".  max_batch / max_frames size the engine's workspace (rows a call, mel frames a row)."""
    num_mels: int
    upsample_rates: list
    upsample_kernel_sizes: list
    upsample_initial_channel: int
    resblock: str
    resblock_kernel_sizes: list
    resblock_dilation_sizes: list
    activation: str
    snake_logscale: bool
    use_bias_at_final: bool = True
    use_tanh_at_final: bool = True
    max_batch: int = 8
    max_frames: int = 1024

    _KEYS = ("num_mels", "upsample_rates", "upsample_kernel_sizes", "upsample_initial_channel", "resblock", "resblock_kernel_sizes",
             "resblock_dilation_sizes", "activation", "snake_logscale")

    def __post_init__(self):
        self.resblock = str(self.resblock)
        if self.resblock not in ("1", "2"):
            raise AudioGenerationError(3, f"BigVGAN: resblock {self.resblock!r} (\"1\" or \"2\")")
        if self.activation not in ("snake", "snakebeta"):
            raise AudioGenerationError(3, f"BigVGAN: activation {self.activation!r} (\"snake\" or \"snakebeta\")")

    @classmethod
    def from_dict(cls, d: dict, **workspace) -> "BigVGANConfig":
        missing = [k for k in cls._KEYS if k not in d]
        if missing:
            raise AudioGenerationError(3, f"BigVGAN: config misses {missing}")
        kw = {k: d[k] for k in cls._KEYS}
        for k in ("use_bias_at_final", "use_tanh_at_final"):
            if k in d:
                kw[k] = bool(d[k])
        return cls(**kw, **workspace)

    @property
    def hop_length(self) -> int:
        return int(np.prod(self.upsample_rates, dtype=np.int64))

    def to_c(self) -> "_lib.BigVGANConfigC":
        c = _lib.BigVGANConfigC()
        if (len(self.upsample_rates) > 8 or len(self.upsample_kernel_sizes) > 8 or len(self.resblock_kernel_sizes) > 8
                or len(self.resblock_dilation_sizes) != len(self.resblock_kernel_sizes) or any(len(d) > 8 for d in self.resblock_dilation_sizes)):
            raise AudioGenerationError(3, "BigVGAN: at most 8 stages, 8 resblock kernels with a dilation list each, 8 dilations a block")
        c.num_mels, c.upsample_initial_channel = self.num_mels, self.upsample_initial_channel
        c.n_upsamples, c.n_upsample_kernel_sizes = len(self.upsample_rates), len(self.upsample_kernel_sizes)
        for i, v in enumerate(self.upsample_rates):
            c.upsample_rates[i] = v
        for i, v in enumerate(self.upsample_kernel_sizes):
            c.upsample_kernel_sizes[i] = v
        c.resblock, c.n_resblock_kernels = int(self.resblock), len(self.resblock_kernel_sizes)
        for i, (k, dil) in enumerate(zip(self.resblock_kernel_sizes, self.resblock_dilation_sizes)):
            c.resblock_kernel_sizes[i], c.n_resblock_dilations[i] = k, len(dil)
            for j, v in enumerate(dil):
                c.resblock_dilation_sizes[i][j] = v
        c.activation, c.snake_logscale = int(self.activation == "snakebeta"), int(self.snake_logscale)
        c.use_bias_at_final, c.use_tanh_at_final = int(self.use_bias_at_final), int(self.use_tanh_at_final)
        c.max_batch, c.max_frames = self.max_batch, self.max_frames
        return c


def bigvgan_expected_shapes(config: BigVGANConfig) -> dict:
    """name -> shape of every parameter of BigVGAN(config) in the reference's (MLX) layouts: conv weight_v [out, k, in] with weight_g
    [out, 1, 1], transposed conv weight_v [out, k, in] with weight_g [1, 1, in] (BigVGANLayers.swift:113-225); act.beta only for
    snakebeta; conv_post.bias only with use_bias_at_final."""
    s = {}

    def conv(p, out, k, cin, bias=True):
        s[p + ".weight_g"], s[p + ".weight_v"] = (out, 1, 1), (out, k, cin)
        if bias:
            s[p + ".bias"] = (out,)

    def act(p, ch):
        s[p + ".act.alpha"] = (ch,)
        if config.activation == "snakebeta":
            s[p + ".act.beta"] = (ch,)

    c0, nk = config.upsample_initial_channel, len(config.resblock_kernel_sizes)
    conv("conv_pre", c0, 7, config.num_mels)
    for i, (rate, ks) in enumerate(zip(config.upsample_rates, config.upsample_kernel_sizes)):
        cin, ch = c0 >> i, c0 >> (i + 1)
        u = f"ups.{i}.0"
        s[u + ".weight_g"], s[u + ".weight_v"], s[u + ".bias"] = (1, 1, cin), (ch, ks, cin), (ch,)
        for j, (k, dil) in enumerate(zip(config.resblock_kernel_sizes, config.resblock_dilation_sizes)):
            q = f"resblocks.{i * nk + j}"
            for d in range(len(dil)):
                if config.resblock == "1":
                    conv(f"{q}.convs1.{d}", ch, k, ch)
                    conv(f"{q}.convs2.{d}", ch, k, ch)
                    act(f"{q}.activations.{2 * d}", ch)
                    act(f"{q}.activations.{2 * d + 1}", ch)
                else:
                    conv(f"{q}.convs.{d}", ch, k, ch)
                    act(f"{q}.activations.{d}", ch)
    cf = c0 >> len(config.upsample_rates)
    act("activation_post", cf)
    conv("conv_post", 1, 7, cf, config.use_bias_at_final)
    return s


def bigvgan_sanitize(config: BigVGANConfig, weights: dict) -> dict:
    """BigVGAN.sanitize (BigVGAN.swift:190-217): num_batches_tracked keys are dropped; a 3-D conv / ups. tensor whose shape differs from
    the parameter's is transposed - ups. with (1, 2, 0) (torch [in, out, k] -> [out, k, in]), any other conv with (0, 2, 1) (torch
    [out, in, k] -> [out, k, in]); a tensor that already has the expected shape, and a key the model does not have, pass untouched."""
    want = bigvgan_expected_shapes(config)
    out = {}
    for key, v in weights.items():
        if "num_batches_tracked" in key:
            continue
        if key in want and ("conv" in key or "ups." in key) and v.ndim == 3 and tuple(v.shape) != want[key]:
            v = _permute(v, (1, 2, 0)) if "ups." in key else _permute(v, (0, 2, 1))
        out[key] = v
    return out


class BigVGAN(NativeHandle):
    """BigVGAN (BigVGAN.swift:92-228): a mel -> waveform vocoder, extension BigVGAN: AudioDecoderModel.  __call__ / decode_audio take
    [B, num_mels, T] and return [B, 1, T hop]; decode takes a ragged batch with per-row frame counts.  Loaders: from_weights
    (sanitized names, all of them and no others), from_model_directory (config.json + *.safetensors through sanitize), synthetic."""
    _prefix = "mis_bigvgan"

    def __init__(self, config: BigVGANConfig, device: int = 0):
        self.config = config
        self.device = device
        self._create(config.to_c(), device)

    @classmethod
    def from_weights(cls, config: BigVGANConfig, weights: dict, device: int = 0) -> "BigVGAN":
        want = bigvgan_expected_shapes(config)
        unknown, missing = sorted(set(weights) - set(want)), sorted(set(want) - set(weights))
        if unknown or missing:
            raise AudioGenerationError(3, f"BigVGAN checkpoint: unexpected keys {unknown[:4]}, missing keys {missing[:4]}")
        m = cls(config, device)
        for name, arr in weights.items():
            m.set_tensor(name, arr)
        m.finalize()
        return m

    @classmethod
    def from_model_directory(cls, model_dir: str, device: int = 0, **workspace) -> "BigVGAN":
        from ._handle import read_safetensors_dir
        path = os.path.join(model_dir, "config.json")
        if not os.path.exists(path):
            raise AudioGenerationError(3, "BigVGAN: config.json not found in model directory")
        with open(path) as f:
            cfg = BigVGANConfig.from_dict(json.load(f), **workspace)
        weights = read_safetensors_dir(model_dir, missing_code=(3, "BigVGAN: no .safetensors file in model directory"))
        return cls.from_weights(cfg, bigvgan_sanitize(cfg, weights), device)

    @classmethod
    def synthetic(cls, config: BigVGANConfig, device: int = 0, seed: int = 777) -> "BigVGAN":
        m = cls(config, device)
        check(_lib.lib().mis_bigvgan_init_synthetic(m._h, seed))
        m.finalize()
        return m

    def sanitize(self, weights: dict) -> dict:
        return bigvgan_sanitize(self.config, weights)

    # -- AudioDecoderModel ---------------------------------------------------------------------------
    @property
    def codec_sample_rate(self):
        return None                                                      # BigVGAN.swift:223

    @property
    def hop_length(self) -> int:
        return int(_lib.lib().mis_bigvgan_hop(self._h))

    def num_samples(self, frames: int) -> int:
        return int(frames) * self.hop_length

    @property
    def launches(self) -> int:
        return int(_lib.lib().mis_bigvgan_launches(self._h))

    def decode(self, mel, frames=None) -> np.ndarray:
        """mel [B, num_mels, T] (or [num_mels, T]) with frames[B] valid frames a row (None: T) -> waveform [B, T hop]; the columns
        behind a row's own frames[b] hop samples are zero."""
        m = np.ascontiguousarray(mel, dtype=np.float32)
        if m.ndim == 2:
            m = m[None]
        if m.ndim != 3 or m.shape[1] != self.config.num_mels:
            raise AudioGenerationError(3, f"BigVGAN: mel of shape {m.shape}, expected [batch, {self.config.num_mels}, frames]")
        B, _, T = m.shape
        fr = None if frames is None else np.ascontiguousarray(frames, dtype=np.int32)
        if fr is not None and fr.shape != (B,):
            raise AudioGenerationError(3, "BigVGAN: one frame count per batch row is expected")
        out = np.zeros((B, T * self.hop_length), np.float32)
        check(_lib.lib().mis_bigvgan_decode(self._h, m.ctypes.data, None if fr is None else fr.ctypes.data, B, T, out.ctypes.data))
        return out

    def __call__(self, mel) -> np.ndarray:
        """callAsFunction (BigVGAN.swift:169-188): [B, num_mels, T] -> [B, 1, T hop]."""
        return self.decode(mel)[:, None, :]

    def decode_audio(self, mel) -> np.ndarray:
        return self(mel)

    def debug_tap(self, stage: int) -> np.ndarray:
        """Tensors of the last call [B, C, length]: 0 conv_pre; with n = num_kernels, 1 + i (n + 2) stage i's transposed conv, + 1 + j its
        AMP block j, + n + 1 the stage mean; 1 + stages (n + 2) activation_post."""
        dims = (C.c_int64 * 3)()
        check(_lib.lib().mis_bigvgan_tap(self._h, stage, None, 0, dims))
        out = np.zeros(tuple(int(d) for d in dims), np.float32)
        check(_lib.lib().mis_bigvgan_tap(self._h, stage, out.ctypes.data, out.size, dims))
        return out

    def timing(self) -> float:
        """Device milliseconds of the last decode's kernels."""
        ms = (C.c_float * 1)()
        check(_lib.lib().mis_debug_bigvgan_timing(self._h, ms))
        return float(ms[0])


def bigvgan_aa_act(x, counts, alpha, beta, device: int = 0) -> np.ndarray:
    """One launch of the anti-aliased activation kernel (tests): x [B, C, T], counts[B], alpha / beta [C] as the activation uses them."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, Cn, T = x.shape
    cn, al, be = (np.ascontiguousarray(counts, dtype=np.int32), np.ascontiguousarray(alpha, dtype=np.float32),
                  np.ascontiguousarray(beta, dtype=np.float32))
    if cn.shape != (B,) or al.shape != (Cn,) or be.shape != (Cn,):
        raise AudioGenerationError(3, "BigVGAN: counts [B] and alpha / beta [C] are expected")
    out = np.zeros_like(x)
    check(_lib.lib().mis_debug_bigvgan_aa_act(device, x.ctypes.data, cn.ctypes.data, B, Cn, T, al.ctypes.data, be.ctypes.data, out.ctypes.data))
    return out
