"""MossFormer2-SE and DeepFilterNet speech enhancement, host mirrors of `MossFormer2SEModel` (Sources/MLXAudioSTS/Models/MossFormer2SE),
`DeepFilterNetModel` (Sources/MLXAudioSTS/Models/DeepFilterNet; csrc/deepfilternet.hip) and of the
`STS.loadModel` factory (Sources/MLXAudioSTS/STSModel.swift).  Configuration, checkpoint loading and the ragged-batch packing stay on
the host; the Kaldi-style fbank + deltas, the mask network and the STFT / inverse STFT run in libmi_speech.so (csrc/mossformer2.hip)."""
from __future__ import annotations

import ctypes as C
import json
import os
from dataclasses import dataclass, fields

import numpy as np

from . import _lib
from ._handle import NativeHandle, pack_rows
from .generation import AudioGenerationError, check

_F = np.float32
_PREFIX = "model.mossformer."
_GROUP, _QK, _INNER, _FF_TAPS, _FSMN_TAPS = 256, 128, 256, 17, 39     # constants of the reference, not configuration


class MossFormer2SEError(AudioGenerationError):
    """MossFormer2SEError (MossFormer2Model.swift:232-253): `.sts_case` is invalidAudioShape, missingSafetensors or duplicateWeightKey.
    The reference's fourth case, missingMask, cannot be reached here: the engine either returns a mask or fails with a status."""

    def __init__(self, sts_case: str, message: str):
        self.sts_case = sts_case
        super().__init__(3, message)


class STSModelError(AudioGenerationError):
    """STSModelError.unsupportedModelType (STSModel.swift:34-48)."""

    def __init__(self, model_type):
        self.model_type = model_type
        super().__init__(3, f"Unsupported STS model type: {model_type!r}")


_CONFIG_KEYS = ("model_type", "sample_rate", "win_len", "win_inc", "fft_len", "num_mels", "win_type", "preemphasis", "in_channels",
                "out_channels", "out_channels_final", "num_blocks", "one_time_decode_length", "decode_window", "chunk_seconds",
                "chunk_overlap", "auto_chunk_threshold", "quantization_config")


@dataclass
class MossFormer2SEConfig:
    """MossFormer2SEConfig (MossFormer2Config.swift): every field, default and JSON key, the chunk fields the reference's enhance never
    reads included.  max_batch / max_seconds size the engine's workspace and are not part of a checkpoint."""
    model_type: str = "mossformer2_se"
    sample_rate: int = 48000
    win_len: int = 1920
    win_inc: int = 384
    fft_len: int = 1920
    num_mels: int = 60
    win_type: str = "hamming"
    preemphasis: float = 0.97
    in_channels: int = 180
    out_channels: int = 512
    out_channels_final: int = 961
    num_blocks: int = 24
    one_time_decode_length: int = 20
    decode_window: int = 4
    chunk_seconds: float = 4.0
    chunk_overlap: float = 0.25
    auto_chunk_threshold: float = 60.0
    quantization_config: dict | None = None
    max_batch: int = 8
    max_seconds: float = 60.0

    @classmethod
    def from_dict(cls, d: dict, **workspace) -> "MossFormer2SEConfig":
        """init(from:): missing or null keys take the defaults, unknown keys are ignored; quantization_config's own keys default to
        bits 4, group_size 64."""
        kw = {k: d[k] for k in _CONFIG_KEYS if d.get(k) is not None}
        if "quantization_config" in kw:
            q = kw["quantization_config"]
            kw["quantization_config"] = {"bits": int(q.get("bits", 4) if q.get("bits") is not None else 4),
                                         "group_size": int(q.get("group_size", 64) if q.get("group_size") is not None else 64)}
        return cls(**kw, **workspace)

    @property
    def max_samples(self) -> int:
        return max(int(self.win_len), int(round(self.max_seconds * self.sample_rate)))

    def to_c(self) -> "_lib.MossFormer2ConfigC":
        if self.quantization_config is not None:
            raise AudioGenerationError(3, "MossFormer2-SE: quantised checkpoints (quantization_config) are not served")
        return _lib.MossFormer2ConfigC(self.sample_rate, self.win_len, self.win_inc, self.fft_len, self.num_mels,
                                       1 if "hann" in self.win_type.lower() else 0, self.in_channels, self.out_channels,
                                       self.out_channels_final, self.num_blocks, self.max_batch, float(self.preemphasis), self.max_samples)


def mossformer2_normalized_key(key: str) -> str:
    """normalizedWeightKey (:267-279): `module.` is stripped, then `mossformer.` becomes `model.mossformer.`."""
    if key.startswith("module."):
        key = key[len("module."):]
    if key.startswith("mossformer."):
        key = "model." + key
    return key


def mossformer2_sanitize(weights: dict) -> dict:
    """sanitize (:281-290)."""
    return {mossformer2_normalized_key(k): v for k, v in weights.items()}


def mossformer2_expected_shapes(config: MossFormer2SEConfig) -> dict:
    """name -> shape of every parameter of MossFormer2SE(config): what update(parameters:verify: .all) accepts."""
    D, Ci, Fo, I, Q = config.out_channels, config.in_channels, config.out_channels_final, _INNER, _QK
    s = {"norm.weight": (Ci, 1), "norm.bias": (Ci, 1), "conv1d_encoder.weight": (D, 1, Ci), "pos_enc.scale": (1,), "pos_enc.inv_freq": (D // 2,)}

    def ffconvm(p, dout, din, scalenorm):
        if scalenorm:
            s[p + ".norm.g"] = (1,)
        else:
            s[p + ".norm.weight"], s[p + ".norm.bias"] = (din,), (din,)
        s[p + ".linear.weight"], s[p + ".linear.bias"] = (dout, din), (dout,)
        s[p + ".conv_module.weight"] = (dout, _FF_TAPS, 1)

    for i in range(config.num_blocks):
        q = f"mdl.intra_mdl.mossformerM.layers.{i}"
        ffconvm(q + ".to_hidden", 4 * D, D, True)
        ffconvm(q + ".to_qk", Q, D, True)
        ffconvm(q + ".to_out", D, 2 * D, True)
        s[q + ".qk_offset_scale.gamma"], s[q + ".qk_offset_scale.beta"] = (4, Q), (4, Q)
        f = f"mdl.intra_mdl.mossformerM.fsmn.{i}"
        s[f + ".conv1.weight"], s[f + ".conv1.bias"] = (I, 1, D), (I,)
        s[f + ".prelu.weight"] = ()
        for n in ("norm1", "norm2"):
            s[f"{f}.{n}.weight"], s[f"{f}.{n}.bias"] = (I,), (I,)
        ffconvm(f + ".gated_fsmn.to_u", I, I, False)
        ffconvm(f + ".gated_fsmn.to_v", I, I, False)
        s[f + ".gated_fsmn.fsmn.linear.weight"], s[f + ".gated_fsmn.fsmn.linear.bias"] = (I, I), (I,)
        s[f + ".gated_fsmn.fsmn.project.weight"] = (I, I)
        s[f + ".gated_fsmn.fsmn.conv1.weight"] = (I, _FSMN_TAPS, 1, 1)
        s[f + ".conv2.weight"], s[f + ".conv2.bias"] = (D, 1, I), (D,)
    for n in ("mdl.intra_mdl.norm", "mdl.intra_norm"):
        s[n + ".weight"], s[n + ".bias"] = (D,), (D,)
    s["conv1d_out.weight"], s["conv1d_out.bias"] = (2 * D, 1, D), (2 * D,)
    s["conv1_decoder.weight"] = (Fo, 1, D)
    s["prelu.weight"] = ()
    for n in ("output", "output_gate"):
        s[n + ".weight"], s[n + ".bias"] = (D, 1, D), (D,)
    return {_PREFIX + k: v for k, v in s.items()}


def mossformer2_check_weights(config: MossFormer2SEConfig, weights: dict):
    """weights: sanitized names.  Every expected key with its shape, and no other key."""
    if any(k.endswith(".scales") for k in weights):
        raise AudioGenerationError(3, "MossFormer2-SE: quantised checkpoints (.scales tensors) are not served")
    want = mossformer2_expected_shapes(config)
    unknown, missing = sorted(set(weights) - set(want)), sorted(set(want) - set(weights))
    if unknown or missing:
        raise AudioGenerationError(3, f"MossFormer2-SE checkpoint: unexpected keys {unknown[:4]}, missing keys {missing[:4]}")
    bad = [k for k in want if tuple(weights[k].shape) != want[k]]
    if bad:
        raise AudioGenerationError(3, f"MossFormer2-SE checkpoint: {bad[0]} has shape {tuple(weights[bad[0]].shape)}, expected {want[bad[0]]}")


def _read_config(model_dir: str, policy: str, **workspace) -> MossFormer2SEConfig:
    """loadConfig (:302-318).  policy "read_error": the defaults when config.json cannot be read (missing or unreadable); "missing":
    the defaults only when the file does not exist.  A file that was read must decode."""
    path = os.path.join(model_dir, "config.json")
    if policy == "read_error":
        try:
            with open(path, "rb") as f:
                data = f.read()
        except OSError:
            return MossFormer2SEConfig(**workspace)
    else:
        if not os.path.exists(path):
            return MossFormer2SEConfig(**workspace)
        with open(path, "rb") as f:
            data = f.read()
    return MossFormer2SEConfig.from_dict(json.loads(data), **workspace)


def _read_weights(model_dir: str, fail_on_duplicate: bool) -> dict:
    """loadWeights (:320-349): every *.safetensors (extension in any case) in name order.  Overwrite policy: a later file's key
    replaces an earlier one.  Fail policy: a key whose normalised form was seen before is an error."""
    files = sorted(fn for fn in os.listdir(model_dir) if fn.lower().endswith(".safetensors"))
    if not files:
        raise MossFormer2SEError("missingSafetensors", f"No .safetensors files found in {model_dir}")
    from safetensors import safe_open
    weights, seen = {}, set()
    for fn in files:
        with safe_open(os.path.join(model_dir, fn), framework="pt") as sf:
            for k in sf.keys():
                if fail_on_duplicate:
                    n = mossformer2_normalized_key(k)
                    if n in seen:
                        raise MossFormer2SEError("duplicateWeightKey",
                                                 f"Duplicate normalized weight key detected while loading local safetensors: {n}")
                    seen.add(n)
                weights[k] = sf.get_tensor(k)
    return weights


class MossFormer2SE(NativeHandle):
    """enhance / callAsFunction of the reference model, plus ragged batches: one handle, 1..max_batch rows a call, each at most
    max_seconds long."""
    _prefix = "mis_mossformer2"

    def __init__(self, config: MossFormer2SEConfig, device: int = 0):
        self.config = config
        self.device = device
        self._create(config.to_c(), device)

    @property
    def sample_rate(self) -> int:
        return self.config.sample_rate

    @classmethod
    def from_weights(cls, config: MossFormer2SEConfig, weights: dict, device: int = 0) -> "MossFormer2SE":
        """weights: sanitized names (what mossformer2_sanitize returns), all of them and no others."""
        config.to_c()
        mossformer2_check_weights(config, weights)
        m = cls(config, device)
        for name, arr in weights.items():
            m.set_tensor(name[len(_PREFIX):], arr.reshape(1) if tuple(arr.shape) == () else arr)
        m.finalize()
        return m

    @classmethod
    def synthetic(cls, config: MossFormer2SEConfig, device: int = 0, seed: int = 777) -> "MossFormer2SE":
        m = cls(config, device)
        check(_lib.lib().mis_mossformer2_init_synthetic(m._h, seed))
        m.finalize()
        return m

    @classmethod
    def from_model_directory(cls, model_dir: str, device: int = 0, **workspace) -> "MossFormer2SE":
        """fromDirectory (:383-387): default config when config.json cannot be read, later files overwrite earlier ones."""
        cfg = _read_config(model_dir, "read_error", **workspace)
        return cls.from_weights(cfg, mossformer2_sanitize(_read_weights(model_dir, False)), device)

    @classmethod
    def from_local(cls, model_dir: str, device: int = 0, **workspace) -> "MossFormer2SE":
        """fromLocal (:389-393): default config only when config.json is missing, a duplicate normalised key is an error."""
        cfg = _read_config(model_dir, "missing", **workspace)
        return cls.from_weights(cfg, mossformer2_sanitize(_read_weights(model_dir, True)), device)

    sanitize = staticmethod(mossformer2_sanitize)

    @property
    def launches(self) -> int:
        return int(_lib.lib().mis_mossformer2_launches(self._h))

    # -- inputs --------------------------------------------------------------------------------------
    def _row(self, audio, sample_rate) -> np.ndarray:
        a = np.asarray(audio)
        if a.ndim != 1:
            raise MossFormer2SEError("invalidAudioShape", f"Expected a 1D waveform, got shape {list(a.shape)}")
        a = a.astype(_F, copy=False)
        rate = self.config.sample_rate
        if sample_rate is not None and int(sample_rate) != rate:
            raise AudioGenerationError(3, f"MossFormer2-SE: audio at {sample_rate} Hz, the model takes {rate} Hz; this package has no "
                                          "resampler - resample before the call")
        if len(a) > self.config.max_samples:
            raise AudioGenerationError(3, f"MossFormer2-SE: a row of {len(a)} samples, the workspace holds {self.config.max_samples} "
                                          "(max_seconds)")
        return a

    def _pack(self, waveforms, sample_rate, junk):
        rows = [self._row(w, sample_rate) for w in waveforms]
        if not rows:
            raise AudioGenerationError(3, "MossFormer2-SE: no rows")
        pcm, lens = pack_rows(rows, junk)
        return pcm, lens, *pcm.shape

    def frames(self, lens):
        """Sample counts -> (frames T, output samples), int32 / int64 arrays."""
        lens = np.ascontiguousarray(lens, np.int64)
        T, n = np.zeros(len(lens), np.int32), np.zeros(len(lens), np.int64)
        check(_lib.lib().mis_mossformer2_frames(self._h, lens.ctypes.data, len(lens), T.ctypes.data, n.ctypes.data))
        return T, n

    # -- calls ---------------------------------------------------------------------------------------
    def features_raw(self, waveforms, sample_rate=None, junk: float | None = None):
        """Ragged list of waveforms -> (features [B, Tmax, 3 num_mels], T [B])."""
        pcm, lens, B, stride = self._pack(waveforms, sample_rate, junk)
        T, _ = self.frames(lens)
        out = np.zeros((B, max(1, int(T.max())), self.config.in_channels), _F)
        check(_lib.lib().mis_mossformer2_features(self._h, pcm.ctypes.data, lens.ctypes.data, B, stride, out.ctypes.data, out.shape[1]))
        return out[:, : int(T.max())], T

    def mask_raw(self, waveforms, sample_rate=None, junk: float | None = None):
        """Ragged list of waveforms -> (mask [B, Tmax, out_channels_final], T [B])."""
        pcm, lens, B, stride = self._pack(waveforms, sample_rate, junk)
        T, _ = self.frames(lens)
        out = np.zeros((B, max(1, int(T.max())), self.config.out_channels_final), _F)
        check(_lib.lib().mis_mossformer2_mask(self._h, pcm.ctypes.data, lens.ctypes.data, B, stride, out.ctypes.data, out.shape[1]))
        return out[:, : int(T.max())], T

    def forward_features(self, features, counts=None) -> np.ndarray:
        """features [T, in_channels] or [B, T, in_channels], counts[B] valid rows each (None: T) -> mask [B, T, out_channels_final]."""
        f = np.ascontiguousarray(features, dtype=_F)
        if f.ndim == 2:
            f = f[None]
        if f.ndim != 3 or f.shape[2] != self.config.in_channels:
            raise AudioGenerationError(3, f"MossFormer2-SE: features of shape {f.shape}, expected [batch, rows, {self.config.in_channels}]")
        B, R = f.shape[0], f.shape[1]
        cn = None if counts is None else np.ascontiguousarray(counts, dtype=np.int32)
        if cn is not None and cn.shape != (B,):
            raise AudioGenerationError(3, "MossFormer2-SE: one row count per batch row is expected")
        out = np.zeros((B, R, self.config.out_channels_final), _F)
        if R == 0:
            return out
        check(_lib.lib().mis_mossformer2_mask_features(self._h, f.ctypes.data, None if cn is None else cn.ctypes.data, B, R, out.ctypes.data))
        return out

    def __call__(self, features, counts=None) -> np.ndarray:
        """callAsFunction (:227-229): features [batch, time, in_channels] -> the mask [batch, time, out_channels_final]."""
        return self.forward_features(features, counts)

    def _waves(self, fn, waveforms, sample_rate, junk, *extra):
        pcm, lens, B, stride = self._pack(waveforms, sample_rate, junk)
        T, n = self.frames(lens)
        out, got = np.zeros((B, max(1, int(n.max()))), _F), np.zeros(B, np.int64)
        check(fn(self._h, pcm.ctypes.data, lens.ctypes.data, B, stride, *extra, out.ctypes.data, out.shape[1], got.ctypes.data))
        return [out[b, : int(got[b])].copy() for b in range(B)]

    def enhance_batch(self, waveforms, sample_rate=None, dither: float = 0.0, junk: float | None = None) -> list:
        """enhance for a ragged batch: one float32 array of (T - 1) win_inc + min(win_len, fft_len) samples per row, empty below one window."""
        if dither > 0:
            raise AudioGenerationError(3, "MossFormer2-SE: dither > 0 is not served: the reference draws it from a random stream that "
                                          "cannot be reproduced")
        return self._waves(_lib.lib().mis_mossformer2_enhance, waveforms, sample_rate, junk)

    def enhance(self, waveform, sample_rate: int = 48000, dither: float = 0.0) -> np.ndarray:
        """enhance (:395-470): one waveform -> the enhanced waveform, (T - 1) win_inc + min(win_len, fft_len) samples."""
        return self.enhance_batch([waveform], sample_rate, dither)[0]

    def synthesize_batch(self, waveforms, mask, sample_rate=None) -> list:
        """The synthesis alone: the rows' STFT x a given mask [B, Tmax, out_channels_final] -> waveforms."""
        m = np.ascontiguousarray(mask, dtype=_F)
        if m.ndim != 3 or m.shape[0] != len(waveforms) or m.shape[2] != self.config.out_channels_final:
            raise AudioGenerationError(3, f"MossFormer2-SE: a mask of shape {m.shape}")
        return self._waves(_lib.lib().mis_mossformer2_synthesize, waveforms, sample_rate, None, m.ctypes.data, m.shape[1])

    def tap(self, stage: int) -> np.ndarray:
        """Tensors of the last call (include/mi_speech.h lists the stages); the waveform stage comes back as [B, samples]."""
        dims = (C.c_int64 * 3)()
        check(_lib.lib().mis_mossformer2_tap(self._h, stage, None, 0, dims))
        out = np.zeros(tuple(int(d) for d in dims), _F)
        check(_lib.lib().mis_mossformer2_tap(self._h, stage, out.ctypes.data, out.size, dims))
        return out[:, :, 0] if stage == 10 + 2 * self.config.num_blocks else out

    def timing(self):
        """Device milliseconds of the last call: (front end, mask network, synthesis)."""
        ms = (C.c_float * 3)()
        check(_lib.lib().mis_debug_mossformer2_timing(self._h, ms))
        return float(ms[0]), float(ms[1]), float(ms[2])


# ------------------------------------------------------------------------------------------------------------ DeepFilterNet
class DeepFilterNetError(AudioGenerationError):
    """DeepFilterNetError (DeepFilterNetModel.swift:8-37): `.sts_case` is modelPathNotFound, missingConfig, missingWeights,
    missingWeightKey, invalidAudioShape or streamingNotSupportedForModelVersion.  invalidRepoID cannot be reached: nothing is downloaded."""

    def __init__(self, sts_case: str, message: str):
        self.sts_case = sts_case
        super().__init__(3, message)


_DFN_KEYS = ("sample_rate", "fft_size", "hop_size", "min_nb_erb_freqs", "nb_erb", "nb_df", "df_order", "df_lookahead", "conv_lookahead",
             "conv_ch", "conv_k_enc", "conv_k_dec", "conv_width_factor", "emb_hidden_dim", "emb_num_layers", "df_hidden_dim", "df_num_layers",
             "gru_groups", "linear_groups", "enc_linear_groups", "group_shuffle", "enc_concat", "df_gru_skip", "conv_kernel", "convt_kernel",
             "conv_kernel_inp", "df_pathway_kernel_size_t", "lsnr_max", "lsnr_min", "model_version", "erb_widths")


def compute_norm_alpha(hop_size: int, sample_rate: int) -> float:
    """computeNormAlpha (DeepFilterNetDSP.swift:102-112) in float32: exp(-hop / sr) rounded to the fewest decimals (from 3) below 1."""
    a_raw = np.exp(-_F(hop_size) / _F(sample_rate), dtype=_F)
    precision, a = 3, _F(1.0)
    while a >= 1.0:
        scale = _F(10.0) ** _F(precision)
        a = _F(np.floor(np.abs(a_raw * scale) + _F(0.5)) * np.sign(a_raw)) / scale      # .rounded(): half away from zero
        precision += 1
    return float(a)


def libdf_erb_band_widths(sample_rate: int, fft_size: int, nb_bands: int, min_nb_freqs: int) -> list:
    """libdfErbBandWidths (DeepFilterNetDSP.swift:159-201) in float32."""
    if sample_rate <= 0 or fft_size <= 0 or nb_bands <= 0:
        return []
    f2e = lambda f: _F(9.265) * np.log1p(_F(f) / (_F(24.7) * _F(9.265)), dtype=_F)
    e2f = lambda e: _F(24.7) * _F(9.265) * (np.exp(_F(e) / _F(9.265), dtype=_F) - _F(1.0))
    nyq, freq_width = sample_rate // 2, _F(sample_rate) / _F(fft_size)
    erb_low, erb_high = f2e(0), f2e(nyq)
    step = (erb_high - erb_low) / _F(nb_bands)
    widths, prev, over, min_bins = [0] * nb_bands, 0, 0, max(1, min_nb_freqs)
    for i in range(1, nb_bands + 1):
        q = e2f(erb_low + _F(i) * step) / freq_width
        fb = int(np.floor(q + _F(0.5)))
        nb = fb - prev - over
        if nb < min_bins:
            over, nb = min_bins - nb, min_bins
        else:
            over = 0
        widths[i - 1] = max(1, nb)
        prev = fb
    widths[-1] += 1
    widths[-1] += fft_size // 2 + 1 - sum(widths)
    return widths


@dataclass
class DeepFilterNetConfig:
    """DeepFilterNetConfig (DeepFilterNetConfig.swift): every field, default and snake_case key.  max_batch / max_seconds size the
    engine's workspace, gru_kr picks the register columns of the recurrence kernel (0: the default); none is part of a checkpoint."""
    sample_rate: int = 48000
    fft_size: int = 960
    hop_size: int = 480
    min_nb_erb_freqs: int = 2
    nb_erb: int = 32
    nb_df: int = 96
    df_order: int = 5
    df_lookahead: int = 2
    conv_lookahead: int = 2
    conv_ch: int = 64
    conv_k_enc: int = 1
    conv_k_dec: int = 1
    conv_width_factor: int = 1
    emb_hidden_dim: int = 256
    emb_num_layers: int = 3
    df_hidden_dim: int = 256
    df_num_layers: int = 2
    gru_groups: int = 8
    linear_groups: int = 16
    enc_linear_groups: int = 32
    group_shuffle: bool = False
    enc_concat: bool = False
    df_gru_skip: str = "groupedlinear"
    conv_kernel: tuple = (1, 3)
    convt_kernel: tuple = (1, 3)
    conv_kernel_inp: tuple = (3, 3)
    df_pathway_kernel_size_t: int = 5
    lsnr_max: int = 35
    lsnr_min: int = -15
    model_version: str = "DeepFilterNet3"
    erb_widths: list | None = None
    max_batch: int = 8
    max_seconds: float = 60.0
    gru_kr: int = 0

    def __post_init__(self):
        if not self.model_version:
            self.model_version = "DeepFilterNet3"

    @classmethod
    def from_dict(cls, d: dict, **workspace) -> "DeepFilterNetConfig":
        """init(from:): missing or null keys take the defaults, unknown keys are ignored; an empty model_version is DeepFilterNet3."""
        return cls(**{k: d[k] for k in _DFN_KEYS if d.get(k) is not None}, **workspace)

    @property
    def freq_bins(self) -> int:
        return self.fft_size // 2 + 1

    @property
    def model_type(self) -> str:
        v = self.model_version.lower()
        return v if v in ("deepfilternet", "deepfilternet2") else "deepfilternet3"

    @property
    def max_samples(self) -> int:
        return max(1, int(round(self.max_seconds * self.sample_rate)))

    @property
    def norm_alpha(self) -> float:
        return compute_norm_alpha(self.hop_size, self.sample_rate)

    @property
    def wnorm(self) -> float:
        return float(_F(1.0) / _F(self.fft_size * self.fft_size) * _F(2 * self.hop_size))

    @property
    def erb_band_widths(self) -> list:
        """The initialiser's rule: the config's widths when they sum to freq_bins, else libdfErbBandWidths."""
        if self.erb_widths is not None and sum(self.erb_widths) == self.freq_bins:
            return [int(w) for w in self.erb_widths]
        return libdf_erb_band_widths(self.sample_rate, self.fft_size, self.nb_erb, max(1, self.min_nb_erb_freqs))

    def check_served(self):
        if self.model_version.lower() == "deepfilternet":
            raise AudioGenerationError(3, "DeepFilterNet: model_version 'DeepFilterNet' (V1) is not served: its graph (grouped GRUs, "
                                          "clc_* decoder, alpha blend) differs from V2 / V3; use a DeepFilterNet2 or DeepFilterNet3 checkpoint")
        if self.enc_concat:
            raise AudioGenerationError(3, "DeepFilterNet: enc_concat = true is not served (the encoder adds its two embeddings)")

    def to_c(self) -> "_lib.DeepFilterNetConfigC":
        self.check_served()
        w = self.erb_band_widths
        if not 1 <= self.nb_erb <= 128 or len(w) != self.nb_erb:
            raise AudioGenerationError(3, f"DeepFilterNet: nb_erb {self.nb_erb} with {len(w)} band widths (1..128 bands are served)")
        c = _lib.DeepFilterNetConfigC()
        for k in ("sample_rate", "fft_size", "hop_size", "nb_erb", "nb_df", "df_order", "df_lookahead", "conv_lookahead", "conv_ch",
                  "emb_hidden_dim", "df_hidden_dim", "lsnr_max", "lsnr_min", "emb_num_layers", "df_num_layers", "linear_groups",
                  "enc_linear_groups", "df_pathway_kernel_size_t", "gru_kr", "max_batch"):
            setattr(c, k, int(getattr(self, k)))
        for k in ("conv_kernel", "convt_kernel", "conv_kernel_inp"):
            v = list(getattr(self, k))
            if len(v) != 2:
                raise AudioGenerationError(3, f"DeepFilterNet: {k} must hold two sizes")
            setattr(c, k, (C.c_int32 * 2)(*v))
        c.norm_alpha = self.norm_alpha
        c.erb_widths = (C.c_int32 * 128)(*w)
        c.max_samples = self.max_samples
        return c


_DFN_OPTIONAL = ("erb_fb", "df_dec.df_skip.weight", "enc.emb_gru.linear_out.0.weight", "erb_dec.emb_gru.linear_out.0.weight")


def deepfilternet_expected_shapes(config: DeepFilterNetConfig, weights: dict) -> dict:
    """name -> shape of every tensor the V2 / V3 chain reads from `weights`, in the order the reference asks for them
    (mask.erb_inv_fb first, as its initialiser does).  GRU layer counts, groups and conv kernel sizes are the tensors' own; erb_fb,
    df_dec.df_skip.weight and the linear_outs are optional.  A missing required key raises missingWeightKey naming it; a shape that
    does not fit the chain raises with both shapes."""
    C_, E, D, O, F = config.conv_ch, config.nb_erb, config.nb_df, config.df_order, config.freq_bins
    want = {}

    def need(key, shape=None):
        if key not in weights:
            raise DeepFilterNetError("missingWeightKey", f"Missing DeepFilterNet weight key: {key}")
        got = tuple(weights[key].shape)
        if shape is not None:
            if len(got) != len(shape) or any(s is not None and s != g for s, g in zip(shape, got)):
                raise AudioGenerationError(3, f"DeepFilterNet checkpoint: {key} has shape {got}, expected "
                                              f"{tuple('*' if s is None else s for s in shape)}")
        want[key] = got
        return got

    def bn(p, n):
        for k in ("weight", "bias", "running_mean", "running_var"):
            need(f"{p}.{k}", (n,))

    def conv(p, main, pw, bnidx, cin, cout=None, transposed=False):
        m = need(f"{p}.{main}.weight", (cin, None, None, None) if transposed else (None, None, None, None))
        mid = cin * m[1] if transposed else m[0]
        if pw is not None:
            mid = need(f"{p}.{pw}.weight", (cout, mid, 1, 1))[0]
        elif cout is not None and mid != cout:
            raise AudioGenerationError(3, f"DeepFilterNet checkpoint: {p}.{main}.weight has shape {m}, expected {cout} outputs")
        bn(f"{p}.{bnidx}", mid)
        return mid

    def squeezed(p, din, hidden, dout):
        g = need(f"{p}.linear_in.0.weight", (None, None, None))
        if g[0] * g[1] != din or g[0] * g[2] != hidden:
            raise AudioGenerationError(3, f"DeepFilterNet checkpoint: {p}.linear_in.0.weight has shape {g}, expected [groups, "
                                          f"{din} / groups, {hidden} / groups]")
        n = 0
        while f"{p}.gru.weight_ih_l{n}" in weights:
            need(f"{p}.gru.weight_ih_l{n}", (3 * hidden, hidden)), need(f"{p}.gru.weight_hh_l{n}", (3 * hidden, hidden))
            need(f"{p}.gru.bias_ih_l{n}", (3 * hidden,)), need(f"{p}.gru.bias_hh_l{n}", (3 * hidden,))
            n += 1
        if n == 0:
            need(f"{p}.gru.weight_ih_l0")
        if dout and f"{p}.linear_out.0.weight" in weights:
            g = need(f"{p}.linear_out.0.weight", (None, None, None))
            if g[0] * g[1] != hidden or g[0] * g[2] != dout:
                raise AudioGenerationError(3, f"DeepFilterNet checkpoint: {p}.linear_out.0.weight has shape {g}, expected [groups, "
                                              f"{hidden} / groups, {dout} / groups]")
            return dout
        return hidden

    need("mask.erb_inv_fb", (E, F))
    if "erb_fb" in weights:
        want["erb_fb"] = tuple(weights["erb_fb"].shape)                  # used only when it is [freq_bins, nb_erb] (erbEnergies)
    conv("enc.erb_conv0", 1, None, 2, 1, C_)
    for i in (1, 2, 3):
        conv(f"enc.erb_conv{i}", 0, 1, 2, C_, C_)
    conv("enc.df_conv0", 1, 2, 3, 2, C_)
    conv("enc.df_conv1", 0, 1, 2, C_, C_)
    emb = C_ * (E // 4)
    g = need("enc.df_fc_emb.0.weight", (None, None, None))
    if g[0] * g[1] != C_ * (D // 2) or g[0] * g[2] != emb:
        raise AudioGenerationError(3, f"DeepFilterNet checkpoint: enc.df_fc_emb.0.weight has shape {g}, expected [groups, "
                                      f"{C_ * (D // 2)} / groups, {emb} / groups]")
    e_out = squeezed("enc.emb_gru", emb, config.emb_hidden_dim, emb)
    need("enc.lsnr_fc.0.weight", (1, e_out)), need("enc.lsnr_fc.0.bias", (1,))
    d_out = squeezed("erb_dec.emb_gru", e_out, config.emb_hidden_dim, emb)
    if d_out != emb:
        raise AudioGenerationError(3, f"DeepFilterNet checkpoint: erb_dec.emb_gru gives {d_out} values a frame, the decoder needs {emb}")
    for i in (3, 2, 1, 0):
        conv(f"erb_dec.conv{i}p", 0, None, 1, C_, C_)
    conv("erb_dec.convt3", 0, 1, 2, C_, C_)
    conv("erb_dec.convt2", 0, 1, 2, C_, C_, transposed=True)
    conv("erb_dec.convt1", 0, 1, 2, C_, C_, transposed=True)
    conv("erb_dec.conv0_out", 0, None, 1, C_, 1)
    squeezed("df_dec.df_gru", e_out, config.df_hidden_dim, 0)
    if "df_dec.df_skip.weight" in weights:
        g = need("df_dec.df_skip.weight", (None, None, None))
        if g[0] * g[1] != e_out or g[0] * g[2] != config.df_hidden_dim:
            raise AudioGenerationError(3, f"DeepFilterNet checkpoint: df_dec.df_skip.weight has shape {g}")
    conv("df_dec.df_convp", 1, 2, 3, C_, 2 * O)
    g = need("df_dec.df_out.0.weight", (None, None, None))
    if g[0] * g[1] != config.df_hidden_dim or g[0] * g[2] != D * O * 2:
        raise AudioGenerationError(3, f"DeepFilterNet checkpoint: df_dec.df_out.0.weight has shape {g}, expected [groups, "
                                      f"{config.df_hidden_dim} / groups, {D * O * 2} / groups]")
    return want


def deepfilternet_synthetic_weights(config: DeepFilterNetConfig, seed: int = 777, layers=None, erb_fb=True, df_skip=True) -> dict:
    """Random float32 weights at the shapes the configuration implies, in the checkpoint's names and layouts.  layers = GRU layers of
    (enc, erb_dec, df_dec); default DeepFilterNet3's (1, emb_num_layers - 1, df_num_layers)."""
    import math
    rng = np.random.default_rng(seed)
    C_, E, D, O, F, H, Hd = (config.conv_ch, config.nb_erb, config.nb_df, config.df_order, config.freq_bins, config.emb_hidden_dim,
                             config.df_hidden_dim)
    G, Ge, emb = config.linear_groups, config.enc_linear_groups, config.conv_ch * (config.nb_erb // 4)
    Le, Lr, Ld = layers if layers is not None else (1, max(1, config.emb_num_layers - 1), max(1, config.df_num_layers))
    W = {}
    u = lambda shape, amp: rng.uniform(-amp, amp, shape).astype(_F)

    def bn(p, n):
        W[p + ".weight"], W[p + ".bias"] = 1 + u((n,), 0.1), u((n,), 0.05)
        W[p + ".running_mean"], W[p + ".running_var"] = u((n,), 0.05), 1 + u((n,), 0.1)

    def conv(name, o, i, kt, kf, gain=1.0):
        W[name] = u((o, i, kt, kf), gain * math.sqrt(3.0 / (i * kt * kf)))

    def glin(name, g, din, dout):
        W[name] = u((g, din // g, dout // g), math.sqrt(3.0 / (din // g)))

    def sgru(p, din, h, n, dout):
        glin(p + ".linear_in.0.weight", G, din, h)
        for l in range(n):
            W[f"{p}.gru.weight_ih_l{l}"], W[f"{p}.gru.weight_hh_l{l}"] = u((3 * h, h), math.sqrt(3.0 / h)), u((3 * h, h), math.sqrt(3.0 / h))
            W[f"{p}.gru.bias_ih_l{l}"], W[f"{p}.gru.bias_hh_l{l}"] = u((3 * h,), 0.05), u((3 * h,), 0.05)
        if dout:
            glin(p + ".linear_out.0.weight", G, h, dout)

    (ki0, ki1), (k0, k1), (t0, t1) = config.conv_kernel_inp, config.conv_kernel, config.convt_kernel
    conv("enc.erb_conv0.1.weight", C_, 1, ki0, ki1), bn("enc.erb_conv0.2", C_)
    for i in (1, 2, 3):
        conv(f"enc.erb_conv{i}.0.weight", C_, 1, k0, k1), conv(f"enc.erb_conv{i}.1.weight", C_, C_, 1, 1, 1.4), bn(f"enc.erb_conv{i}.2", C_)
    conv("enc.df_conv0.1.weight", C_, 1, ki0, ki1), conv("enc.df_conv0.2.weight", C_, C_, 1, 1, 1.4), bn("enc.df_conv0.3", C_)
    conv("enc.df_conv1.0.weight", C_, 1, k0, k1), conv("enc.df_conv1.1.weight", C_, C_, 1, 1, 1.4), bn("enc.df_conv1.2", C_)
    glin("enc.df_fc_emb.0.weight", Ge, C_ * (D // 2), emb)
    sgru("enc.emb_gru", emb, H, Le, emb)
    W["enc.lsnr_fc.0.weight"], W["enc.lsnr_fc.0.bias"] = u((1, emb), math.sqrt(3.0 / emb)), u((1,), 0.05)
    sgru("erb_dec.emb_gru", emb, H, Lr, emb)
    for i in (0, 1, 2, 3):
        conv(f"erb_dec.conv{i}p.0.weight", C_, 1, 1, 1), bn(f"erb_dec.conv{i}p.1", C_)
    conv("erb_dec.convt3.0.weight", C_, 1, k0, k1), conv("erb_dec.convt3.1.weight", C_, C_, 1, 1, 1.4), bn("erb_dec.convt3.2", C_)
    for i in (1, 2):
        conv(f"erb_dec.convt{i}.0.weight", C_, 1, t0, t1), conv(f"erb_dec.convt{i}.1.weight", C_, C_, 1, 1, 1.4), bn(f"erb_dec.convt{i}.2", C_)
    conv("erb_dec.conv0_out.0.weight", 1, C_, k0, k1), bn("erb_dec.conv0_out.1", 1)
    sgru("df_dec.df_gru", emb, Hd, Ld, 0)
    if df_skip:
        glin("df_dec.df_skip.weight", G, emb, Hd)
    gc = math.gcd(C_, 2 * O)
    conv("df_dec.df_convp.1.weight", 2 * O, C_ // gc, config.df_pathway_kernel_size_t, 1)
    conv("df_dec.df_convp.2.weight", 2 * O, 2 * O, 1, 1, 1.4), bn("df_dec.df_convp.3", 2 * O)
    glin("df_dec.df_out.0.weight", G, Hd, D * O * 2)
    fb, inv, f = np.zeros((F, E), _F), np.zeros((E, F), _F), 0
    for e, w in enumerate(config.erb_band_widths):
        fb[f: f + w, e], inv[e, f: f + w], f = _F(1.0) / _F(w), 1.0, f + w
    W["mask.erb_inv_fb"] = inv
    if erb_fb:
        W["erb_fb"] = fb
    return W


class DeepFilterNet(NativeHandle):
    """DeepFilterNetModel.enhance (V2 / V3, offline) for ragged batches: one handle, 1..max_batch rows a call, each at most
    max_seconds long.  Hop by hop: DeepFilterNetStreamer(model) (createStreamer), deepfilternet_enhance_streaming(model, audio) and
    deepfilternet_stream_chunks(model, audio) (the two enhanceStreaming overloads); the method enhance_streaming of this class still
    raises, as it did before the streamer existed."""
    _prefix = "mis_deepfilternet"

    def __init__(self, config: DeepFilterNetConfig, device: int = 0):
        self.config = config
        self.device = device
        self.model_version = config.model_version
        self.layers = None
        self._create(config.to_c(), device)

    @property
    def sample_rate(self) -> int:
        return self.config.sample_rate

    supports_streaming = False

    @classmethod
    def from_weights(cls, config: DeepFilterNetConfig, weights: dict, device: int = 0) -> "DeepFilterNet":
        """weights: the checkpoint's names; every tensor the chain reads (deepfilternet_expected_shapes) is staged as f32, whatever the
        checkpoint's dtype; other keys (num_batches_tracked, ...) are ignored."""
        config.check_served()
        want = deepfilternet_expected_shapes(config, weights)
        m = cls(config, device)
        for name in want:
            arr = weights[name]
            try:
                import torch
                if isinstance(arr, torch.Tensor):
                    arr = arr.detach().to(torch.float32).cpu().numpy()
            except ImportError:
                pass
            m.set_tensor(name, np.ascontiguousarray(arr, dtype=_F))
        m.finalize()
        m.layers = tuple(sum(1 for k in want if k.startswith(p + ".gru.weight_ih_l"))
                         for p in ("enc.emb_gru", "erb_dec.emb_gru", "df_dec.df_gru"))
        return m

    @classmethod
    def synthetic(cls, config: DeepFilterNetConfig, device: int = 0, seed: int = 777) -> "DeepFilterNet":
        config.check_served()
        m = cls(config, device)
        check(_lib.lib().mis_deepfilternet_init_synthetic(m._h, seed))
        m.finalize()
        m.layers = (1, max(1, config.emb_num_layers - 1), max(1, config.df_num_layers))
        return m

    @classmethod
    def from_local(cls, directory: str, subfolder: str | None = None, device: int = 0, **workspace) -> "DeepFilterNet":
        """fromLocal (:280-312): the directory itself when it holds config.json, else its subfolder; model.safetensors first, else the
        first *.safetensors in name order."""
        model_dir = os.path.expanduser(directory)
        if not os.path.exists(os.path.join(model_dir, "config.json")) and subfolder:
            model_dir = os.path.join(model_dir, subfolder)
        cfg_path = os.path.join(model_dir, "config.json")
        if not os.path.exists(cfg_path):
            raise DeepFilterNetError("missingConfig", f"Missing config.json in model directory: {model_dir}")
        with open(cfg_path) as f:
            config = DeepFilterNetConfig.from_dict(json.load(f), **workspace)
        files = sorted(fn for fn in os.listdir(model_dir) if fn.lower().endswith(".safetensors"))
        if not files:
            raise DeepFilterNetError("missingWeights", f"Missing .safetensors weights in model directory: {model_dir}")
        name = "model.safetensors" if "model.safetensors" in files else files[0]
        config.check_served()
        from safetensors import safe_open
        with safe_open(os.path.join(model_dir, name), framework="pt") as sf:
            weights = {k: sf.get_tensor(k) for k in sf.keys()}
        m = cls.from_weights(config, weights, device)
        m.model_directory = model_dir
        return m

    @classmethod
    def from_pretrained(cls, path: str, subfolder: str | None = "v3", device: int = 0, **workspace) -> "DeepFilterNet":
        """fromPretrained (:244-268) for local paths: a directory goes to from_local with the subfolder, a file means its directory.
        Nothing is downloaded: any other path is modelPathNotFound."""
        local = os.path.abspath(os.path.expanduser(path))
        if os.path.isdir(local):
            return cls.from_local(local, subfolder, device, **workspace)
        if os.path.exists(local):
            return cls.from_local(os.path.dirname(local), None, device, **workspace)
        raise DeepFilterNetError("modelPathNotFound", f"Model path not found: {path} (this package downloads nothing)")

    @property
    def launches(self) -> int:
        return int(_lib.lib().mis_deepfilternet_launches(self._h))

    def expected_launches(self, erb_fb: bool, df_skip: bool, enc_linear_out: bool = True, erb_linear_out: bool = True) -> int:
        """The launch count of a call as the chain gives it."""
        le, lr, ld = self.layers
        paired = max(lr, ld) if self.config.emb_hidden_dim == self.config.df_hidden_dim else lr + ld
        return 26 + int(erb_fb) + int(df_skip) + int(enc_linear_out) + int(erb_linear_out) + 2 * le + lr + ld + paired

    def _row(self, audio, sample_rate) -> np.ndarray:
        a = np.asarray(audio)
        if a.ndim != 1:
            raise DeepFilterNetError("invalidAudioShape", f"Expected mono 1D audio array, got shape: {list(a.shape)}")
        a = a.astype(_F, copy=False)
        rate = self.config.sample_rate
        if sample_rate is not None and int(sample_rate) != rate:
            raise AudioGenerationError(3, f"DeepFilterNet: audio at {sample_rate} Hz, the model takes {rate} Hz; this package has no "
                                          "resampler - resample before the call")
        if len(a) > self.config.max_samples:
            raise AudioGenerationError(3, f"DeepFilterNet: a row of {len(a)} samples, the workspace holds {self.config.max_samples} "
                                          "(max_seconds)")
        return a

    def frames(self, lens):
        """Sample counts -> (frames T, output samples), int32 / int64 arrays."""
        lens = np.ascontiguousarray(lens, np.int64)
        T, n = np.zeros(len(lens), np.int32), np.zeros(len(lens), np.int64)
        check(_lib.lib().mis_deepfilternet_frames(self._h, lens.ctypes.data, len(lens), T.ctypes.data, n.ctypes.data))
        return T, n

    def enhance_raw(self, waveforms, sample_rate=None, junk: float | None = None):
        """Ragged list of waveforms -> (waveforms, lsnr): one float32 array of the row's own length and one of its T frames per row."""
        rows = [self._row(w, sample_rate) for w in waveforms]
        if not rows:
            raise AudioGenerationError(3, "DeepFilterNet: no rows")
        pcm, lens = pack_rows(rows, junk)
        B, stride = pcm.shape
        T, _ = self.frames(lens)
        out, got, lsnr = np.zeros((B, stride), _F), np.zeros(B, np.int64), np.zeros((B, int(T.max())), _F)
        check(_lib.lib().mis_deepfilternet_enhance(self._h, pcm.ctypes.data, lens.ctypes.data, B, stride, out.ctypes.data, stride,
                                                   got.ctypes.data, lsnr.ctypes.data, lsnr.shape[1]))
        return [out[b, : int(got[b])].copy() for b in range(B)], [lsnr[b, : int(T[b])].copy() for b in range(B)]

    def enhance_batch(self, waveforms, sample_rate=None, junk: float | None = None) -> list:
        return self.enhance_raw(waveforms, sample_rate, junk)[0]

    def enhance(self, waveform, sample_rate: int = 48000) -> np.ndarray:
        """enhance (:323-418): one waveform -> the enhanced waveform of the same length."""
        return self.enhance_batch([waveform], sample_rate)[0]

    def enhance_streaming(self, *a, **kw):
        raise DeepFilterNetError("streamingNotSupportedForModelVersion",
                                 f"Streaming is not supported for model version {self.model_version}. Use offline enhancement instead.")

    def tap(self, stage: int) -> np.ndarray:
        """Tensors of the last call (include/mi_speech.h lists the stages), [B, rows, width]; the waveform stage as [B, samples]."""
        dims = (C.c_int64 * 3)()
        check(_lib.lib().mis_deepfilternet_tap(self._h, stage, None, 0, dims))
        out = np.zeros(tuple(int(d) for d in dims), _F)
        check(_lib.lib().mis_deepfilternet_tap(self._h, stage, out.ctypes.data, out.size, dims))
        return out[:, :, 0] if stage == 25 else out

    def timing(self):
        """Device milliseconds of the last call: (front end, network without the recurrences, recurrences, synthesis)."""
        ms = (C.c_float * 4)()
        check(_lib.lib().mis_debug_deepfilternet_timing(self._h, ms))
        return tuple(float(v) for v in ms)


# ------------------------------------------------------------------------------------------------------------ DeepFilterNet, hop by hop
@dataclass
class DeepFilterNetStreamingConfig:
    """DeepFilterNetStreamingConfig (DeepFilterNetModel.swift:40-82): every field and default.  Stage skipping is refused by the
    streamer (its thresholds stay so that the fields round-trip); the profiling fields and materialize_every_hops are accepted and
    ignored: they steer the reference's lazy evaluation, which this engine does not have."""
    pad_end_frames: int = 3
    compensate_delay: bool = True
    enable_stage_skipping: bool = False
    min_db_thresh: float = -10.0
    max_db_erb_thresh: float = 30.0
    max_db_df_thresh: float = 20.0
    enable_profiling: bool = False
    profiling_force_eval_per_stage: bool = False
    materialize_every_hops: int = 512


def deepfilternet_stream_check_served(config: DeepFilterNetConfig, streaming: "DeepFilterNetStreamingConfig"):
    """What the streamer refuses before the device is touched (csrc/deepfilternet_stream.hip refuses the two shapes again)."""
    config.check_served()
    if streaming.enable_stage_skipping:
        raise AudioGenerationError(3, "DeepFilterNet streaming: enable_stage_skipping = true is not served: the reference lets the decoder "
                                      "GRUs stand still on skipped frames, which needs one host decision a hop; every stage runs on every hop")
    if config.fft_size != 2 * config.hop_size:
        raise AudioGenerationError(3, f"DeepFilterNet streaming: fft_size {config.fft_size} with hop_size {config.hop_size} is not served "
                                      "(fft_size == 2 hop_size: the offline frame grid and the analysis memory coincide at this ratio only)")
    if config.df_lookahead > config.conv_lookahead:
        raise AudioGenerationError(3, f"DeepFilterNet streaming: df_lookahead {config.df_lookahead} above conv_lookahead "
                                      f"{config.conv_lookahead} is not served (the deep filter would read frames that have not arrived)")
    if streaming.pad_end_frames < 0:
        raise AudioGenerationError(3, "DeepFilterNet streaming: pad_end_frames is negative")


class DeepFilterNetStreamer:
    """DeepFilterNetStreamer (DeepFilterNetStreamer.swift) for 1..max_batch streams on one model: process_chunk / flush / reset for
    stream 0, process_chunks for all slots at once.  The host keeps what processChunk keeps, a stream's pending remainder below one hop,
    the delay counter and the end padding; whole hops go to mis_deepfilternet_stream_feed, at most max_hops a stream and feed.  Fed any
    chunking and flushed, a stream returns count = (H - conv_lookahead) hop - (fft - hop) samples for its H whole hops (compensate_delay;
    fft - hop more without), bit for bit the first count samples of model.enhance on the same zero-extended samples.

    _feed (tests): a callable (list of float32 arrays of whole hops, one a slot) -> (list of outputs, list of lsnr) in place of the device."""

    def __init__(self, model, config: DeepFilterNetStreamingConfig | None = None, streams: int = 1, max_hops: int = 16, _feed=None):
        self.model = model
        self.config = config if config is not None else DeepFilterNetStreamingConfig()
        deepfilternet_stream_check_served(model.config, self.config)
        self.streams, self.max_hops = int(streams), int(max_hops)
        self.hop, self.delay = model.config.hop_size, model.config.fft_size - model.config.hop_size
        self._h, self._fake = None, _feed
        if _feed is None:
            h = C.c_void_p()
            check(_lib.lib().mis_deepfilternet_stream_create(model._h, self.streams, self.max_hops, C.byref(h)))
            self._h = h
        elif not (1 <= self.streams and 1 <= self.max_hops):
            raise AudioGenerationError(3, "DeepFilterNet streaming: streams and max_hops start at 1")
        self._seen = [0] * self.streams
        self._pending = [np.zeros(0, _F) for _ in range(self.streams)]
        self._dropped = [0] * self.streams
        self.last_lsnr = [np.zeros(0, _F) for _ in range(self.streams)]

    def close(self):
        h, self._h = self._h, None
        if h:
            _lib.lib().mis_deepfilternet_stream_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:                                                # interpreter shutdown
            pass

    @property
    def launches(self) -> int:
        """Kernel launches of the last feed."""
        return int(_lib.lib().mis_deepfilternet_stream_launches(self._h)) if self._h else 0

    def expected_launches(self, targets: bool, erb_fb: bool, df_skip: bool, enc_linear_out: bool = True, erb_linear_out: bool = True) -> int:
        """The launch count of a feed: with targets the offline chain + the roll; before the look-ahead has filled, the
        front end (analysis [+ erb_fb] + features) + the roll."""
        return self.model.expected_launches(erb_fb, df_skip, enc_linear_out, erb_linear_out) + 1 if targets else 3 + int(erb_fb)

    @property
    def hops_seen(self):
        """Hops every stream has been fed since its last reset; an int for a single stream."""
        seen = [int(_lib.lib().mis_deepfilternet_stream_hops_seen(self._h, b)) for b in range(self.streams)] if self._h else list(self._seen)
        return seen[0] if self.streams == 1 else seen

    def timing(self):
        """Device milliseconds of the last feed: (the whole feed, its recurrence launches)."""
        ms = (C.c_float * 2)()
        check(_lib.lib().mis_debug_deepfilternet_stream_timing(self._h, ms))
        return float(ms[0]), float(ms[1])

    def set_gru_step_frames(self, frames: int):
        """Measurements and tests: feeds of at most `frames` targets run the short-chunk recurrence (0 never, negative the default)."""
        check(_lib.lib().mis_debug_deepfilternet_stream_gru_step_frames(self._h, int(frames)))

    def reset(self, stream: int | None = None):
        """reset(): one stream (None: all) back to the state after create."""
        if stream is not None and not 0 <= stream < self.streams:
            raise AudioGenerationError(3, f"DeepFilterNet streaming: stream {stream} outside 0..{self.streams - 1}")
        if self._h:
            check(_lib.lib().mis_deepfilternet_stream_reset(self._h, -1 if stream is None else int(stream)))
        for b in range(self.streams) if stream is None else (stream,):
            self._seen[b], self._pending[b], self._dropped[b], self.last_lsnr[b] = 0, np.zeros(0, _F), 0, np.zeros(0, _F)

    # ---- whole hops to the device
    def feed_hops(self, rows, junk=None):
        """rows: a float32 array of whole hops (at most max_hops; may be empty) for every slot -> (outputs, lsnr), one array each a slot.
        The raw device interface: no pending remainder, no delay drop."""
        rows = [np.ascontiguousarray(r, _F) for r in rows]
        if len(rows) != self.streams or any(r.ndim != 1 or len(r) % self.hop for r in rows):
            raise AudioGenerationError(3, f"DeepFilterNet streaming: a feed takes {self.streams} rows of whole hops")
        for b, r in enumerate(rows):
            self._seen[b] += len(r) // self.hop
        if self._fake is not None:
            return self._fake(rows)
        pcm, lens = pack_rows(rows, junk)
        hops = np.ascontiguousarray(lens // self.hop, np.int32)
        B, room = self.streams, max(1, self.max_hops * self.hop)
        out, got = np.zeros((B, room), _F), np.zeros(B, np.int64)
        lsnr, lc = np.zeros((B, self.max_hops), _F), np.zeros(B, np.int32)
        check(_lib.lib().mis_deepfilternet_stream_feed(self._h, pcm.ctypes.data, hops.ctypes.data, pcm.shape[1], out.ctypes.data, room,
                                                       got.ctypes.data, lsnr.ctypes.data, lsnr.shape[1], lc.ctypes.data))
        return [out[b, : int(got[b])].copy() for b in range(B)], [lsnr[b, : int(lc[b])].copy() for b in range(B)]

    def _run(self, chunks, last):
        """processChunk for every slot: chunks[b] an array or None (the slot is left alone), last[b] its isLast."""
        hop, B = self.hop, self.streams
        todo = [np.zeros(0, _F)] * B
        for b, ch in enumerate(chunks):
            if ch is None:
                continue
            a = np.asarray(ch)
            if a.ndim != 1:
                raise DeepFilterNetError("invalidAudioShape", f"Expected mono 1D audio array, got shape: {list(a.shape)}")
            p = np.concatenate([self._pending[b], a.astype(_F, copy=False)])
            n = len(p) // hop * hop
            whole, p = p[:n], p[n:]
            if last[b] and self.config.pad_end_frames > 0:               # the remainder stays in front of the padding, as in the reference
                p = np.concatenate([p, np.zeros(self.config.pad_end_frames * hop, _F)])
                n = len(p) // hop * hop
                whole, p = np.concatenate([whole, p[:n]]), p[n:]
            todo[b], self._pending[b] = whole, p
        outs, lsnrs = [[] for _ in range(B)], [[] for _ in range(B)]
        step = self.max_hops * hop
        for at in range(0, max(len(t) for t in todo), step):             # a chunk above max_hops hops is walked in several feeds
            o, l = self.feed_hops([t[at: at + step] for t in todo])
            for b in range(B):
                outs[b].append(o[b]), lsnrs[b].append(l[b])
        res = []
        for b in range(B):
            if chunks[b] is None:
                res.append(None)
                continue
            y = np.concatenate(outs[b]) if outs[b] else np.zeros(0, _F)
            self.last_lsnr[b] = np.concatenate(lsnrs[b]) if lsnrs[b] else np.zeros(0, _F)
            if self.config.compensate_delay and self._dropped[b] < self.delay:
                drop = min(self.delay - self._dropped[b], len(y))
                y, self._dropped[b] = y[drop:], self._dropped[b] + drop
            res.append(y)
        return res

    def process_chunks(self, chunks, is_last=False) -> list:
        """One chunk (1-D array) or None for every stream slot -> one output array, or None, a slot.  is_last: one flag, or one a slot."""
        chunks = list(chunks)
        if len(chunks) != self.streams:
            raise AudioGenerationError(3, f"DeepFilterNet streaming: {len(chunks)} chunks for {self.streams} streams")
        last = list(is_last) if isinstance(is_last, (list, tuple)) else [bool(is_last)] * self.streams
        return self._run(chunks, last)

    def process_chunk(self, chunk, is_last: bool = False) -> np.ndarray:
        """processChunk (:282-359) for stream 0: enhanced samples, possibly none while the look-ahead fills.  The per-frame lsnr of the
        targets it ran is in last_lsnr[0]."""
        return self._run([chunk] + [None] * (self.streams - 1), [is_last] + [False] * (self.streams - 1))[0]

    def flush(self) -> np.ndarray:
        """flush (:374-381): the end padding and what it releases."""
        return self.process_chunk(np.zeros(0, _F), True)


def deepfilternet_stream_chunks(model, audio, chunk_samples=None, config: DeepFilterNetStreamingConfig | None = None, max_hops: int = 16):
    """enhanceStreaming as a stream of chunks (DeepFilterNetModel.swift:496-547): yields (audio, chunk_index, is_last_chunk) for every
    non-empty output; chunk_samples is floored at one hop."""
    a = np.asarray(audio)
    if a.ndim != 1:
        raise DeepFilterNetError("invalidAudioShape", f"Expected mono 1D audio array, got shape: {list(a.shape)}")
    a = a.astype(_F, copy=False)
    st = DeepFilterNetStreamer(model, config, 1, max_hops)
    try:
        step = max(model.config.hop_size, int(chunk_samples) if chunk_samples is not None else model.config.hop_size)
        index = 0
        for at in range(0, len(a), step):
            out = st.process_chunk(a[at: at + step])
            if len(out):
                yield out, index, False
                index += 1
        tail = st.flush()
        if len(tail):
            yield tail, index, True
    finally:
        st.close()


def deepfilternet_enhance_streaming(model, audio, chunk_samples=None, config: DeepFilterNetStreamingConfig | None = None) -> np.ndarray:
    """enhanceStreaming (DeepFilterNetModel.swift:448-487): the clipped concatenation of the streamer's outputs; empty audio gives
    empty audio."""
    a = np.asarray(audio)
    if a.ndim != 1:
        raise DeepFilterNetError("invalidAudioShape", f"Expected mono 1D audio array, got shape: {list(a.shape)}")
    if a.size == 0:
        return np.zeros(0, _F)
    parts = [out for out, _, _ in deepfilternet_stream_chunks(model, a, chunk_samples, config)]
    return np.clip(np.concatenate(parts), -1.0, 1.0).astype(_F) if parts else np.zeros(0, _F)


# ------------------------------------------------------------------------------------------------------------ the factory
_MOSSFORMER_TYPES = ("mossformer2_se", "mossformer2", "mossformer")
_DEEPFILTERNET_TYPES = ("deepfilternet", "deepfilternet2", "deepfilternet3", "dfn")


def _infer_model_type(path: str):
    """inferModelType (:143-158), in the reference's order."""
    lower = path.lower()
    if "lfm" in lower:
        return "lfm_audio"
    if "mossformer" in lower:
        return "mossformer2_se"
    if "deepfilter" in lower or "dfn" in lower:
        return "deepfilternet3"
    if "sam" in lower or "source-separation" in lower:
        return "sam_audio"
    return None


def resolve_sts_model_type(path: str, model_type=None):
    """The type STS.loadModel would load (:54-132): an explicit model_type (trimmed, lower-cased, empty = none), else for an existing
    local path model_type, architecture, model_version of its config.json in that order, else inference from the path."""
    if model_type is not None and model_type.strip():
        return model_type.strip().lower()
    p = os.path.abspath(os.path.expanduser(path))
    if model_type is None and os.path.exists(p):
        cfg = os.path.join(p, "config.json") if os.path.isdir(p) else (p if os.path.basename(p) == "config.json"
                                                                        else os.path.join(os.path.dirname(p), "config.json"))
        if os.path.exists(cfg):
            with open(cfg) as f:
                d = json.load(f)
            if isinstance(d, dict):
                for key in ("model_type", "architecture", "model_version"):
                    if isinstance(d.get(key), str):
                        found = d[key].strip().lower()
                        return found if found else _infer_model_type(path)
        return _infer_model_type(p)
    return _infer_model_type(path)


def load_sts_model(path: str, model_type=None, device: int = 0, **workspace):
    """STS.loadModel for a local directory; this package downloads nothing.  Serves mossformer2_se / mossformer2 / mossformer, and
    deepfilternet / deepfilternet2 / deepfilternet3 / dfn when the path is an existing directory."""
    resolved = resolve_sts_model_type(path, model_type)
    if resolved in _DEEPFILTERNET_TYPES and os.path.isdir(os.path.expanduser(path)):
        return DeepFilterNet.from_local(os.path.expanduser(path), "v3", device, **workspace)
    if resolved not in _MOSSFORMER_TYPES:
        raise STSModelError(resolved if resolved is not None else model_type)
    p = os.path.expanduser(path)
    if not os.path.isdir(p):
        raise AudioGenerationError(3, f"MossFormer2-SE: {path} is no local model directory (nothing is downloaded)")
    return MossFormer2SE.from_model_directory(p, device, **workspace)
