"""MossFormer2-SE speech enhancement, host mirror of `MossFormer2SEModel` (Sources/MLXAudioSTS/Models/MossFormer2SE) and of the
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


# ------------------------------------------------------------------------------------------------------------ the factory
_MOSSFORMER_TYPES = ("mossformer2_se", "mossformer2", "mossformer")


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
    """STS.loadModel for a local directory; this package downloads nothing.  Serves mossformer2_se / mossformer2 / mossformer."""
    resolved = resolve_sts_model_type(path, model_type)
    if resolved not in _MOSSFORMER_TYPES:
        raise STSModelError(resolved if resolved is not None else model_type)
    p = os.path.expanduser(path)
    if not os.path.isdir(p):
        raise AudioGenerationError(3, f"MossFormer2-SE: {path} is no local model directory (nothing is downloaded)")
    return MossFormer2SE.from_model_directory(p, device, **workspace)
