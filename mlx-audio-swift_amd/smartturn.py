"""Smart Turn endpoint detection, host mirror of `SmartTurnModel` (Sources/MLXAudioVAD/Models/SmartTurn/SmartTurn.swift:152-363,
SmartTurnConfig.swift:3-178, SmartTurnFeatures.swift:10-81).  Configuration, checkpoint key mapping and the ragged-batch packing stay on
the host; the window, its normalisation, the log-mel features, the encoder, the attention pool and the classifier run in
libmi_speech.so (csrc/smartturn.hip)."""
from __future__ import annotations

import ctypes as C
import json
import os
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._handle import NativeHandle, pack_rows, read_safetensors_dir
from .generation import AudioGenerationError, check


@dataclass
class SmartTurnEncoderConfig:
    """SmartTurnEncoderConfig (SmartTurnConfig.swift:3-55), every field and default."""
    model_type: str = "smart_turn_encoder"
    num_mel_bins: int = 80
    max_source_positions: int = 400
    d_model: int = 384
    encoder_attention_heads: int = 6
    encoder_layers: int = 4
    encoder_ffn_dim: int = 1536
    k_proj_bias: bool = False

    @classmethod
    def from_dict(cls, d: dict) -> "SmartTurnEncoderConfig":
        return cls(**{k: v for k, v in d.items() if k in cls.__dataclass_fields__ and v is not None})


@dataclass
class SmartTurnProcessorConfig:
    """SmartTurnProcessorConfig (SmartTurnConfig.swift:57-104)."""
    sampling_rate: int = 16000
    max_audio_seconds: int = 8
    n_fft: int = 400
    hop_length: int = 160
    n_mels: int = 80
    normalize_audio: bool = True
    threshold: float = 0.5

    @classmethod
    def from_dict(cls, d: dict) -> "SmartTurnProcessorConfig":
        return cls(**{k: v for k, v in d.items() if k in cls.__dataclass_fields__ and v is not None})


@dataclass
class SmartTurnConfig:
    """SmartTurnConfig (SmartTurnConfig.swift:106-178).  sample_rate / max_audio_seconds / threshold are the compatibility keys of the
    conversion scripts: they fill a missing processor_config (together with the encoder's num_mel_bins) and are ignored otherwise."""
    model_type: str = "smart_turn"
    architecture: str = "smart_turn"
    dtype: str = "float32"
    encoder_config: SmartTurnEncoderConfig = field(default_factory=SmartTurnEncoderConfig)
    processor_config: SmartTurnProcessorConfig | None = None
    sample_rate: int = 16000
    max_audio_seconds: int = 8
    threshold: float = 0.5

    def __post_init__(self):
        if isinstance(self.encoder_config, dict):
            self.encoder_config = SmartTurnEncoderConfig.from_dict(self.encoder_config)
        if isinstance(self.processor_config, dict):
            self.processor_config = SmartTurnProcessorConfig.from_dict(self.processor_config)
        if self.processor_config is None:                         # :146-151,170-175
            self.processor_config = SmartTurnProcessorConfig(sampling_rate=self.sample_rate, max_audio_seconds=self.max_audio_seconds,
                                                             n_mels=self.encoder_config.num_mel_bins, threshold=self.threshold)

    @classmethod
    def from_dict(cls, d: dict) -> "SmartTurnConfig":
        """init(from:) (:154-177): missing or null keys take the defaults, unknown keys are ignored."""
        return cls(**{k: v for k, v in d.items() if k in cls.__dataclass_fields__ and v is not None})

    @property
    def window_samples(self) -> int:
        return self.processor_config.max_audio_seconds * self.processor_config.sampling_rate

    @property
    def frames(self) -> int:                                      # targetFrames, SmartTurn.swift:231-233
        return self.window_samples // self.processor_config.hop_length

    @property
    def positions(self) -> int:
        return self.frames // 2

    def to_c(self) -> "_lib.SmartTurnConfigC":
        e, p = self.encoder_config, self.processor_config
        if p.n_mels != e.num_mel_bins:
            raise AudioGenerationError(3, f"Smart Turn: the processor makes {p.n_mels} mel bins, the encoder takes {e.num_mel_bins}")
        return _lib.SmartTurnConfigC(e.num_mel_bins, e.max_source_positions, e.d_model, e.encoder_attention_heads, e.encoder_layers,
                                     e.encoder_ffn_dim, int(bool(e.k_proj_bias)), p.sampling_rate, p.max_audio_seconds, p.n_fft,
                                     p.hop_length, int(bool(p.normalize_audio)), float(p.threshold))


@dataclass
class SmartTurnEndpointOutput:                                    # SmartTurn.swift:8-16
    prediction: int
    probability: float


_HEAD_RENAMES = (("pool_attention.0.", "pool_attention_0."), ("pool_attention.2.", "pool_attention_2."), ("classifier.0.", "classifier_0."),
                 ("classifier.1.", "classifier_1."), ("classifier.4.", "classifier_4."), ("classifier.6.", "classifier_6."))


def _swap(v, *axes):
    """A transposed view of a numpy array or torch tensor (layout only)."""
    return v.permute(*axes) if hasattr(v, "permute") else np.transpose(v, axes)


def smart_turn_sanitize(weights: dict) -> dict:
    """SmartTurnModel.sanitize (:274-324): val_* dropped, "inner." stripped, the Sequential indices of the head renamed, conv weights
    [out, in, k] -> [out, k, in], and the four orientation fixes (fc1 stored [d, ffn], fc2 stored [ffn, d], pool_attention_0 not
    [256, d], pool_attention_2 not [1, 256])."""
    out = {}
    for key, v in weights.items():
        if key.startswith("val_"):
            continue
        k = key[len("inner."):] if key.startswith("inner.") else key
        for a, b in _HEAD_RENAMES:
            k = k.replace(a, b)
        nd = len(v.shape)
        if k in ("encoder.conv1.weight", "encoder.conv2.weight") and nd == 3:
            v = _swap(v, 0, 2, 1)
        if k.endswith("fc1.weight") and nd == 2 and v.shape[0] < v.shape[1]:
            v = _swap(v, 1, 0)
        if k.endswith("fc2.weight") and nd == 2 and v.shape[0] > v.shape[1]:
            v = _swap(v, 1, 0)
        if k == "pool_attention_0.weight" and nd == 2 and v.shape[0] != 256:
            v = _swap(v, 1, 0)
        if k == "pool_attention_2.weight" and nd == 2 and v.shape[0] != 1:
            v = _swap(v, 1, 0)
        out[k] = v
    return out


def smart_turn_expected_keys(config: SmartTurnConfig) -> set:
    """The parameters of SmartTurnModel(config): what update(parameters:verify: .noUnusedKeys) accepts (:359)."""
    e = config.encoder_config
    keys = {"encoder.conv1.weight", "encoder.conv1.bias", "encoder.conv2.weight", "encoder.conv2.bias", "encoder.embed_positions.weight",
            "encoder.layer_norm.weight", "encoder.layer_norm.bias", "classifier_1.weight", "classifier_1.bias"}
    for n in ("pool_attention_0", "pool_attention_2", "classifier_0", "classifier_4", "classifier_6"):
        keys |= {n + ".weight", n + ".bias"}
    for i in range(e.encoder_layers):
        q = f"encoder.layers.{i}."
        for n in ("self_attn_layer_norm", "final_layer_norm", "fc1", "fc2", "self_attn.q_proj", "self_attn.v_proj", "self_attn.out_proj"):
            keys |= {q + n + ".weight", q + n + ".bias"}
        keys.add(q + "self_attn.k_proj.weight")
        if e.k_proj_bias:
            keys.add(q + "self_attn.k_proj.bias")
    return keys


def smart_turn_read_directory(model_dir: str):
    """config.json and every *.safetensors of a model directory (fromModelDirectory, :339-358) -> (SmartTurnConfig, sanitized weights).
    No device is touched.  MLX-quantised directories and keys the model does not have are errors."""
    with open(os.path.join(model_dir, "config.json")) as f:
        cfg = SmartTurnConfig.from_dict(json.load(f))

    def no_quant(fn, keys):
        quant = [k for k in keys if k.endswith(".scales") or k.endswith(".biases")]
        if quant:
            raise AudioGenerationError(3, f"{fn}: MLX-quantised Smart Turn checkpoints are not supported ({quant[0]})")

    weights = read_safetensors_dir(model_dir, missing_code=(1, f"No safetensors files found in {model_dir}"), on_keys=no_quant)
    weights = smart_turn_sanitize(weights)
    unknown = sorted(set(weights) - smart_turn_expected_keys(cfg))
    if unknown:
        raise AudioGenerationError(3, f"Smart Turn checkpoint has keys the model does not: {', '.join(unknown[:4])}")
    return cfg, weights


class SmartTurnModel(NativeHandle):
    """predict_endpoint / predict_endpoints / prepare_input_features / __call__ of the reference class; one handle, 1..64 rows a call."""
    _prefix = "mis_smartturn"

    def __init__(self, config: SmartTurnConfig, device: int = 0):
        self.config = config
        self.device = device
        self._last_batch = 0
        self._create(config.to_c(), device)

    @classmethod
    def from_weights(cls, config: SmartTurnConfig, weights: dict, device: int = 0) -> "SmartTurnModel":
        """weights: sanitized names and layouts (what smart_turn_sanitize returns)."""
        m = cls(config, device)
        for name, arr in weights.items():
            m.set_tensor(name, arr)
        m.finalize()
        return m

    @classmethod
    def synthetic(cls, config: SmartTurnConfig, device: int = 0, seed: int = 777) -> "SmartTurnModel":
        m = cls(config, device)
        check(_lib.lib().mis_smartturn_init_synthetic(m._h, seed))
        m.finalize()
        return m

    @classmethod
    def from_model_directory(cls, model_dir: str, device: int = 0) -> "SmartTurnModel":
        cfg, weights = smart_turn_read_directory(model_dir)
        return cls.from_weights(cfg, weights, device)

    @classmethod
    def from_pretrained(cls, model_name: str, device: int = 0) -> "SmartTurnModel":
        """fromPretrained (:326-337) for a local directory; repository ids would need a download, which this package never does."""
        path = os.path.expanduser(model_name)
        if not os.path.isdir(path):
            raise AudioGenerationError(3, f"Smart Turn: {model_name!r} is not a local model directory (downloads are not supported)")
        return cls.from_model_directory(path, device)

    @property
    def launches(self) -> int:
        return int(_lib.lib().mis_smartturn_launches(self._h))

    # -- inputs --------------------------------------------------------------------------------------
    def _row(self, audio, sample_rate) -> np.ndarray:
        a = np.asarray(audio, np.float32)
        if a.ndim != 1:                                           # SmartTurnError.invalidAudioShape (SmartTurnFeatures.swift:15-17)
            raise AudioGenerationError(3, f"Smart Turn: audio must be one-dimensional, got shape {a.shape}")
        rate = self.config.processor_config.sampling_rate
        if sample_rate is not None and int(sample_rate) != rate:
            raise AudioGenerationError(3, f"Smart Turn: audio at {sample_rate} Hz, the model takes {rate} Hz; this package has no "
                                          "resampler - resample before the call")
        return a

    @staticmethod
    def _pack(rows, junk: float | None = None):
        pcm, lens = pack_rows(rows, junk)
        return pcm, lens, pcm.shape[1]

    # -- calls ---------------------------------------------------------------------------------------
    def predict_raw(self, rows, sample_rate=None, threshold=None, junk: float | None = None):
        """Ragged list of waveforms -> (probability [B] f32, logit [B] f32, prediction [B] int32)."""
        rows = [self._row(r, sample_rate) for r in rows]
        B = len(rows)
        if B == 0:
            raise AudioGenerationError(3, "Smart Turn: no rows")
        pcm, lens, stride = self._pack(rows, junk)
        prob, logit, pred = np.zeros(B, np.float32), np.zeros(B, np.float32), np.zeros(B, np.int32)
        check(_lib.lib().mis_smartturn_predict(self._h, pcm.ctypes.data, lens.ctypes.data, B, stride,
                                               -1.0 if threshold is None else float(threshold), prob.ctypes.data, logit.ctypes.data,
                                               pred.ctypes.data))
        self._last_batch = B
        return prob, logit, pred

    def predict_endpoints(self, rows, sample_rate=None, threshold=None):
        prob, _, pred = self.predict_raw(rows, sample_rate, threshold)
        return [SmartTurnEndpointOutput(int(p), float(q)) for p, q in zip(pred, prob)]

    def predict_endpoint(self, audio, sample_rate=None, threshold=None) -> SmartTurnEndpointOutput:
        """predictEndpoint (:254-264)."""
        return self.predict_endpoints([audio], sample_rate, threshold)[0]

    def prepare_input_features(self, audio, sample_rate=None) -> np.ndarray:
        """prepareInputFeatures (:212-246) -> [n_mels, frames] float32 (HF layout).  The C ABI has no features-only call: this runs a
        whole one-row `predict` and reads its stage-1 tap, so it replaces the handle's last-call taps, timing and launch count."""
        self.predict_raw([audio], sample_rate)
        return np.ascontiguousarray(self.tap(1)[0].T)

    def __call__(self, features, return_logits: bool = False) -> np.ndarray:
        """callAsFunction (:180-202): features [n_mels, frames] or [batch, n_mels, frames] -> [batch, 1] probabilities (or logits)."""
        f = np.ascontiguousarray(features, dtype=np.float32)
        if f.ndim == 2:
            f = f[None]
        want = (self.config.encoder_config.num_mel_bins, self.config.frames)
        if f.ndim != 3 or f.shape[1:] != want:
            raise AudioGenerationError(3, f"Smart Turn: features of shape {f.shape}, expected [batch, {want[0]}, {want[1]}]")
        B = f.shape[0]
        prob, logit = np.zeros(B, np.float32), np.zeros(B, np.float32)
        check(_lib.lib().mis_smartturn_forward_features(self._h, f.ctypes.data, B, prob.ctypes.data, logit.ctypes.data))
        self._last_batch = B
        return (logit if return_logits else prob)[:, None]

    def tap(self, stage: int) -> np.ndarray:
        """Tensors of the last call: 0 prepared samples [B, W], 1 features [B, F, n_mels], 2 encoder output [B, T, d], 3 pooled [B, d]."""
        c = self.config
        shape = {0: (c.window_samples,), 1: (c.frames, c.encoder_config.num_mel_bins), 2: (c.positions, c.encoder_config.d_model),
                 3: (c.encoder_config.d_model,)}[stage]
        if not self._last_batch:
            raise AudioGenerationError(3, "Smart Turn: no call to tap")
        out = np.zeros((self._last_batch,) + shape, np.float32)
        check(_lib.lib().mis_debug_smartturn_tap(self._h, stage, out.ctypes.data, out.size))
        return out

    def timing(self):
        """Device milliseconds of the last call: (prepare + mel, encoder, head); inside a graph replay (encoder + head, -1)."""
        ms = (C.c_float * 3)()
        check(_lib.lib().mis_debug_smartturn_timing(self._h, ms))
        return tuple(float(v) for v in ms)
