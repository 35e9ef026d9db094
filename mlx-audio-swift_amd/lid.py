"""Spoken language identification, host mirror of `EcapaTdnn` (Sources/MLXAudioLID/Models/EcapaTdnn/EcapaTdnnLID.swift:13-195,
EcapaTdnnConfig.swift:8-89, LIDOutput.swift).  Configuration, checkpoint key mapping, labels and the ragged-batch packing stay on the
host; the SpeechBrain mel front end, the ECAPA-TDNN backbone, the classifier and the top-k run in libmi_speech.so
(csrc/ecapa_lid.hip)."""
from __future__ import annotations

import ctypes as C
import json
import os
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._handle import NativeHandle, pack_rows, read_safetensors_dir
from .generation import AudioGenerationError, check

SAMPLE_RATE, HOP_LENGTH = 16000, 160                              # EcapaMelSpectrogram.swift:5-9

_JSON_KEYS = ("n_mels", "channels", "kernel_sizes", "dilations", "attention_channels", "res2net_scale", "se_channels", "embedding_dim",
              "classifier_hidden_dim", "num_classes", "id2label")


class LIDError(AudioGenerationError):
    """LIDError (LIDOutput.swift:25-39): `.lid_case` is configNotFound, weightsNotFound or noLabels."""

    def __init__(self, lid_case: str, message: str):
        self.lid_case = lid_case
        super().__init__(1, message)


@dataclass
class EcapaTdnnConfig:
    """EcapaTdnnConfig (EcapaTdnnConfig.swift:8-74), every field, default and JSON key.  num_classes None: len(id2label), else 107.
    max_batch / max_samples size the engine's workspace and are not part of a checkpoint."""
    n_mels: int = 60
    channels: int = 1024
    kernel_sizes: list = field(default_factory=lambda: [5, 3, 3, 3, 1])
    dilations: list = field(default_factory=lambda: [1, 2, 3, 4, 1])
    attention_channels: int = 128
    res2net_scale: int = 8
    se_channels: int = 128
    embedding_dim: int = 256
    classifier_hidden_dim: int = 512
    num_classes: int | None = None
    id2label: dict | None = None
    max_batch: int = 8
    max_samples: int = 30 * SAMPLE_RATE

    def __post_init__(self):
        if self.num_classes is None:                              # :47
            self.num_classes = len(self.id2label) if self.id2label is not None else 107

    @classmethod
    def from_dict(cls, d: dict, **workspace) -> "EcapaTdnnConfig":
        """init(from:) (:35-48): missing or null keys take the defaults, unknown keys are ignored."""
        return cls(**{k: d[k] for k in _JSON_KEYS if d.get(k) is not None}, **workspace)

    def to_c(self) -> "_lib.EcapaLidConfigC":
        if len(self.kernel_sizes) != 5 or len(self.dilations) != 5:
            raise AudioGenerationError(3, "ECAPA LID: kernel_sizes and dilations have five entries each")
        return _lib.EcapaLidConfigC(self.n_mels, self.channels, (C.c_int32 * 5)(*self.kernel_sizes), (C.c_int32 * 5)(*self.dilations),
                                    self.attention_channels, self.res2net_scale, self.se_channels, self.embedding_dim,
                                    self.classifier_hidden_dim, self.num_classes, self.max_batch, self.max_samples)


@dataclass
class LanguagePrediction:                                         # LIDOutput.swift:3-11
    language: str
    confidence: float


@dataclass
class LIDOutput:                                                  # LIDOutput.swift:13-23
    language: str
    confidence: float
    top_languages: list


_RENAMES = (("embedding_model.blocks.0.", "embedding_model.block0."), ("embedding_model.blocks.1.", "embedding_model.block1."),
            ("embedding_model.blocks.2.", "embedding_model.block2."), ("embedding_model.blocks.3.", "embedding_model.block3."),
            (".conv.conv.", ".conv."), (".norm.norm.", ".norm."), (".se_block.conv1.conv.", ".se_block.conv1."),
            (".se_block.conv2.conv.", ".se_block.conv2."), (".asp_bn.norm.", ".asp_bn."), (".fc.conv.", ".fc."))


def ecapa_lid_sanitize(weights: dict) -> dict:
    """EcapaTdnn.sanitize (EcapaTdnnLID.swift:99-131): num_batches_tracked dropped, the top-level `blocks.N` renamed to `blockN` (the
    Res2Net `blocks.N` array is kept), SpeechBrain's double nesting flattened.  Layouts are untouched: conv weights are [out, k, in]."""
    out = {}
    for key, v in weights.items():
        if "num_batches_tracked" in key:
            continue
        k = key
        for a, b in _RENAMES:
            k = k.replace(a, b)
        out[k] = v
    return out


def _bn(p):
    return {p + ".weight", p + ".bias", p + ".running_mean", p + ".running_var"}


def ecapa_lid_expected_shapes(config: EcapaTdnnConfig) -> dict:
    """name -> shape of every parameter of EcapaTdnn(config): what update(parameters:verify: .all) accepts (:187-189)."""
    c, h = config.channels, config.channels // config.res2net_scale
    s = {}

    def bn(p, n):
        for k in _bn(p):
            s[k] = (n,)

    def tdnn(p, cin, cout, k):
        s[p + ".conv.weight"], s[p + ".conv.bias"] = (cout, k, cin), (cout,)
        bn(p + ".norm", cout)

    e = "embedding_model."
    tdnn(e + "block0", config.n_mels, c, config.kernel_sizes[0])
    for i in (1, 2, 3):
        q = f"{e}block{i}."
        tdnn(q + "tdnn1", c, c, 1)
        for j in range(config.res2net_scale - 1):
            tdnn(f"{q}res2net_block.blocks.{j}", h, h, config.kernel_sizes[i])
        tdnn(q + "tdnn2", c, c, 1)
        s[q + "se_block.conv1.weight"], s[q + "se_block.conv1.bias"] = (config.se_channels, 1, c), (config.se_channels,)
        s[q + "se_block.conv2.weight"], s[q + "se_block.conv2.bias"] = (c, 1, config.se_channels), (c,)
    tdnn(e + "mfa", 3 * c, 3 * c, config.kernel_sizes[4])
    tdnn(e + "asp.tdnn", 9 * c, config.attention_channels, 1)
    s[e + "asp.conv.weight"], s[e + "asp.conv.bias"] = (3 * c, 1, config.attention_channels), (3 * c,)
    bn(e + "asp_bn", 6 * c)
    s[e + "fc.weight"], s[e + "fc.bias"] = (config.embedding_dim, 1, 6 * c), (config.embedding_dim,)
    bn("classifier.norm", config.embedding_dim)
    s["classifier.DNN.block_0.linear.w.weight"] = (config.classifier_hidden_dim, config.embedding_dim)
    s["classifier.DNN.block_0.linear.w.bias"] = (config.classifier_hidden_dim,)
    bn("classifier.DNN.block_0.norm", config.classifier_hidden_dim)
    s["classifier.out.w.weight"], s["classifier.out.w.bias"] = (config.num_classes, config.classifier_hidden_dim), (config.num_classes,)
    return s


def ecapa_lid_labels(id2label: dict | None) -> dict:
    """index -> the text in front of ":", trimmed (EcapaTdnnLID.swift:23-33); keys that are no integers are dropped."""
    out = {}
    for k, v in (id2label or {}).items():
        try:
            out[int(k)] = str(v).split(":")[0].strip()
        except ValueError:
            pass
    return out


def ecapa_lid_read_directory(model_dir: str, **workspace):
    """config.json and every *.safetensors of a model directory in name order, later files winning (fromModelDirectory, :158-194) ->
    (EcapaTdnnConfig, sanitized weights).  No device is touched.  Raises the reference's three errors, and invalidInput for keys or
    shapes the model does not have."""
    path = os.path.join(model_dir, "config.json")
    if not os.path.isfile(path):
        raise LIDError("configNotFound", "config.json not found in model directory")
    with open(path) as f:
        cfg = EcapaTdnnConfig.from_dict(json.load(f), **workspace)
    if cfg.id2label is None:
        raise LIDError("noLabels", "No id2label mapping found in config")
    missing = LIDError("weightsNotFound", "No .safetensors files found in model directory")
    weights = ecapa_lid_sanitize(read_safetensors_dir(model_dir, missing_code=missing))
    want = ecapa_lid_expected_shapes(cfg)
    unknown, missing = sorted(set(weights) - set(want)), sorted(set(want) - set(weights))
    if unknown or missing:
        raise AudioGenerationError(3, f"ECAPA LID checkpoint: unknown keys {unknown[:4]}, missing keys {missing[:4]}")
    bad = [k for k in want if tuple(weights[k].shape) != want[k]]
    if bad:
        raise AudioGenerationError(3, f"ECAPA LID checkpoint: {bad[0]} has shape {tuple(weights[bad[0]].shape)}, expected {want[bad[0]]}")
    return cfg, weights


class EcapaTdnnLID(NativeHandle):
    """predict / callAsFunction of the reference class, plus ragged batches; one handle, 1..max_batch rows a call."""
    _prefix = "mis_ecapa_lid"

    def __init__(self, config: EcapaTdnnConfig, device: int = 0):
        self.config = config
        self.device = device
        self.id2label = ecapa_lid_labels(config.id2label)
        self._create(config.to_c(), device)

    @classmethod
    def from_weights(cls, config: EcapaTdnnConfig, weights: dict, device: int = 0) -> "EcapaTdnnLID":
        """weights: sanitized names (what ecapa_lid_sanitize returns)."""
        m = cls(config, device)
        for name, arr in weights.items():
            m.set_tensor(name, arr)
        m.finalize()
        return m

    @classmethod
    def synthetic(cls, config: EcapaTdnnConfig, device: int = 0, seed: int = 777) -> "EcapaTdnnLID":
        m = cls(config, device)
        check(_lib.lib().mis_ecapa_lid_init_synthetic(m._h, seed))
        m.finalize()
        return m

    @classmethod
    def from_model_directory(cls, model_dir: str, device: int = 0, **workspace) -> "EcapaTdnnLID":
        cfg, weights = ecapa_lid_read_directory(model_dir, **workspace)
        return cls.from_weights(cfg, weights, device)

    sanitize = staticmethod(ecapa_lid_sanitize)

    @property
    def launches(self) -> int:
        return int(_lib.lib().mis_ecapa_lid_launches(self._h))

    # -- calls ---------------------------------------------------------------------------------------
    def _k(self, top_k: int) -> int:
        return max(0, min(int(top_k), self.config.num_classes))

    def predict_raw(self, waveforms, top_k: int = 5, junk: float | None = None):
        """Ragged list of 1-D waveforms -> (log_probs [B, classes], embedding [B, E], top_idx [B, k] int32, top_prob [B, k]); `junk`
        fills the padding behind every row (tests)."""
        rows = [np.asarray(w, np.float32) for w in waveforms]
        if not rows or any(r.ndim != 1 for r in rows):
            raise AudioGenerationError(3, "ECAPA LID: a non-empty list of one-dimensional waveforms is expected")
        pcm, lens = pack_rows(rows, junk)
        B, stride = pcm.shape
        return self._run(lambda *o: _lib.lib().mis_ecapa_lid_predict(self._h, pcm.ctypes.data, lens.ctypes.data, B, stride, *o), B, top_k)

    def _run(self, call, B, top_k):
        c, k = self.config, self._k(top_k)
        logp, emb = np.zeros((B, c.num_classes), np.float32), np.zeros((B, c.embedding_dim), np.float32)
        idx, prob = np.zeros((B, k), np.int32), np.zeros((B, k), np.float32)
        check(call(int(top_k), logp.ctypes.data, emb.ctypes.data, idx.ctypes.data if k else None, prob.ctypes.data if k else None))
        return logp, emb, idx, prob

    def _output(self, idx, prob) -> LIDOutput:
        top = [LanguagePrediction(self.id2label.get(int(i), f"unknown_{int(i)}"), float(p)) for i, p in zip(idx, prob)]
        best = top[0] if top else LanguagePrediction("unknown", 0.0)
        return LIDOutput(best.language, best.confidence, top)

    def predict_batch(self, waveforms, top_k: int = 5) -> list:
        _, _, idx, prob = self.predict_raw(waveforms, top_k)
        return [self._output(i, p) for i, p in zip(idx, prob)]

    def predict(self, waveform, top_k: int = 5) -> LIDOutput:
        """predict(waveform:topK:) (:56-81): one 16 kHz mono waveform."""
        return self.predict_batch([waveform], top_k)[0]

    def embed(self, waveforms) -> np.ndarray:
        """The backbone's embeddings [B, embedding_dim] of a ragged list of waveforms."""
        return self.predict_raw(waveforms, 0)[1]

    def forward_features(self, mel_features, frames=None, top_k: int = 0):
        """mel dB [T, n_mels] or [B, T, n_mels], frames[B] valid frames each (None: T) -> the tuple of predict_raw."""
        f = np.ascontiguousarray(mel_features, dtype=np.float32)
        if f.ndim == 2:
            f = f[None]
        if f.ndim != 3 or f.shape[2] != self.config.n_mels:
            raise AudioGenerationError(3, f"ECAPA LID: features of shape {f.shape}, expected [batch, frames, {self.config.n_mels}]")
        B, T = f.shape[0], f.shape[1]
        fr = None if frames is None else np.ascontiguousarray(frames, dtype=np.int32)
        if fr is not None and fr.shape != (B,):
            raise AudioGenerationError(3, "ECAPA LID: one frame count per row is expected")
        return self._run(lambda *o: _lib.lib().mis_ecapa_lid_forward_features(self._h, f.ctypes.data, None if fr is None else fr.ctypes.data,
                                                                             B, T, *o), B, top_k)

    def __call__(self, mel_features, frames=None) -> np.ndarray:
        """callAsFunction (:42-46): mel [batch, time, n_mels] -> log-probabilities [batch, classes]."""
        return self.forward_features(mel_features, frames)[0]

    def tap(self, stage: int) -> np.ndarray:
        """Tensors of the last call: 0 mel dB [B, Ts, n_mels], 1 normalised features, 2 block0 [B, Ts, C], 3-5 the SE-Res2Net blocks,
        6 mfa [B, Ts, 3 C], 7 pooled [B, 6 C], 8 embedding [B, E], 9 log-probabilities [B, classes]; zeros behind a row's own frames."""
        dims = (C.c_int64 * 3)()
        check(_lib.lib().mis_ecapa_lid_tap(self._h, stage, None, 0, dims))
        out = np.zeros(tuple(int(d) for d in dims), np.float32)
        check(_lib.lib().mis_ecapa_lid_tap(self._h, stage, out.ctypes.data, out.size, dims))
        return out[:, 0] if stage >= 7 else out

    def timing(self):
        """Device milliseconds of the last call: (front end, model)."""
        ms = (C.c_float * 2)()
        check(_lib.lib().mis_debug_ecapa_lid_timing(self._h, ms))
        return float(ms[0]), float(ms[1])
