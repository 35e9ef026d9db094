"""LASR CTC speech-to-text, host mirror of `LasrCTCModel` (Sources/MLXAudioSTT/Models/LasrCTC/LasrCTCModel.swift:275-423,
LasrCTCConfig.swift:3-193) and of `SentencePieceTokenizer.decode` (MLXAudioCore/SentencePieceTokenizer.swift:565-596).  Configuration,
checkpoint key handling, the tokenizer and the ragged-batch packing stay on the host; the log-mel front end, the Conformer encoder, the
CTC head and the greedy collapse run in libmi_speech.so (csrc/lasr.hip).  No tensor arithmetic happens here."""
from __future__ import annotations

import ctypes as C
import json
import os
import time
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._handle import NativeHandle, pack_rows, read_safetensors_dir
from .generation import AudioGenerationError, check
from .stt import STTGenerateParameters, STTOutput

LASR_SAMPLE_RATE, LASR_HOP = 16000, 160

_ENC_KEYS = ("hidden_size", "num_hidden_layers", "num_attention_heads", "num_key_value_heads", "intermediate_size", "hidden_act",
             "conv_kernel_size", "convolution_bias", "num_mel_bins", "subsampling_conv_channels", "subsampling_conv_kernel_size",
             "subsampling_conv_stride", "dropout", "attention_dropout", "activation_dropout", "layer_norm_eps", "batch_norm_momentum",
             "max_position_embeddings", "attention_bias", "rope_theta", "rope_type", "conv_residual_weights",
             "feed_forward_residual_weights")
_CTC_KEYS = ("vocab_size", "ctc_loss_reduction", "ctc_zero_infinity", "pad_token_id", "initializer_range", "model_type")


@dataclass
class LasrEncoderConfig:
    """LasrEncoderConfig (LasrCTCConfig.swift:3-144), every field and default."""
    hidden_size: int = 512
    num_hidden_layers: int = 17
    num_attention_heads: int = 8
    num_key_value_heads: int | None = None          # :115: the head count
    intermediate_size: int = 2048
    hidden_act: str = "silu"
    conv_kernel_size: int = 32
    convolution_bias: bool = False
    num_mel_bins: int = 128
    subsampling_conv_channels: int = 256
    subsampling_conv_kernel_size: int = 5
    subsampling_conv_stride: int = 2
    dropout: float = 0.1
    attention_dropout: float = 0.1
    activation_dropout: float = 0.1
    layer_norm_eps: float = 1e-6
    batch_norm_momentum: float = 0.01
    max_position_embeddings: int = 10000
    attention_bias: bool = False
    rope_theta: float = 10000.0
    rope_type: str = "default"
    conv_residual_weights: list = field(default_factory=lambda: [2.0, 1.0])
    feed_forward_residual_weights: list = field(default_factory=lambda: [1.5, 0.5])

    def __post_init__(self):
        if self.num_key_value_heads is None:
            self.num_key_value_heads = self.num_attention_heads

    @classmethod
    def from_dict(cls, d: dict) -> "LasrEncoderConfig":
        """init(from:) (:110-143): missing or null keys take the defaults; `rope_parameters` overrides rope_theta / rope_type."""
        kw = {k: d[k] for k in _ENC_KEYS if d.get(k) is not None}
        rope = d.get("rope_parameters")
        if isinstance(rope, dict):
            for k in ("rope_theta", "rope_type"):
                if rope.get(k) is not None:
                    kw[k] = rope[k]
        return cls(**kw)


@dataclass
class LasrCTCConfig:
    """LasrCTCConfig (LasrCTCConfig.swift:146-193).  max_batch / max_seconds size the engine's workspace and are not part of a
    checkpoint."""
    vocab_size: int = 512
    encoder_config: LasrEncoderConfig = field(default_factory=LasrEncoderConfig)
    ctc_loss_reduction: str = "mean"
    ctc_zero_infinity: bool = True
    pad_token_id: int = 0
    initializer_range: float = 0.02
    model_type: str = "lasr"
    max_batch: int = 8
    max_seconds: int = 30

    @classmethod
    def from_dict(cls, d: dict, **workspace) -> "LasrCTCConfig":
        kw = {k: d[k] for k in _CTC_KEYS if d.get(k) is not None}
        if isinstance(d.get("encoder_config"), dict):
            kw["encoder_config"] = LasrEncoderConfig.from_dict(d["encoder_config"])
        return cls(**kw, **workspace)

    def to_c(self) -> "_lib.LasrConfigC":
        e = self.encoder_config
        if len(e.conv_residual_weights) != 2 or len(e.feed_forward_residual_weights) != 2:
            raise AudioGenerationError(3, "LASR: conv_residual_weights and feed_forward_residual_weights have two entries each")
        return _lib.LasrConfigC(
            self.vocab_size, e.hidden_size, e.num_hidden_layers, e.num_attention_heads, e.num_key_value_heads, e.intermediate_size,
            1 if e.hidden_act.lower() == "relu" else 0, e.conv_kernel_size, int(e.convolution_bias), e.num_mel_bins,
            e.subsampling_conv_channels, e.subsampling_conv_kernel_size, e.subsampling_conv_stride, int(e.attention_bias),
            0 if e.rope_type == "default" else 1, self.pad_token_id, self.max_batch, self.max_seconds, e.layer_norm_eps, e.rope_theta,
            (C.c_float * 2)(*e.conv_residual_weights), (C.c_float * 2)(*e.feed_forward_residual_weights))


def lasr_sanitize(weights: dict) -> dict:
    """LasrCTCModel.sanitize (:352-367): `rotary_emb.inv_freq` and `num_batches_tracked` dropped, 3-D `*.weight` whose key contains
    `conv` transposed (0, 2, 1) to [out, k, in], a 3-D `ctc_head.weight` squeezed."""
    out = {}
    for key, v in weights.items():
        if "rotary_emb.inv_freq" in key or key.endswith("num_batches_tracked"):
            continue
        if "conv" in key and key.endswith(".weight") and v.ndim == 3:
            v = v.transpose(0, 2, 1) if isinstance(v, np.ndarray) else v.permute(0, 2, 1)
        if key == "ctc_head.weight" and v.ndim == 3:
            v = v[:, :, 0]
        out[key] = v
    return out


def lasr_expected_keys(config: LasrCTCConfig) -> set:
    """Every parameter name of LasrCTCModel(config): what update(parameters:verify: .noUnusedKeys) accepts (:401)."""
    e = config.encoder_config
    keys = set()

    def lin(p, bias=True):
        keys.add(p + ".weight")
        if bias:
            keys.add(p + ".bias")

    for n in ("dense_0", "conv_0", "conv_1", "dense_1"):
        lin("encoder.subsampler." + n)
    for i in range(e.num_hidden_layers):
        q = f"encoder.layers.{i}."
        for n in ("norm_feed_forward1", "norm_self_att", "norm_conv", "norm_feed_forward2", "norm_out"):
            lin(q + n)
        for n in ("feed_forward1", "feed_forward2"):
            lin(q + n + ".linear1", e.attention_bias)
            lin(q + n + ".linear2", e.attention_bias)
        for n in ("q_proj", "k_proj", "v_proj", "o_proj"):
            lin(q + "self_attn." + n, e.attention_bias)
        for n in ("pointwise_conv1", "depthwise_conv", "pointwise_conv2"):
            lin(q + "conv." + n, e.convolution_bias)
        keys.update(q + "conv.norm." + n for n in ("weight", "bias", "running_mean", "running_var"))
    lin("encoder.out_norm")
    lin("ctc_head")
    return keys


class SentencePieceTokenizer:
    """The decode side of SentencePieceTokenizer (SentencePieceTokenizer.swift:565-596), built from tokenizer.json's `model.vocab`
    (a list of [piece, score] or a piece -> id map); `added_tokens` marked special are control pieces."""

    def __init__(self, pieces: list, control: set | None = None):
        self.pieces = list(pieces)
        self.control = set(control or ())

    @classmethod
    def from_tokenizer_json(cls, path: str) -> "SentencePieceTokenizer":
        with open(path, encoding="utf-8") as f:
            d = json.load(f)
        vocab = d["model"]["vocab"]
        if isinstance(vocab, dict):
            pieces = [None] * (max(vocab.values()) + 1)
            for tok, i in vocab.items():
                pieces[i] = tok
            pieces = [p if p is not None else "" for p in pieces]
        else:
            pieces = [v[0] if isinstance(v, (list, tuple)) else str(v) for v in vocab]
        control = {int(t["id"]) for t in d.get("added_tokens", []) if t.get("special")}
        return cls(pieces, control)

    def decode(self, ids) -> str:
        raw, out = bytearray(), []

        def flush():
            if raw:
                try:
                    out.append(raw.decode("utf-8"))
                except UnicodeDecodeError:
                    pass
                raw.clear()

        for i in ids:
            i = int(i)
            if i < 0 or i >= len(self.pieces) or i in self.control:
                continue
            tok = self.pieces[i]
            if tok.startswith("<0x") and tok.endswith(">") and len(tok) == 6:
                try:
                    raw.append(int(tok[3:5], 16))
                except ValueError:
                    pass
                continue
            flush()
            out.append(tok)
        flush()
        return "".join(out).replace("▁", " ").strip(" \t")


def greedy_ctc_tokens(logits, blank_token_id: int = 0, frames=None) -> list:
    """Wav2Vec2CTCModel.greedyCTCTokens (Wav2Vec2CTC.swift:520-542) on logits [B, T, V]: per-frame arg-max (lowest index on ties), a
    token is kept when it differs from the previous frame's and is not the blank.  frames[B]: each row's own frame count."""
    pred = np.argmax(np.asarray(logits), axis=-1)
    rows = []
    for b in range(pred.shape[0]):
        prev, row = -1, []
        for t in range(pred.shape[1] if frames is None else int(frames[b])):
            tok = int(pred[b, t])
            if tok != prev and tok != blank_token_id:
                row.append(tok)
            prev = tok
        rows.append(row)
    return rows


class LasrCTCModel(NativeHandle):
    """generate / generateStream / callAsFunction of the reference class, plus ragged batches; one handle, 1..max_batch rows a call."""
    _prefix = "mis_lasr"

    def __init__(self, config: LasrCTCConfig, tokenizer: SentencePieceTokenizer | None = None, device: int = 0):
        self.config, self.tokenizer, self.device = config, tokenizer, device
        self._create(config.to_c(), device)

    default_generation_parameters = STTGenerateParameters(max_tokens=0, temperature=0.0, language=None)      # :282-284
    sanitize = staticmethod(lasr_sanitize)
    greedy_ctc_tokens = staticmethod(greedy_ctc_tokens)

    @classmethod
    def from_weights(cls, config: LasrCTCConfig, weights: dict, tokenizer=None, device: int = 0) -> "LasrCTCModel":
        """weights: sanitized names (what lasr_sanitize returns)."""
        m = cls(config, tokenizer, device)
        for name, arr in weights.items():
            m.set_tensor(name, arr)
        m.finalize()
        return m

    @classmethod
    def synthetic(cls, config: LasrCTCConfig, device: int = 0, seed: int = 777) -> "LasrCTCModel":
        m = cls(config, None, device)
        check(_lib.lib().mis_lasr_init_synthetic(m._h, seed))
        m.finalize()
        return m

    @classmethod
    def from_model_directory(cls, model_dir: str, device: int = 0, **workspace) -> "LasrCTCModel":
        """fromModelDirectory (:391-423): config.json, tokenizer.json if it is there and loads, every *.safetensors in name order with
        later files winning; keys the model does not have are rejected."""
        with open(os.path.join(model_dir, "config.json")) as f:
            config = LasrCTCConfig.from_dict(json.load(f), **workspace)
        tokenizer, tpath = None, os.path.join(model_dir, "tokenizer.json")
        if os.path.isfile(tpath):
            try:
                tokenizer = SentencePieceTokenizer.from_tokenizer_json(tpath)
            except Exception:                                     # `try?`: a tokenizer that does not load is no error
                tokenizer = None
        weights = lasr_sanitize(read_safetensors_dir(model_dir, missing_code=(2, f"No safetensors files found in {model_dir}")))
        unknown = sorted(set(weights) - lasr_expected_keys(config))
        if unknown:
            raise AudioGenerationError(3, f"LASR checkpoint: unused keys {unknown[:4]}")
        return cls.from_weights(config, weights, tokenizer, device)

    @property
    def launches(self) -> int:
        return int(_lib.lib().mis_lasr_launches(self._h))

    # -- calls ---------------------------------------------------------------------------------------
    def frames(self, lens):
        """(F, T2) of rows of `lens` samples; T2 0: too short for the stem."""
        n = np.ascontiguousarray(lens, dtype=np.int64)
        F, T2 = np.zeros(len(n), np.int32), np.zeros(len(n), np.int32)
        check(_lib.lib().mis_lasr_frames(self._h, n.ctypes.data, len(n), F.ctypes.data, T2.ctypes.data))
        return F, T2

    @staticmethod
    def _pack(audios, junk=None):
        rows = [np.asarray(w, np.float32) for w in audios]
        if not rows or any(r.ndim != 1 for r in rows):
            raise AudioGenerationError(3, "LASR: a non-empty list of one-dimensional waveforms is expected")
        return pack_rows(rows, junk)

    def features(self, audios, junk=None) -> np.ndarray:
        """Normalised log-mel features [B, Fmax, mels] of a ragged list of waveforms, zeros behind a row's own frames; `junk` fills the
        padding behind every row (tests)."""
        pcm, lens = self._pack(audios, junk)
        F, _ = self.frames(lens)
        out = np.zeros((len(lens), int(F.max()), self.config.encoder_config.num_mel_bins), np.float32)
        check(_lib.lib().mis_lasr_features(self._h, pcm.ctypes.data, lens.ctypes.data, len(lens), pcm.shape[1], out.ctypes.data))
        return out

    def forward(self, audios, junk=None) -> np.ndarray:
        """Logits [B, T2max, vocab] of a ragged list of waveforms, zeros behind a row's own T2."""
        pcm, lens = self._pack(audios, junk)
        _, T2 = self.frames(lens)
        out = np.zeros((len(lens), max(1, int(T2.max())), self.config.vocab_size), np.float32)
        check(_lib.lib().mis_lasr_forward(self._h, pcm.ctypes.data, lens.ctypes.data, len(lens), pcm.shape[1], out.ctypes.data))
        return out

    def _t2(self, F: int) -> int:
        e = self.config.encoder_config
        k, s = e.subsampling_conv_kernel_size, e.subsampling_conv_stride
        t1 = (F - k) // s + 1 if F >= k else 0
        return (t1 - k) // s + 1 if t1 >= k else 0

    def __call__(self, features, frames=None) -> np.ndarray:
        """callAsFunction (:294-296): features [B, F, mels] (or [F, mels]) -> logits [B, T2, vocab]; frames[B]: valid frames a row."""
        f = np.ascontiguousarray(features, dtype=np.float32)
        if f.ndim == 2:
            f = f[None]
        if f.ndim != 3 or f.shape[2] != self.config.encoder_config.num_mel_bins:
            raise AudioGenerationError(3, f"LASR: features of shape {f.shape}, expected [batch, frames, num_mel_bins]")
        B, F = f.shape[0], f.shape[1]
        fr = None if frames is None else np.ascontiguousarray(frames, dtype=np.int32)
        out = np.zeros((B, max(1, self._t2(F)), self.config.vocab_size), np.float32)
        check(_lib.lib().mis_lasr_forward_features(self._h, f.ctypes.data, None if fr is None else fr.ctypes.data, B, F, out.ctypes.data))
        return out

    def generate_tokens(self, audios, junk=None) -> list:
        """Greedy CTC ids of a ragged list of waveforms, collapsed on the device."""
        pcm, lens = self._pack(audios, junk)
        _, T2 = self.frames(lens)
        stride = max(1, int(T2.max()))
        toks, n = np.zeros((len(lens), stride), np.int32), np.zeros(len(lens), np.int32)
        check(_lib.lib().mis_stt_lasr_generate(self._h, pcm.ctypes.data, lens.ctypes.data, len(lens), pcm.shape[1], toks.ctypes.data,
                                               stride, n.ctypes.data))
        return [toks[b, : n[b]].tolist() for b in range(len(lens))]

    def _prepare(self, audio):
        """prepareFeatures (:331-350): 3-D with last dim = mels passes through, 2-D with second dim = mels gets a batch axis (both are
        features); anything else is a waveform, multi-channel audio averaged over the last axis."""
        a = np.asarray(audio, np.float32)
        mels = self.config.encoder_config.num_mel_bins
        if a.ndim == 3 and a.shape[2] == mels:
            return "features", a
        if a.ndim == 2 and a.shape[1] == mels:
            return "features", a[None]
        return "audio", (a.mean(axis=-1, dtype=np.float32) if a.ndim > 1 else a)

    def decode_text(self, tokens) -> str:
        return self.tokenizer.decode(tokens) if self.tokenizer is not None else " ".join(str(t) for t in tokens)

    def _output(self, tokens, language, seconds) -> STTOutput:
        text = self.decode_text(tokens)
        return STTOutput(text=text, segments=[{"text": text, "start": 0.0, "end": 0.0}], language=language, prompt_tokens=0,
                         generation_tokens=len(tokens), total_tokens=len(tokens), prompt_tps=0.0,
                         generation_tps=len(tokens) / max(seconds, 0.001), total_time=seconds, peak_memory_usage=0.0,
                         token_ids=[list(tokens)])

    def generate_batch(self, audios, generation_parameters=None) -> list:
        start = time.perf_counter()
        prepared = [self._prepare(a) for a in audios]
        if any(kind != "audio" for kind, _ in prepared):
            raise AudioGenerationError(3, "LASR generate_batch takes waveforms; pass prepared features to generate, one request a call")
        rows = self.generate_tokens([a for _, a in prepared])
        seconds = time.perf_counter() - start
        language = getattr(generation_parameters, "language", None)
        return [self._output(r, language, seconds) for r in rows]

    def generate(self, audio, generation_parameters=None) -> STTOutput:
        """generate (:298-315): a waveform, or already-prepared features."""
        start = time.perf_counter()
        kind, a = self._prepare(audio)
        if kind == "audio":
            tokens = self.generate_tokens([a])[0]
        else:
            tokens = greedy_ctc_tokens(self(a), self.config.pad_token_id)[0]
        return self._output(tokens, getattr(generation_parameters, "language", None), time.perf_counter() - start)

    def generate_stream(self, audio, generation_parameters=None):
        """generateStream (:317-329): ("token", text) if the text is not empty, then ("result", STTOutput)."""
        out = self.generate(audio, generation_parameters)
        if out.text:
            yield ("token", out.text)
        yield ("result", out)

    def tap(self, stage: int) -> np.ndarray:
        """Tensors of the last call [B, T2max, hidden]: 0 the stem's output, 1..L that block's output, L + 1 out_norm; zero rows behind a
        row's own T2."""
        dims = (C.c_int64 * 3)()
        check(_lib.lib().mis_lasr_tap(self._h, stage, None, 0, dims))
        out = np.zeros(tuple(int(d) for d in dims), np.float32)
        check(_lib.lib().mis_lasr_tap(self._h, stage, out.ctypes.data, out.size, dims))
        return out

    def enable_timing(self):
        check(_lib.lib().mis_debug_lasr_timing(self._h, None))

    def timing(self):
        """Device milliseconds of the last generate: (front end, encoder, tail); enable_timing() first."""
        ms = (C.c_float * 3)()
        check(_lib.lib().mis_debug_lasr_timing(self._h, ms))
        return float(ms[0]), float(ms[1]), float(ms[2])
