"""Sortformer speaker diarization, host mirror of `SortformerModel` (Sources/MLXAudioVAD/Models/Sortformer/Sortformer.swift,
SortformerConfig.swift, SortformerFeatures.swift trimSilence, VADOutput.swift).  Configuration, checkpoint key handling, silence
trimming, segments and the streaming state (speaker cache, FIFO, AOSC compression: a few hundred frames once per chunk) stay on the
host in numpy; the log-mel front end, the stem, both encoders and the speaker sigmoids run in libmi_speech.so (csrc/sortformer.hip)."""
from __future__ import annotations

import ctypes as C
import json
import math
import os
import time
from dataclasses import dataclass, field, fields

import numpy as np

from . import _lib
from ._handle import NativeHandle, pack_rows, read_safetensors_dir
from .generation import AudioGenerationError, check


def _from(cls, d: dict):
    """decodeIfPresent of every field: missing or null keys take the defaults."""
    return cls(**{f.name: d[f.name] for f in fields(cls) if d.get(f.name) is not None and not isinstance(d[f.name], dict)})


@dataclass
class FCEncoderConfig:
    hidden_size: int = 512
    num_hidden_layers: int = 18
    num_attention_heads: int = 8
    num_key_value_heads: int = 8
    intermediate_size: int = 2048
    num_mel_bins: int = 80
    conv_kernel_size: int = 9
    subsampling_factor: int = 8
    subsampling_conv_channels: int = 256
    subsampling_conv_kernel_size: int = 3
    subsampling_conv_stride: int = 2
    max_position_embeddings: int = 5000
    attention_bias: bool = True
    scale_input: bool = True


@dataclass
class TFEncoderConfig:
    d_model: int = 192
    encoder_layers: int = 18
    encoder_attention_heads: int = 8
    encoder_ffn_dim: int = 768
    layer_norm_eps: float = 1e-5
    max_source_positions: int = 1500
    k_proj_bias: bool = False


@dataclass
class ModulesConfig:
    num_speakers: int = 4
    fc_d_model: int = 512
    tf_d_model: int = 192
    subsampling_factor: int = 8
    chunk_len: int = 188
    fifo_len: int = 0
    spkcache_len: int = 188
    spkcache_update_period: int = 188
    chunk_left_context: int = 1
    chunk_right_context: int = 1
    spkcache_sil_frames_per_spk: int = 5
    pred_score_threshold: float = 1e-6
    max_index: int = 10000
    scores_boost_latest: float = 0.5
    sil_threshold: float = 0.1
    strong_boost_rate: float = 0.3
    weak_boost_rate: float = 0.7
    min_pos_scores_rate: float = 0.5
    use_aosc: bool = False


@dataclass
class ProcessorConfig:
    feature_size: int = 80
    sampling_rate: int = 16000
    hop_length: int = 160
    n_fft: int = 512
    win_length: int = 400
    preemphasis: float = 0.97


@dataclass
class SortformerConfig:
    """SortformerConfig (SortformerConfig.swift:191-217).  A nested config that is absent is decoded from the top-level dictionary (the
    flat-config fallback).  max_batch / max_seconds size the engine's workspace and are not part of a checkpoint."""
    model_type: str = "sortformer"
    num_speakers: int = 4
    fc_encoder_config: FCEncoderConfig = field(default_factory=FCEncoderConfig)
    tf_encoder_config: TFEncoderConfig = field(default_factory=TFEncoderConfig)
    modules_config: ModulesConfig = field(default_factory=ModulesConfig)
    processor_config: ProcessorConfig = field(default_factory=ProcessorConfig)
    max_batch: int = 8
    max_seconds: int = 90

    @classmethod
    def from_dict(cls, d: dict, **workspace) -> "SortformerConfig":
        kw = {k: d[k] for k in ("model_type", "num_speakers") if d.get(k) is not None}
        for name, sub in (("fc_encoder_config", FCEncoderConfig), ("tf_encoder_config", TFEncoderConfig), ("modules_config", ModulesConfig),
                          ("processor_config", ProcessorConfig)):
            kw[name] = _from(sub, d[name] if isinstance(d.get(name), dict) else d)
        return cls(**kw, **workspace)

    def to_c(self) -> "_lib.SortformerConfigC":
        e, t, m, p = self.fc_encoder_config, self.tf_encoder_config, self.modules_config, self.processor_config
        if p.feature_size != e.num_mel_bins:
            raise AudioGenerationError(3, f"Sortformer: feature_size {p.feature_size} differs from num_mel_bins {e.num_mel_bins}")
        return _lib.SortformerConfigC(
            e.hidden_size, e.num_hidden_layers, e.num_attention_heads, e.num_key_value_heads, e.intermediate_size, e.num_mel_bins,
            e.conv_kernel_size, e.subsampling_factor, e.subsampling_conv_channels, e.subsampling_conv_kernel_size, e.subsampling_conv_stride,
            int(e.attention_bias), int(e.scale_input), t.d_model, t.encoder_layers, t.encoder_attention_heads, t.encoder_ffn_dim,
            t.max_source_positions, int(t.k_proj_bias), m.num_speakers, m.fc_d_model, m.tf_d_model, p.sampling_rate, p.hop_length, p.n_fft,
            p.win_length, self.max_batch, self.max_seconds, t.layer_norm_eps, p.preemphasis)


def _perm(v, order):
    return v.transpose(*order) if isinstance(v, np.ndarray) else v.permute(*order)


def sortformer_sanitize(weights: dict) -> dict:
    """SortformerModel.sanitize (:1346-1382): `num_batches_tracked` skipped; unless a key already holds `subsampling.layers_` (an
    already converted checkpoint passes through): `fc_encoder.subsampling.layers.N` -> `layers_N`, 4-D subsampling conv weights
    (O, I, H, W) -> (O, H, W, I), 3-D pointwise / depthwise conv weights (O, I, K) -> (O, K, I)."""
    converted = any("subsampling.layers_" in k for k in weights)
    out = {}
    for k, v in weights.items():
        if "num_batches_tracked" in k:
            continue
        if not converted:
            if "fc_encoder.subsampling.layers." in k:
                k = k.replace("subsampling.layers.", "subsampling.layers_")
            if "subsampling" in k and "weight" in k and "linear" not in k and v.ndim == 4:
                v = _perm(v, (0, 2, 3, 1))
            if any(n in k for n in ("pointwise_conv1", "pointwise_conv2", "depthwise_conv")) and "weight" in k and v.ndim == 3:
                v = _perm(v, (0, 2, 1))
        out[k] = v
    return out


def sortformer_expected_keys(config: SortformerConfig) -> set:
    """Every parameter name of SortformerModel(config): what update(parameters:verify: .noUnusedKeys) accepts (:1428)."""
    e, t = config.fc_encoder_config, config.tf_encoder_config
    keys = set()

    def lin(p, bias=True):
        keys.add(p + ".weight")
        if bias:
            keys.add(p + ".bias")

    for n in ("layers_0", "layers_2", "layers_3", "layers_5", "layers_6", "linear"):
        lin("fc_encoder.subsampling." + n)
    for i in range(e.num_hidden_layers):
        q = f"fc_encoder.layers.{i}."
        for n in ("norm_feed_forward1", "norm_self_att", "norm_conv", "norm_feed_forward2", "norm_out", "feed_forward1.linear1",
                  "feed_forward1.linear2", "feed_forward2.linear1", "feed_forward2.linear2", "conv.pointwise_conv1", "conv.depthwise_conv",
                  "conv.pointwise_conv2"):
            lin(q + n)
        for n in ("q_proj", "k_proj", "v_proj", "o_proj"):
            lin(q + "self_attn." + n, e.attention_bias)
        lin(q + "self_attn.relative_k_proj", False)
        keys.update(q + "self_attn." + n for n in ("bias_u", "bias_v"))
        keys.update(q + "conv.norm." + n for n in ("weight", "bias", "running_mean", "running_var"))
    keys.add("tf_encoder.embed_positions.weight")
    for i in range(t.encoder_layers):
        q = f"tf_encoder.layers.{i}."
        for n in ("self_attn.q_proj", "self_attn.v_proj", "self_attn.out_proj", "self_attn_layer_norm", "fc1", "fc2", "final_layer_norm"):
            lin(q + n)
        lin(q + "self_attn.k_proj", t.k_proj_bias)
    for n in ("encoder_proj", "first_hidden_to_hidden", "single_hidden_to_spks", "hidden_to_spks"):
        lin("sortformer_modules." + n)
    return keys


@dataclass
class DiarizationSegment:
    start: float
    end: float
    speaker: int


@dataclass
class StreamingState:
    """StreamingState (VADOutput.swift:56-85) as numpy arrays: spkcache [1, n, emb], spkcache_preds [1, n, spk], fifo, fifo_preds,
    mean_sil_emb [1, emb], n_sil_frames [1]."""
    spkcache: np.ndarray
    spkcache_preds: np.ndarray
    fifo: np.ndarray
    fifo_preds: np.ndarray
    frames_processed: int
    mean_sil_emb: np.ndarray
    n_sil_frames: np.ndarray

    @property
    def spkcache_len(self) -> int:
        return int(self.spkcache.shape[1])

    @property
    def fifo_len(self) -> int:
        return int(self.fifo.shape[1])


@dataclass
class DiarizationOutput:
    segments: list
    speaker_probs: np.ndarray | None = None
    num_speakers: int = 0
    total_time: float = 0.0
    state: StreamingState | None = None

    @property
    def text(self) -> str:
        """RTTM, one line a segment (VADOutput.swift:42-51)."""
        return "\n".join(f"SPEAKER audio 1 {s.start:.3f} {np.float32(s.end) - np.float32(s.start):.3f} <NA> <NA> speaker_{s.speaker} <NA> <NA>"
                         for s in self.segments)


def trim_silence(waveform, sample_rate: int, frame_ms: int = 30, energy_ratio: float = 0.01, min_speech_sec: float = 0.5):
    """trimSilence (SortformerFeatures.swift:117-163): (trimmed waveform, offset in samples)."""
    w = np.asarray(waveform, np.float32)
    frame_len = int(np.float32(sample_rate) * np.float32(frame_ms) / np.float32(1000.0))
    min_frames = max(3, int(np.float32(min_speech_sec) * np.float32(1000.0) / np.float32(frame_ms)))
    n = len(w) // frame_len
    if n < min_frames * 2:
        return w, 0
    energy = np.sqrt(np.mean(np.square(w[: n * frame_len].reshape(n, frame_len)), axis=1, dtype=np.float32))
    speech = energy > np.float32(energy.max()) * np.float32(energy_ratio)
    start = 0
    for i in range(n - min_frames + 1):
        if speech[i: i + min_frames].all():
            start = i
            break
    end = n
    for i in range(n - 1, min_frames - 2, -1):
        if speech[i - min_frames + 1: i + 1].all():
            end = i + 1
            break
    a, b = start * frame_len, min(end * frame_len, len(w))
    if a == 0 and b == len(w):
        return w, 0
    return w[a:b], a


def preds_to_segments(preds, frame_duration: float, threshold: float = 0.5, min_duration: float = 0.0, merge_gap: float = 0.0) -> list:
    """predsToSegments (:1284-1342) on [frames, speakers]; times are float32 products, as in the reference."""
    p = np.asarray(preds, np.float32)
    fd, thr, md, mg = np.float32(frame_duration), np.float32(threshold), np.float32(min_duration), np.float32(merge_gap)
    out = []
    for spk in range(p.shape[1] if p.ndim == 2 else 0):
        segs, start = [], -1
        active = p[:, spk] > thr
        for f in range(p.shape[0] + 1):
            if f < p.shape[0] and active[f]:
                if start < 0:
                    start = f
            elif start >= 0:
                a, b = np.float32(start) * fd, np.float32(f) * fd
                if b - a >= md:
                    segs.append(DiarizationSegment(float(a), float(b), spk))
                start = -1
        if mg > 0 and len(segs) > 1:
            merged = [segs[0]]
            for s in segs[1:]:
                if np.float32(s.start) - np.float32(merged[-1].end) <= mg:
                    merged[-1] = DiarizationSegment(merged[-1].start, s.end, s.speaker)
                else:
                    merged.append(s)
            segs = merged
        out.extend(segs)
    out.sort(key=lambda s: s.start)
    return out


# ---------------------------------------------------------------------------------------------------- streaming state (numpy, float32)
_NEG_INF = np.float32(-np.inf)


def _top_k(flat: np.ndarray, k: int) -> np.ndarray:
    """Indices of the k largest entries of each row.  MLX leaves argPartition's order among equal scores unspecified; here ties go to
    the LOWER flat index (a stable sort of the negated scores)."""
    return np.argsort(-flat, axis=1, kind="stable")[:, :k]


def get_silence_profile(mean_sil_emb, n_sil_frames, embs, preds, sil_threshold):
    is_sil = (preds.sum(axis=2, dtype=np.float32) < np.float32(sil_threshold)).astype(np.float32)
    sil_count = is_sil.sum(axis=1, dtype=np.float32)
    sil_sum = (embs * is_sil[..., None]).sum(axis=1, dtype=np.float32)
    upd_n = (n_sil_frames + sil_count).astype(np.float32)
    total = mean_sil_emb * n_sil_frames[..., None] + sil_sum
    return (total / np.maximum(upd_n[..., None], np.float32(1))).astype(np.float32), upd_n


def get_log_pred_scores(preds, threshold):
    thr = np.float32(threshold)
    lp = np.log(np.maximum(preds, thr))
    l1 = np.log(np.maximum(np.float32(1.0) - preds, thr))
    return (lp - l1 + l1.sum(axis=2, keepdims=True, dtype=np.float32) - np.float32(math.log(0.5))).astype(np.float32)


def disable_low_scores(preds, scores, min_pos_scores_per_spk: int):
    is_speech = preds > np.float32(0.5)
    res = np.where(is_speech, scores, _NEG_INF)
    is_pos = res > 0
    enough = is_pos.astype(np.float32).sum(axis=1, keepdims=True, dtype=np.float32) >= np.float32(min_pos_scores_per_spk)
    return np.where(~is_pos & is_speech & enough, _NEG_INF, res).astype(np.float32)


def boost_topk_scores(scores, n_boost_per_spk: int, scale_factor: float = 1.0):
    if n_boost_per_spk <= 0:
        return scores
    n_frames = scores.shape[1]
    k = min(n_boost_per_spk, n_frames)
    boost = np.float32(-np.float32(scale_factor) * np.float32(math.log(0.5)))
    out = scores.copy()
    for spk in range(scores.shape[2]):
        flat = scores[:, :, spk]
        mask = np.zeros_like(flat)
        np.put_along_axis(mask, _top_k(flat, k), np.float32(1), axis=1)
        out[:, :, spk] = flat + mask * boost * (flat > _NEG_INF).astype(np.float32)
    return out


def get_topk_indices(scores, spkcache_len: int, sil_frames_per_spk: int, max_index: int):
    B, n_frames, _ = scores.shape
    flat = scores.transpose(0, 2, 1).reshape(B, -1)
    k = min(spkcache_len, flat.shape[1])
    idx = _top_k(flat, k)
    idx = np.where(np.take_along_axis(flat, idx, axis=1) > _NEG_INF, idx, max_index)
    idx = np.sort(idx, axis=1)
    disabled = idx == max_index
    idx = idx % n_frames
    disabled |= idx >= n_frames - sil_frames_per_spk
    return np.where(disabled, 0, idx), disabled


def compress_spkcache_aosc(embs, preds, mean_sil_emb, m: ModulesConfig):
    """compressSpkcacheAosc (:1216-1264)."""
    n_spk, L, sil = m.num_speakers, m.spkcache_len, m.spkcache_sil_frames_per_spk
    per = L // n_spk - sil
    f32 = np.float32
    strong, weak, min_pos = (int(math.floor(f32(per) * f32(r))) for r in (m.strong_boost_rate, m.weak_boost_rate, m.min_pos_scores_rate))
    scores = disable_low_scores(preds, get_log_pred_scores(preds, m.pred_score_threshold), min_pos)
    if m.scores_boost_latest > 0 and scores.shape[1] > L:
        scores = scores.copy()
        scores[:, L:, :] += f32(m.scores_boost_latest)
    scores = boost_topk_scores(scores, strong, 2.0)
    scores = boost_topk_scores(scores, weak, 1.0)
    if sil > 0:
        scores = np.concatenate([scores, np.full((scores.shape[0], sil, n_spk), np.inf, f32)], axis=1)
    idx, disabled = get_topk_indices(scores, L, sil, m.max_index)
    g_embs = np.take_along_axis(embs, idx[..., None], axis=1)
    g_embs = np.where(disabled[..., None], mean_sil_emb[:, None, :], g_embs).astype(f32)
    g_preds = np.where(disabled[..., None], f32(0), np.take_along_axis(preds, idx[..., None], axis=1)).astype(f32)
    return g_embs, g_preds


def compress_spkcache_simple(embs, preds, target_len: int):
    """compressSpkcacheSimple (:1266-1280): the target_len frames with the largest sum of log-probabilities, in time order."""
    score = np.log(np.clip(preds[0], np.float32(1e-7), np.float32(1.0))).sum(axis=-1, dtype=np.float32)
    top = np.sort(np.argsort(-score, kind="stable")[:target_len])
    return embs[:, top, :], preds[:, top, :]


def maybe_compress_state(state: StreamingState, spkcache_max: int, fifo_max: int, m: ModulesConfig) -> StreamingState:
    """maybeCompressState (:1018-1084)."""
    if state.fifo_len <= fifo_max:
        return state
    pop = state.fifo_len - fifo_max
    if m.use_aosc:
        pop = min(pop, m.spkcache_update_period)
    p_embs, p_preds = state.fifo[:, :pop], state.fifo_preds[:, :pop]
    mean_sil, n_sil = state.mean_sil_emb, state.n_sil_frames
    if m.use_aosc:
        mean_sil, n_sil = get_silence_profile(mean_sil, n_sil, p_embs, p_preds, m.sil_threshold)
    cache = np.concatenate([state.spkcache, p_embs], axis=1)
    cache_preds = np.concatenate([state.spkcache_preds, p_preds], axis=1)
    if cache.shape[1] > spkcache_max:
        if m.use_aosc:
            cache, cache_preds = compress_spkcache_aosc(cache, cache_preds, mean_sil, m)
        else:
            cache, cache_preds = compress_spkcache_simple(cache, cache_preds, spkcache_max)
    return StreamingState(cache, cache_preds, state.fifo[:, pop:], state.fifo_preds[:, pop:], state.frames_processed, mean_sil, n_sil)


class SortformerModel(NativeHandle):
    """generate / feed / generateStream / callAsFunction of the reference class, plus ragged batches; 1..max_batch rows a call."""
    _prefix = "mis_sortformer"

    def __init__(self, config: SortformerConfig, device: int = 0):
        self.config, self.device = config, device
        self._create(config.to_c(), device)

    sanitize = staticmethod(sortformer_sanitize)
    preds_to_segments = staticmethod(preds_to_segments)
    maybe_compress_state = staticmethod(maybe_compress_state)

    @classmethod
    def from_weights(cls, config: SortformerConfig, weights: dict, device: int = 0) -> "SortformerModel":
        """weights: sanitized names (what sortformer_sanitize returns)."""
        m = cls(config, device)
        for name, arr in weights.items():
            m.set_tensor(name, arr)
        m.finalize()
        return m

    @classmethod
    def synthetic(cls, config: SortformerConfig, device: int = 0, seed: int = 777) -> "SortformerModel":
        m = cls(config, device)
        check(_lib.lib().mis_sortformer_init_synthetic(m._h, seed))
        m.finalize()
        return m

    @classmethod
    def from_model_directory(cls, model_dir: str, device: int = 0, **workspace) -> "SortformerModel":
        """fromModelDirectory (:1406-1432): config.json, every *.safetensors; keys the model does not have are rejected."""
        with open(os.path.join(model_dir, "config.json")) as f:
            config = SortformerConfig.from_dict(json.load(f), **workspace)
        weights = sortformer_sanitize(read_safetensors_dir(model_dir, missing_code=(2, f"No safetensors files found in {model_dir}")))
        unknown = sorted(set(weights) - sortformer_expected_keys(config))
        if unknown:
            raise AudioGenerationError(3, f"Sortformer checkpoint: unused keys {unknown[:4]}")
        return cls.from_weights(config, weights, device)

    @classmethod
    def from_pretrained(cls, path: str, device: int = 0, **workspace) -> "SortformerModel":
        """Local directories only: nothing is downloaded."""
        if not os.path.isdir(path):
            raise AudioGenerationError(3, f"Sortformer: {path} is not a local model directory")
        return cls.from_model_directory(path, device, **workspace)

    # -- sizes ---------------------------------------------------------------------------------------
    @property
    def launches(self) -> int:
        return int(_lib.lib().mis_sortformer_launches(self._h))

    @property
    def frame_duration(self) -> np.float32:
        p = self.config.processor_config
        return np.float32(p.hop_length * self.config.fc_encoder_config.subsampling_factor) / np.float32(p.sampling_rate)

    def frames(self, lens, pad_to: int = 16):
        """(F, T) of rows of `lens` samples: feature frames (pad_to applied) and diarization frames."""
        n = np.ascontiguousarray(lens, dtype=np.int64)
        F, T = np.zeros(len(n), np.int32), np.zeros(len(n), np.int32)
        check(_lib.lib().mis_sortformer_frames(self._h, n.ctypes.data, len(n), pad_to, F.ctypes.data, T.ctypes.data))
        return F, T

    @staticmethod
    def diar_frames(F: int) -> int:
        for _ in range(3):
            F = (F - 1) // 2 + 1
        return F

    @staticmethod
    def _pack(audios, junk=None):
        rows = [np.asarray(w, np.float32) for w in audios]
        if not rows or any(r.ndim != 1 for r in rows):
            raise AudioGenerationError(3, "Sortformer: a non-empty list of one-dimensional waveforms is expected")
        return pack_rows(rows, junk)

    # -- device calls --------------------------------------------------------------------------------
    def features(self, audios, peak_normalize=True, normalize=True, pad_to: int = 16, junk=None) -> np.ndarray:
        """Log-mel features [B, Fmax, mels] of a ragged list of waveforms, zeros behind a row's own frames."""
        pcm, lens = self._pack(audios, junk)
        F, _ = self.frames(lens, pad_to)
        out = np.zeros((len(lens), int(F.max()), self.config.fc_encoder_config.num_mel_bins), np.float32)
        check(_lib.lib().mis_sortformer_features(self._h, pcm.ctypes.data, lens.ctypes.data, len(lens), pcm.shape[1], int(peak_normalize),
                                                 int(bool(normalize)), pad_to, out.ctypes.data))
        return out

    def forward(self, audios, peak_normalize=True, normalize=True, pad_to: int = 16, junk=None) -> np.ndarray:
        """Probabilities [B, Tmax, speakers] of a ragged list of waveforms, zeros behind a row's own T; one device call."""
        pcm, lens = self._pack(audios, junk)
        _, T = self.frames(lens, pad_to)
        out = np.zeros((len(lens), int(T.max()), self.config.modules_config.num_speakers), np.float32)
        check(_lib.lib().mis_sortformer_forward(self._h, pcm.ctypes.data, lens.ctypes.data, len(lens), pcm.shape[1], int(peak_normalize),
                                                int(bool(normalize)), pad_to, out.ctypes.data))
        return out

    def _features_arg(self, features):
        f = np.ascontiguousarray(features, dtype=np.float32)
        if f.ndim == 2:
            f = f[None]
        if f.ndim != 3 or f.shape[2] != self.config.fc_encoder_config.num_mel_bins:
            raise AudioGenerationError(3, f"Sortformer: features of shape {f.shape}, expected [batch, frames, num_mel_bins]")
        return f

    def __call__(self, features, frames=None) -> np.ndarray:
        """callAsFunction (:548-559) on features [B, F, mels] (time-major, the transpose of the reference's [B, mels, F]) ->
        probabilities [B, T, speakers]; frames[B]: valid frames a row."""
        f = self._features_arg(features)
        fr = None if frames is None else np.ascontiguousarray(frames, dtype=np.int32)
        out = np.zeros((f.shape[0], self.diar_frames(f.shape[1]), self.config.modules_config.num_speakers), np.float32)
        check(_lib.lib().mis_sortformer_forward_features(self._h, f.ctypes.data, None if fr is None else fr.ctypes.data, f.shape[0], f.shape[1],
                                                         out.ctypes.data))
        return out

    def pre_encode(self, features, frames=None) -> np.ndarray:
        """fcEncoder.preEncode: features [B, F, mels] -> stem embeddings [B, T, hidden]."""
        f = self._features_arg(features)
        fr = None if frames is None else np.ascontiguousarray(frames, dtype=np.int32)
        out = np.zeros((f.shape[0], self.diar_frames(f.shape[1]), self.config.fc_encoder_config.hidden_size), np.float32)
        check(_lib.lib().mis_sortformer_pre_encode(self._h, f.ctypes.data, None if fr is None else fr.ctypes.data, f.shape[0], f.shape[1],
                                                   out.ctypes.data))
        return out

    def encode_embeddings(self, embs, counts=None) -> np.ndarray:
        """fcEncoder.encode onward: embeddings [B, T, hidden] -> probabilities [B, T, speakers]."""
        e = np.ascontiguousarray(embs, dtype=np.float32)
        if e.ndim == 2:
            e = e[None]
        if e.ndim != 3 or e.shape[2] != self.config.fc_encoder_config.hidden_size:
            raise AudioGenerationError(3, f"Sortformer: embeddings of shape {e.shape}, expected [batch, frames, hidden_size]")
        cn = None if counts is None else np.ascontiguousarray(counts, dtype=np.int32)
        out = np.zeros((e.shape[0], e.shape[1], self.config.modules_config.num_speakers), np.float32)
        check(_lib.lib().mis_sortformer_encode_embeddings(self._h, e.ctypes.data, None if cn is None else cn.ctypes.data, e.shape[0], e.shape[1],
                                                          out.ctypes.data))
        return out

    def tap(self, stage: int) -> np.ndarray:
        """Tensors of the last call: 0 the stem, 1..L the Conformer blocks, L + 1 the projection, L + 2 .. L + 1 + Lt the BART layers,
        L + 2 + Lt the probabilities; zero rows behind a row's own T."""
        dims = (C.c_int64 * 3)()
        check(_lib.lib().mis_sortformer_tap(self._h, stage, None, 0, dims))
        out = np.zeros(tuple(int(d) for d in dims), np.float32)
        check(_lib.lib().mis_sortformer_tap(self._h, stage, out.ctypes.data, out.size, dims))
        return out

    def enable_timing(self):
        check(_lib.lib().mis_debug_sortformer_timing(self._h, None))

    def timing(self):
        """Device milliseconds of the last forward: (front end, stem, Conformer, BART + head); enable_timing() first."""
        ms = (C.c_float * 4)()
        check(_lib.lib().mis_debug_sortformer_timing(self._h, ms))
        return tuple(float(v) for v in ms)

    # -- offline -------------------------------------------------------------------------------------
    @staticmethod
    def _mono(audio) -> np.ndarray:
        a = np.asarray(audio, np.float32)
        return a.mean(axis=-1, dtype=np.float32) if a.ndim > 1 else a

    def _shift(self, segments, offset):
        off = np.float32(offset)
        return [DiarizationSegment(float(np.float32(s.start) + off), float(np.float32(s.end) + off), s.speaker) for s in segments]

    def generate_batch(self, audios, sample_rate: int = 16000, threshold: float = 0.5, min_duration: float = 0.0, merge_gap: float = 0.0) -> list:
        """generate (:563-651) for a ragged list of waveforms in ONE device call: each row trimmed, peak-normalised on the device,
        features padded to 16 frames, segments shifted by the row's trim offset."""
        start = time.perf_counter()
        sr = self.config.processor_config.sampling_rate
        trimmed = [trim_silence(self._mono(a), sr) for a in audios]
        probs = self.forward([w for w, _ in trimmed])
        _, T = self.frames([len(w) for w, _ in trimmed])
        elapsed = time.perf_counter() - start
        outs = []
        for b, (_, off) in enumerate(trimmed):
            p = probs[b, : T[b]]
            segs = preds_to_segments(p, self.frame_duration, threshold, min_duration, merge_gap)
            if off > 0:
                segs = self._shift(segs, np.float32(off) / np.float32(sr))
            outs.append(DiarizationOutput(segs, p, len({s.speaker for s in segs}), elapsed))
        return outs

    def generate(self, audio, sample_rate: int = 16000, threshold: float = 0.5, min_duration: float = 0.0, merge_gap: float = 0.0) -> DiarizationOutput:
        return self.generate_batch([audio], sample_rate, threshold, min_duration, merge_gap)[0]

    # -- streaming -----------------------------------------------------------------------------------
    def init_streaming_state(self) -> StreamingState:
        d, s = self.config.fc_encoder_config.hidden_size, self.config.modules_config.num_speakers
        z = lambda *shape: np.zeros(shape, np.float32)
        return StreamingState(z(1, 0, d), z(1, 0, s), z(1, 0, d), z(1, 0, s), 0, z(1, d), z(1))

    def streaming_step(self, chunk_features, state: StreamingState, right_context_embs=None):
        """streamingStep (:672-743): chunk features [F, mels] -> (chunk probabilities [T, speakers], new state)."""
        m = self.config.modules_config
        lc = m.chunk_left_context if m.use_aosc else 0
        rc = m.chunk_right_context if m.use_aosc else 0
        chunk = self.pre_encode(chunk_features)
        n_chunk = chunk.shape[1]
        parts = []
        if state.spkcache_len > 0:
            parts.append(state.spkcache)
        if state.fifo_len > 0:
            parts.append(state.fifo)
        left = 0
        if lc > 0 and state.fifo_len > 0:
            left = min(lc, state.fifo_len)
            parts.append(state.fifo[:, state.fifo_len - left:])
        parts.append(chunk)
        if right_context_embs is not None and rc > 0 and right_context_embs.shape[1] > 0:
            parts.append(np.asarray(right_context_embs, np.float32))
        preds = self.encode_embeddings(np.concatenate(parts, axis=1))
        a, b = state.spkcache_len, state.spkcache_len + state.fifo_len
        c0 = b + left
        chunk_preds = preds[:, c0: c0 + n_chunk]
        cache_preds = preds[:, :a] if a > 0 else state.spkcache_preds
        fifo_preds = preds[:, a:b] if state.fifo_len > 0 else state.fifo_preds
        new = StreamingState(state.spkcache, cache_preds, np.concatenate([state.fifo, chunk], axis=1),
                             np.concatenate([fifo_preds, chunk_preds], axis=1), state.frames_processed + n_chunk, state.mean_sil_emb,
                             state.n_sil_frames)
        return chunk_preds[0], new

    def _stream_features(self, waveform, pad_to):
        aosc = self.config.modules_config.use_aosc
        return self.features([waveform], peak_normalize=not aosc, normalize=not aosc, pad_to=pad_to)[0]

    def _chunk_output(self, preds, offset, threshold, min_duration, merge_gap, state=None):
        segs = self._shift(preds_to_segments(preds, self.frame_duration, threshold, min_duration, merge_gap), offset)
        return DiarizationOutput(segs, preds, len({s.speaker for s in segs}), state=state)

    def feed(self, chunk, state: StreamingState, sample_rate: int = 16000, threshold: float = 0.5, min_duration: float = 0.0,
             merge_gap: float = 0.0, spkcache_max: int = 188, fifo_max: int = 188):
        """feed (:746-831): one audio chunk -> (DiarizationOutput, new state)."""
        offset = np.float32(state.frames_processed) * self.frame_duration
        preds, new = self.streaming_step(self._stream_features(self._mono(chunk), 0), state)
        out = self._chunk_output(preds, offset, threshold, min_duration, merge_gap)
        return out, maybe_compress_state(new, spkcache_max, fifo_max, self.config.modules_config)

    def generate_stream(self, audio, sample_rate: int = 16000, chunk_duration: float = 5.0, threshold: float = 0.5, min_duration: float = 0.0,
                        merge_gap: float = 0.0, spkcache_max: int = 188, fifo_max: int = 188):
        """generateStream (:834-988): yields one DiarizationOutput a chunk (its `state` is the state behind that chunk).  v2.1
        (use_aosc): un-normalised features, and the right context of every chunk is cut from ONE pre-encode of the whole file."""
        p, m = self.config.processor_config, self.config.modules_config
        sub = self.config.fc_encoder_config.subsampling_factor
        w = self._mono(audio)
        trim_sec = np.float32(0)
        if not m.use_aosc:
            w, off = trim_silence(w, p.sampling_rate)
            trim_sec = np.float32(off) / np.float32(p.sampling_rate)
        feats = self._stream_features(w, 0 if m.use_aosc else 16)
        total = feats.shape[0]
        chunk_mel = max(int(round(float(np.float32(chunk_duration) * np.float32(p.sampling_rate) / np.float32(p.hop_length) / np.float32(sub)))) * sub, sub)
        rc = m.chunk_right_context
        all_pre = self.pre_encode(feats) if (m.use_aosc and rc > 0) else None
        state, offset_mel, emb_off = self.init_streaming_state(), 0, 0
        while offset_mel < total:
            end = min(offset_mel + chunk_mel, total)
            right = None
            if all_pre is not None:
                n_emb = self.diar_frames(end - offset_mel)
                a, b = emb_off + n_emb, min(emb_off + n_emb + rc, all_pre.shape[1])
                if b > a:
                    right = all_pre[:, a:b]
                emb_off += n_emb
            preds, state = self.streaming_step(feats[offset_mel:end], state, right)
            t0 = np.float32(offset_mel * p.hop_length) / np.float32(p.sampling_rate) + trim_sec
            out = self._chunk_output(preds, t0, threshold, min_duration, merge_gap, state)
            state = maybe_compress_state(state, spkcache_max, fifo_max, m)
            yield out
            offset_mel = end
