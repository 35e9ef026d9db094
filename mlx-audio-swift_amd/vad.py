"""FSMN voice activity detection, host mirror of `FSMNVAD` (Sources/MLXAudioVAD/Models/FSMNVAD/FSMNVAD.swift).  Configuration,
checkpoint and CMVN loading, the ragged-batch packing and the serial post-processing (:239-701) stay on the host; the Kaldi-style fbank,
LFR stacking + CMVN and the FSMN encoder run in libmi_speech.so (csrc/fsmn_vad.hip), for rows of any length."""
from __future__ import annotations

import ctypes as C
import json
import os
from dataclasses import dataclass, field, fields

import numpy as np

from . import _lib
from ._handle import NativeHandle, pack_rows
from .generation import AudioGenerationError, check

_F = np.float32


@dataclass
class FSMNVADEncoderConfig:
    """FSMNVADEncoderConfig (:7-59): every field, default and JSON key."""
    input_dim: int = 400
    input_affine_dim: int = 140
    fsmn_layers: int = 4
    linear_dim: int = 250
    proj_dim: int = 128
    lorder: int = 20
    rorder: int = 0
    lstride: int = 1
    rstride: int = 0
    output_affine_dim: int = 140
    output_dim: int = 248

    @classmethod
    def from_dict(cls, d: dict) -> "FSMNVADEncoderConfig":
        """The synthesized Codable init: every key is required."""
        names = [f.name for f in fields(cls)]
        missing = [k for k in names if k not in d]
        if missing:
            raise AudioGenerationError(3, f"FSMN VAD: encoder config misses {missing}")
        return cls(**{k: int(d[k]) for k in names})


_TOP_KEYS = ("model_type", "architecture", "sample_rate", "n_mels", "frame_length", "frame_shift", "lfr_m", "lfr_n", "max_end_silence_time",
             "max_start_silence_time", "window_size_ms", "sil_to_speech_time_thres", "speech_to_sil_time_thres", "speech_noise_thres",
             "sil_pdf_ids", "frame_in_ms")


@dataclass
class FSMNVADConfig:
    """FSMNVADConfig (:61-158): every field, default and JSON key.  max_batch / chunk_frames size the engine's workspace (rows a call,
    LFR rows a time chunk) and are not part of a checkpoint."""
    model_type: str = "fsmn"
    architecture: str = "fsmn_vad"
    encoder: FSMNVADEncoderConfig = field(default_factory=FSMNVADEncoderConfig)
    sample_rate: int = 16000
    n_mels: int = 80
    frame_length: int = 25
    frame_shift: int = 10
    lfr_m: int = 5
    lfr_n: int = 1
    max_end_silence_time: int = 800
    max_start_silence_time: int = 3000
    window_size_ms: int = 200
    sil_to_speech_time_thres: int = 150
    speech_to_sil_time_thres: int = 150
    speech_noise_thres: float = 0.6
    sil_pdf_ids: list = field(default_factory=lambda: [0])
    frame_in_ms: int = 10
    max_batch: int = 8
    chunk_frames: int = 3000

    @classmethod
    def from_dict(cls, d: dict, **workspace) -> "FSMNVADConfig":
        """init(from:) (:138-157): missing or null keys take the defaults, unknown keys are ignored."""
        kw = {k: d[k] for k in _TOP_KEYS if d.get(k) is not None}
        if d.get("encoder") is not None:
            kw["encoder"] = FSMNVADEncoderConfig.from_dict(d["encoder"])
        return cls(**kw, **workspace)

    def to_c(self) -> "_lib.FsmnVadConfigC":
        e = self.encoder
        ids = [int(i) for i in self.sil_pdf_ids if 0 <= int(i) < e.output_dim]        # (an id beyond the scores is skipped, :536-540)
        if len(ids) > 16:
            raise AudioGenerationError(3, "FSMN VAD: at most 16 sil_pdf_ids are served")
        if self.frame_in_ms != self.frame_shift:
            raise AudioGenerationError(3, "FSMN VAD: frame_in_ms differs from frame_shift; the decibel and score frames would not line up")
        return _lib.FsmnVadConfigC(e.input_dim, e.input_affine_dim, e.fsmn_layers, e.linear_dim, e.proj_dim, e.lorder, e.rorder, e.lstride,
                                   e.rstride, e.output_affine_dim, e.output_dim, self.sample_rate, self.n_mels, self.frame_length,
                                   self.frame_shift, self.lfr_m, self.lfr_n, len(ids), (C.c_int32 * 16)(*ids), self.max_batch,
                                   self.chunk_frames)


def fsmn_vad_sanitize(weights: dict) -> dict:
    """sanitizeEncoderWeights (:812-819): the `encoder.` prefix is stripped, nothing else changes."""
    return {(k[len("encoder."):] if k.startswith("encoder.") else k): v for k, v in weights.items()}


def fsmn_vad_expected_shapes(config: FSMNVADConfig) -> dict:
    """name -> shape of every parameter of FSMNVADEncoder(config): what update(parameters:verify: .all) accepts (:785).  There is no
    right-context tensor: a checkpoint that carries one has unexpected keys."""
    e = config.encoder
    s = {"in_linear1.weight": (e.input_affine_dim, e.input_dim), "in_linear1.bias": (e.input_affine_dim,),
         "in_linear2.weight": (e.linear_dim, e.input_affine_dim), "in_linear2.bias": (e.linear_dim,)}
    for i in range(e.fsmn_layers):
        s[f"fsmn.{i}.linear.weight"] = (e.proj_dim, e.linear_dim)
        s[f"fsmn.{i}.fsmn_block.conv_left.weight"] = (e.proj_dim, e.lorder, 1)
        s[f"fsmn.{i}.affine.weight"], s[f"fsmn.{i}.affine.bias"] = (e.linear_dim, e.proj_dim), (e.linear_dim,)
    s["out_linear1.weight"], s["out_linear1.bias"] = (e.output_affine_dim, e.linear_dim), (e.output_affine_dim,)
    s["out_linear2.weight"], s["out_linear2.bias"] = (e.output_dim, e.output_affine_dim), (e.output_dim,)
    return s


def fsmn_vad_check_weights(config: FSMNVADConfig, weights: dict):
    want = fsmn_vad_expected_shapes(config)
    unknown, missing = sorted(set(weights) - set(want)), sorted(set(want) - set(weights))
    if unknown or missing:
        raise AudioGenerationError(3, f"FSMN VAD checkpoint: unexpected keys {unknown[:4]}, missing keys {missing[:4]}")
    bad = [k for k in want if tuple(weights[k].shape) != want[k]]
    if bad:
        raise AudioGenerationError(3, f"FSMN VAD checkpoint: {bad[0]} has shape {tuple(weights[bad[0]].shape)}, expected {want[bad[0]]}")


def parse_kaldi_cmvn(text) -> tuple:
    """parseKaldiCMVN (:900-921): the numbers of the first [ ... ] behind <AddShift> and behind <Rescale> -> (shift, scale) float32;
    tokens that are no numbers are dropped."""
    if isinstance(text, bytes):
        text = text.decode("utf-8", errors="replace")

    def block(marker):
        at = text.find(marker)
        if at < 0:
            return None
        a = text.find("[", at + len(marker))
        if a < 0:
            return None
        b = text.find("]", a)
        if b < 0:
            return None
        vals = []
        for tok in text[a + 1: b].replace("\n", " ").replace("\t", " ").split(" "):
            if tok:
                try:
                    vals.append(float(tok))
                except ValueError:
                    pass
        return np.asarray(vals, _F)

    shift, scale = block("<AddShift>"), block("<Rescale>")
    if shift is None or scale is None:
        raise AudioGenerationError(3, "Could not parse Kaldi CMVN data")
    return shift, scale


def fsmn_vad_read_cmvn(model_dir: str):
    """loadCMVN (:796-810): cmvn.json wins over am.mvn; None when the directory has neither."""
    path = os.path.join(model_dir, "cmvn.json")
    if os.path.isfile(path):
        with open(path) as f:
            d = json.load(f)
        return np.asarray(d["shift"], _F), np.asarray(d["scale"], _F)
    path = os.path.join(model_dir, "am.mvn")
    if os.path.isfile(path):
        with open(path, "rb") as f:
            return parse_kaldi_cmvn(f.read())
    return None


def fsmn_vad_read_directory(model_dir: str, **workspace):
    """config.json, model.safetensors and the CMVN of a model directory (fromModelDirectory, :780-789) -> (FSMNVADConfig, sanitized
    weights, cmvn or None).  No device is touched."""
    path = os.path.join(model_dir, "config.json")
    if not os.path.isfile(path):
        raise AudioGenerationError(3, "FSMN VAD: config.json not found in model directory")
    with open(path) as f:
        cfg = FSMNVADConfig.from_dict(json.load(f), **workspace)
    path = os.path.join(model_dir, "model.safetensors")
    if not os.path.isfile(path):
        raise AudioGenerationError(3, "FSMN VAD: model.safetensors not found in model directory")
    from safetensors import safe_open
    weights = {}
    with safe_open(path, framework="pt") as sf:
        for k in sf.keys():
            weights[k] = sf.get_tensor(k)
    weights = fsmn_vad_sanitize(weights)
    fsmn_vad_check_weights(cfg, weights)
    return cfg, weights, fsmn_vad_read_cmvn(model_dir)


# ------------------------------------------------------------------------------------------------------------ post-processing
_NOT_DETECTED, _IN_SPEECH, _END_DETECTED = 0, 1, 2
_SIL_SIL, _SIL_SPEECH, _SPEECH_SIL, _SPEECH_SPEECH = 0, 1, 2, 3


def fsmn_vad_postprocess(silence, decibel, n_samples: int, config: FSMNVADConfig) -> list:
    """FSMNVADPostprocess.forward (:239-701) for one whole recording: silence[r] = the sum of frame r's scores over sil_pdf_ids, decibel[t]
    the frame energies, n_samples the waveform's length -> [[start_ms, end_ms], ...].  The arithmetic on the probabilities and the noise
    average is numpy.float32 where the Swift uses Float.  The reference's copies of the audio buffer are not made: only the lengths of
    dataBuf / dataBufAll ever reach a decision, and those are carried."""
    c = config
    sil = np.asarray(silence, _F)
    dec = np.asarray(decibel, _F)
    frame_ms = c.frame_in_ms
    shift = c.frame_in_ms * c.sample_rate // 1000
    win_frames = c.window_size_ms // frame_ms
    sil_to_speech, speech_to_sil = c.sil_to_speech_time_thres // frame_ms, c.speech_to_sil_time_thres // frame_ms
    max_end_sil = c.max_end_silence_time - c.speech_to_sil_time_thres
    thr = _F(c.speech_noise_thres)
    has_ids = len(c.sil_pdf_ids) > 0
    latency = win_frames + c.window_size_ms // frame_ms
    max_single = 60000 // frame_ms
    lo, hi, one = _F(1e-7), _F(1.0) - _F(1e-7), _F(1.0)
    # window detector
    win = [0] * max(win_frames, 1)
    st = dict(pos=0, sum=0, prev_speech=False)
    # stats
    s = dict(buf_start=0, frame_count=len(sil), speech=0, silence=-1, cont_sil=0, state=_NOT_DETECTED, start=-1, end=-1, n_end=0,
             noise=_F(-100.0), buf_len=int(n_samples), all_len=int(n_samples), drop=0, dec_off=0, sc_off=0)
    out = []                                                          # [start_ms, end_ms, has_start, has_end]

    def pop_till(frame):
        while s["buf_start"] < frame:
            if s["buf_len"] >= shift:
                s["buf_start"] += 1
                start = max(0, (s["buf_start"] - s["drop"]) * shift)
                s["buf_len"] = s["all_len"] - start if start < s["all_len"] else 0
            else:
                break

    def pop_to_output(start_frame, count, first_is_start, last_is_end):
        pop_till(start_frame)
        if not out or first_is_start:
            out.append([start_frame * frame_ms, start_frame * frame_ms, False, False])
        cur = out[-1]
        s["buf_start"] += count
        cur[1] = (start_frame + count) * frame_ms
        if first_is_start:
            cur[2] = True
        if last_is_end:
            cur[3] = True

    def on_silence(frame):
        s["silence"] = frame
        if s["state"] == _NOT_DETECTED:
            pop_till(frame)

    def on_voice(frame):
        s["speech"] = frame
        pop_to_output(frame, 1, False, False)

    def on_voice_start(frame, fake=False):
        if s["start"] == -1:
            s["start"] = frame
        if not fake and s["state"] == _NOT_DETECTED:
            pop_to_output(s["start"], 1, True, False)

    def on_voice_end(frame, fake):
        for f in range(s["speech"] + 1, frame):
            on_voice(f)
        if s["end"] == -1:
            s["end"] = frame
        if not fake:
            pop_to_output(s["end"], 1, False, True)
        s["n_end"] += 1

    def end_if_last(final, frame):
        if final:
            on_voice_end(frame, False)
            s["state"] = _END_DETECTED

    def reset():
        s.update(cont_sil=0, speech=0, silence=-1, start=-1, end=-1, state=_NOT_DETECTED)
        for i in range(len(win)):
            win[i] = 0
        st.update(pos=0, sum=0, prev_speech=False)
        if out and out[-1][3]:
            drop = out[-1][1] // frame_ms
            real = drop - s["drop"]
            s["drop"] = drop
            samples = real * shift
            s["all_len"] = s["all_len"] - samples if samples < s["all_len"] else 0
            s["dec_off"] = s["dec_off"] + real if real < len(dec) - s["dec_off"] else len(dec)
            s["sc_off"] = s["sc_off"] + real if real < len(sil) - s["sc_off"] else len(sil)

    def frame_is_speech(index):
        if index < 0 or index >= len(dec) - s["dec_off"] or index >= len(sil) - s["sc_off"]:
            return False
        cur = dec[s["dec_off"] + index]
        snr = cur - s["noise"]
        if cur < _F(-100.0):
            return False
        if has_ids:
            p = np.maximum(np.minimum(sil[s["sc_off"] + index], hi), lo)
            noise_prob, speech = np.log(p), one - p
        else:
            noise_prob, speech = np.log(lo), _F(0.0)
        with np.errstate(divide="ignore"):
            speech_prob = np.log(speech)
        if np.exp(speech_prob) >= np.exp(noise_prob) + thr:
            return bool(snr >= _F(-100.0) and cur >= _F(-100.0))
        if s["noise"] < _F(-99.9):
            s["noise"] = cur
        else:
            s["noise"] = (cur + s["noise"] * _F(99)) / _F(100)
        return False

    def window_step(speech):
        cur = 1 if speech else 0
        st["sum"] += cur - win[st["pos"]]
        win[st["pos"]] = cur
        st["pos"] = (st["pos"] + 1) % len(win)
        if not st["prev_speech"] and st["sum"] >= sil_to_speech:
            st["prev_speech"] = True
            return _SIL_SPEECH
        if st["prev_speech"] and st["sum"] <= speech_to_sil:
            st["prev_speech"] = False
            return _SPEECH_SIL
        return _SPEECH_SPEECH if st["prev_speech"] else _SIL_SIL

    def in_speech_step(frame, final):
        if frame - s["start"] + 1 > max_single:
            on_voice_end(frame, False)
            s["state"] = _END_DETECTED
        elif not final:
            on_voice(frame)
        else:
            end_if_last(final, frame)

    def detect_one(speech, frame, final):
        change = window_step(speech)
        if change == _SIL_SPEECH:
            s["cont_sil"] = 0
            if s["state"] == _NOT_DETECTED:
                start = max(s["buf_start"], frame - latency)
                on_voice_start(start)
                s["state"] = _IN_SPEECH
                for f in range(start + 1, frame + 1):
                    on_voice(f)
            elif s["state"] == _IN_SPEECH:
                for f in range(s["speech"] + 1, frame):
                    on_voice(f)
                in_speech_step(frame, final)
        elif change in (_SPEECH_SIL, _SPEECH_SPEECH):
            s["cont_sil"] = 0
            if s["state"] == _IN_SPEECH:
                in_speech_step(frame, final)
        else:
            s["cont_sil"] += 1
            if s["state"] == _NOT_DETECTED:
                if final and s["n_end"] == 0:
                    for f in range(s["silence"] + 1, frame):
                        on_silence(f)
                    on_voice_start(0, fake=True)
                    on_voice_end(0, True)
                    s["state"] = _END_DETECTED
                elif frame >= latency:
                    on_silence(frame - latency)
            elif s["state"] == _IN_SPEECH:
                if s["cont_sil"] * frame_ms >= max_end_sil:
                    look = max(0, max_end_sil // frame_ms - c.window_size_ms // frame_ms // 2 - 1)
                    on_voice_end(frame - look, False)
                    s["state"] = _END_DETECTED
                elif frame - s["start"] + 1 > max_single:
                    on_voice_end(frame, False)
                    s["state"] = _END_DETECTED
                elif s["cont_sil"] <= c.window_size_ms // frame_ms // 2 and not final:
                    on_voice(frame)
                else:
                    end_if_last(final, frame)
        if s["state"] == _END_DETECTED:
            reset()

    block = len(sil)
    for i in range(block - 1, -1, -1):
        frame = s["frame_count"] - 1 - i
        detect_one(frame_is_speech(frame - s["drop"]), frame, i == 0)
    return [[a, b] for a, b, _, _ in out]


def chunks_from_segments(segments_ms, n_samples: int, sample_rate: int, merge_gap_s: float = 1.0, max_chunk_s: float = 30.0) -> list:
    """Speech segments in milliseconds -> [(start_sample, end_sample, offset_s)] for the batch STT calls: neighbours closer than
    merge_gap_s are merged while the chunk stays within max_chunk_s, longer runs are cut at max_chunk_s (mergeRuns / splitLong,
    SpeechSegmenter.swift:115-155).  Ends are clamped to n_samples, the maximum chunk to >= 1 sample; no segments -> the whole buffer at
    offset 0.  The reference's segmentSpeech is typed to Silero; this is the model-agnostic half of it, fed here by FSMNVAD.detect."""
    runs = []
    for a, b in segments_ms:
        s0, e0 = int(a) * sample_rate // 1000, min(int(b) * sample_rate // 1000, int(n_samples))
        if s0 < e0:
            runs.append((s0, e0))
    if not runs:
        return [(0, int(n_samples), 0.0)]
    max_chunk = max(1, int(_F(max_chunk_s) * _F(sample_rate)))
    max_gap = int(_F(merge_gap_s) * _F(sample_rate))

    def split(a, b):
        if b - a <= max_chunk:
            return [(a, b)]
        return [(cur, min(cur + max_chunk, b)) for cur in range(a, b, max_chunk)]

    merged = split(*runs[0])
    for a, b in runs[1:]:
        p0, p1 = merged[-1]
        if a - p1 <= max_gap and b - p0 <= max_chunk:
            merged[-1] = (p0, b)
        else:
            merged.extend(split(a, b))
    return [(a, b, a / float(sample_rate)) for a, b in merged]


# ------------------------------------------------------------------------------------------------------------ the model
class FSMNVAD(NativeHandle):
    """extractFeatures / callAsFunction / detect of the reference class, plus ragged batches; one handle, 1..max_batch rows a call, rows
    of any length (the engine walks them in chunks of chunk_frames)."""
    _prefix = "mis_fsmn_vad"

    def __init__(self, config: FSMNVADConfig, device: int = 0):
        self.config = config
        self.device = device
        self._create(config.to_c(), device)

    @classmethod
    def from_weights(cls, config: FSMNVADConfig, weights: dict, cmvn=None, device: int = 0) -> "FSMNVAD":
        """weights: sanitized names (what fsmn_vad_sanitize returns), all of them and no others; cmvn: (shift, scale) or None."""
        fsmn_vad_check_weights(config, weights)
        m = cls(config, device)
        for name, arr in weights.items():
            m.set_tensor(name, arr)
        if cmvn is not None:
            m.set_tensor("cmvn.shift", np.ascontiguousarray(cmvn[0], _F))
            m.set_tensor("cmvn.scale", np.ascontiguousarray(cmvn[1], _F))
        m.finalize()
        return m

    @classmethod
    def synthetic(cls, config: FSMNVADConfig, device: int = 0, seed: int = 777) -> "FSMNVAD":
        m = cls(config, device)
        check(_lib.lib().mis_fsmn_vad_init_synthetic(m._h, seed))
        m.finalize()
        return m

    @classmethod
    def from_model_directory(cls, model_dir: str, device: int = 0, **workspace) -> "FSMNVAD":
        cfg, weights, cmvn = fsmn_vad_read_directory(model_dir, **workspace)
        return cls.from_weights(cfg, weights, cmvn, device)

    @classmethod
    def from_pretrained(cls, path: str, device: int = 0, **workspace) -> "FSMNVAD":
        """fromPretrained (:762-778) for a local path; this package downloads nothing."""
        p = os.path.expanduser(path)
        if not os.path.isdir(p):
            raise AudioGenerationError(3, f"FSMN VAD: {path} is no local model directory (nothing is downloaded)")
        return cls.from_model_directory(p, device, **workspace)

    sanitize = staticmethod(fsmn_vad_sanitize)

    @property
    def launches(self) -> int:
        return int(_lib.lib().mis_fsmn_vad_launches(self._h))

    # -- inputs --------------------------------------------------------------------------------------
    def _row(self, audio, sample_rate) -> np.ndarray:
        a = np.asarray(audio, _F)
        if a.ndim != 1:
            raise AudioGenerationError(3, f"FSMN VAD: audio must be one-dimensional, got shape {a.shape}")
        rate = self.config.sample_rate
        if sample_rate is not None and int(sample_rate) != rate:
            raise AudioGenerationError(3, f"FSMN VAD: audio at {sample_rate} Hz, the model takes {rate} Hz; this package has no "
                                          "resampler - resample before the call")
        return a

    def _pack(self, waveforms, sample_rate, junk):
        rows = [self._row(w, sample_rate) for w in waveforms]
        if not rows:
            raise AudioGenerationError(3, "FSMN VAD: no rows")
        pcm, lens = pack_rows(rows, junk)
        return pcm, lens, *pcm.shape

    def frames(self, lens):
        """Sample counts -> (fbank frames T, LFR rows R), int32 arrays."""
        lens = np.ascontiguousarray(lens, np.int64)
        T, R = np.zeros(len(lens), np.int32), np.zeros(len(lens), np.int32)
        check(_lib.lib().mis_fsmn_vad_frames(self._h, lens.ctypes.data, len(lens), T.ctypes.data, R.ctypes.data))
        return T, R

    # -- calls ---------------------------------------------------------------------------------------
    def features_raw(self, waveforms, sample_rate=None, junk: float | None = None):
        """Ragged list of waveforms -> (features [B, Rmax, input_dim], R [B])."""
        pcm, lens, B, stride = self._pack(waveforms, sample_rate, junk)
        T, R = self.frames(lens)
        out = np.zeros((B, max(1, int(R.max())), self.config.encoder.input_dim), _F)
        check(_lib.lib().mis_fsmn_vad_features(self._h, pcm.ctypes.data, lens.ctypes.data, B, stride, out.ctypes.data, out.shape[1]))
        return out[:, : int(R.max())], R

    def extract_features(self, waveform, sample_rate: int = 16000) -> np.ndarray:
        """extractFeatures (:720-740): one waveform -> [T + 2, 400] at the published configuration ([0, 400] below one window)."""
        out, R = self.features_raw([waveform], sample_rate)
        return out[0, : int(R[0])]

    def scores_raw(self, waveforms, sample_rate=None, junk: float | None = None):
        """Ragged list of waveforms -> (scores [B, Rmax, output_dim], R [B])."""
        pcm, lens, B, stride = self._pack(waveforms, sample_rate, junk)
        T, R = self.frames(lens)
        out = np.zeros((B, max(1, int(R.max())), self.config.encoder.output_dim), _F)
        check(_lib.lib().mis_fsmn_vad_forward(self._h, pcm.ctypes.data, lens.ctypes.data, B, stride, out.ctypes.data, out.shape[1]))
        return out[:, : int(R.max())], R

    def forward_features(self, features, counts=None) -> np.ndarray:
        """features [R, input_dim] or [B, R, input_dim], counts[B] valid rows each (None: R) -> scores [B, R, output_dim]."""
        f = np.ascontiguousarray(features, dtype=_F)
        if f.ndim == 2:
            f = f[None]
        if f.ndim != 3 or f.shape[2] != self.config.encoder.input_dim:
            raise AudioGenerationError(3, f"FSMN VAD: features of shape {f.shape}, expected [batch, rows, {self.config.encoder.input_dim}]")
        B, R = f.shape[0], f.shape[1]
        cn = None if counts is None else np.ascontiguousarray(counts, dtype=np.int32)
        if cn is not None and cn.shape != (B,):
            raise AudioGenerationError(3, "FSMN VAD: one row count per batch row is expected")
        out = np.zeros((B, R, self.config.encoder.output_dim), _F)
        if R == 0:
            return out
        check(_lib.lib().mis_fsmn_vad_forward_features(self._h, f.ctypes.data, None if cn is None else cn.ctypes.data, B, R, out.ctypes.data))
        return out

    def __call__(self, features, counts=None) -> np.ndarray:
        """callAsFunction (:716-718): features [batch, time, input_dim] -> scores [batch, time, output_dim]."""
        return self.forward_features(features, counts)

    def detect_raw(self, waveforms, sample_rate=None, junk: float | None = None):
        """Ragged list of waveforms -> (silence [B, Rmax], decibel [B, Tmax], R [B], T [B]): the two floats a frame the post-processing
        reads."""
        pcm, lens, B, stride = self._pack(waveforms, sample_rate, junk)
        T, R = self.frames(lens)
        sil, dec = np.zeros((B, max(1, int(R.max()))), _F), np.zeros((B, max(1, int(T.max()))), _F)
        check(_lib.lib().mis_fsmn_vad_detect_raw(self._h, pcm.ctypes.data, lens.ctypes.data, B, stride, sil.ctypes.data, sil.shape[1],
                                                 dec.ctypes.data, dec.shape[1]))
        return sil[:, : int(R.max())], dec[:, : int(T.max())], R, T

    def detect_batch(self, waveforms, sample_rate=None) -> list:
        """detect for a ragged batch: one list of [start_ms, end_ms] per row; a row below one window gives []."""
        rows = [self._row(w, sample_rate) for w in waveforms]
        sil, dec, R, T = self.detect_raw(rows)
        return [fsmn_vad_postprocess(sil[b, : R[b]], dec[b, : T[b]], len(rows[b]), self.config) if R[b] > 0 else []
                for b in range(len(rows))]

    def detect(self, waveform, sample_rate: int = 16000) -> list:
        """detect (:742-760): one waveform -> [[start_ms, end_ms], ...]."""
        return self.detect_batch([waveform], sample_rate)[0]

    def tap(self, stage: int) -> np.ndarray:
        """Tensors of the last chunk of the last call: 0 fbank [B, F, n_mels], 1 decibel [B, F], 2 features [B, R, input_dim], 3 in_linear1,
        4 in_linear2, 5 + 2 i layer i's projection, 6 + 2 i its output, 5 + 2 L out_linear1, 6 + 2 L scores, 7 + 2 L silence sum [B, R]."""
        dims = (C.c_int64 * 3)()
        check(_lib.lib().mis_fsmn_vad_tap(self._h, stage, None, 0, dims))
        out = np.zeros(tuple(int(d) for d in dims), _F)
        check(_lib.lib().mis_fsmn_vad_tap(self._h, stage, out.ctypes.data, out.size, dims))
        return out[:, :, 0] if out.shape[2] == 1 and stage in (1, 7 + 2 * self.config.encoder.fsmn_layers) else out

    def timing(self):
        """Device milliseconds of the last call: (front end, encoder)."""
        ms = (C.c_float * 2)()
        check(_lib.lib().mis_debug_fsmn_vad_timing(self._h, ms))
        return float(ms[0]), float(ms[1])
