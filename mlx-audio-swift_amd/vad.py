"""Voice activity detection, host mirrors of `FSMNVAD` (Sources/MLXAudioVAD/Models/FSMNVAD/FSMNVAD.swift), `SileroVAD`
(Models/SileroVAD/SileroVAD.swift) and `segmentSpeech` (SpeechSegmenter.swift).  Configuration, checkpoint and CMVN loading, the
ragged-batch packing and the serial post-processing stay on the host; the Kaldi-style fbank, LFR stacking + CMVN and the FSMN encoder
(csrc/fsmn_vad.hip), and Silero's chunk-parallel front end and LSTM recurrence (csrc/silero_vad.hip) run in libmi_speech.so, for rows of
any length."""
from __future__ import annotations

import ctypes as C
import json
import os
from dataclasses import dataclass, field, fields

import numpy as np

from . import _lib
from ._handle import NativeHandle, pack_rows, read_safetensors_dir
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
    return [(a, b, a / float(sample_rate)) for a, b in merge_runs(runs, sample_rate, merge_gap_s, max_chunk_s)]


def merge_runs(runs, sample_rate: int, merge_gap_s: float = 1.0, max_chunk_s: float = 30.0) -> list:
    """mergeRuns / splitLong (SpeechSegmenter.swift:115-155) on a non-empty list of (start_sample, end_sample): what
    chunks_from_segments and segment_speech share.  The two limits are formed in float32 as the Swift forms them."""
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
    return merged


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


# ============================================================================================================ Silero VAD
class SileroVADError(AudioGenerationError):
    """SileroVADError (SileroVAD.swift:29-48): `.kind` holds the Swift case name, the message its errorDescription."""

    def __init__(self, kind: str, message: str):
        self.kind = kind
        super().__init__(3, message)

    @classmethod
    def invalid_repository_id(cls, repo):
        return cls("invalidRepositoryID", f"Invalid repository ID: {repo}")

    @classmethod
    def unsupported_sample_rate(cls, sr):
        return cls("unsupportedSampleRate", f"Silero VAD supports 8000 Hz and 16000 Hz audio (got {sr})")

    @classmethod
    def state_sample_rate_mismatch(cls, expected, got):
        return cls("stateSampleRateMismatch", f"Streaming state is for {expected} Hz, got {got} Hz")

    @classmethod
    def unexpected_chunk_size(cls, expected, got):
        return cls("unexpectedChunkSize", f"Expected {expected} samples per chunk, got {got}")

    @classmethod
    def insufficient_reflect_pad_input(cls, samples, pad):
        return cls("insufficientReflectPadInput", f"Reflect padding of {pad} requires more than {pad} samples (got {samples})")


@dataclass
class SileroVADBranchConfig:
    """SileroVADBranchConfig (SileroVADConfig.swift:3-50): every field, default and JSON key."""
    sample_rate: int = 16000
    filter_length: int = 256
    hop_length: int = 128
    pad: int = 64
    cutoff: int = 129
    context_size: int = 64
    chunk_size: int = 512

    @classmethod
    def default_16k(cls) -> "SileroVADBranchConfig":
        return cls()

    @classmethod
    def default_8k(cls) -> "SileroVADBranchConfig":
        return cls(sample_rate=8000, filter_length=128, hop_length=64, pad=32, cutoff=65, context_size=32, chunk_size=256)

    @classmethod
    def from_dict(cls, d: dict) -> "SileroVADBranchConfig":
        """The synthesized Codable init: every key is required."""
        names = [f.name for f in fields(cls)]
        missing = [k for k in names if k not in d]
        if missing:
            raise AudioGenerationError(3, f"Silero VAD: branch config misses {missing}")
        return cls(**{k: int(d[k]) for k in names})

    @property
    def window(self) -> int:
        return self.context_size + self.chunk_size

    def to_c(self) -> "_lib.SileroVadBranchConfigC":
        return _lib.SileroVadBranchConfigC(self.sample_rate, self.filter_length, self.hop_length, self.pad, self.cutoff, self.context_size,
                                           self.chunk_size)


_SILERO_KEYS = ("model_type", "architecture", "dtype", "threshold", "min_speech_duration_ms", "min_silence_duration_ms", "speech_pad_ms")


@dataclass
class SileroVADConfig:
    """SileroVADConfig (SileroVADConfig.swift:52-109): every field and default; the JSON keys of the branches are branch_16k / branch_8k.
    max_batch / max_chunks size the engine's workspace (rows a call, chunks a pass) and are not part of a checkpoint."""
    model_type: str = "silero_vad"
    architecture: str = "silero_vad"
    dtype: str = "float32"
    threshold: float = 0.5
    min_speech_duration_ms: int = 250
    min_silence_duration_ms: int = 100
    speech_pad_ms: int = 30
    branch16k: SileroVADBranchConfig = field(default_factory=SileroVADBranchConfig.default_16k)
    branch8k: SileroVADBranchConfig = field(default_factory=SileroVADBranchConfig.default_8k)
    max_batch: int = 8
    max_chunks: int = 1024

    @classmethod
    def from_dict(cls, d: dict, **workspace) -> "SileroVADConfig":
        """init(from:) (:97-108): missing or null keys take the defaults, unknown keys are ignored."""
        kw = {k: d[k] for k in _SILERO_KEYS if d.get(k) is not None}
        if d.get("branch_16k") is not None:
            kw["branch16k"] = SileroVADBranchConfig.from_dict(d["branch_16k"])
        if d.get("branch_8k") is not None:
            kw["branch8k"] = SileroVADBranchConfig.from_dict(d["branch_8k"])
        return cls(**kw, **workspace)

    def branch(self, sample_rate: int) -> SileroVADBranchConfig:
        """branch(forSampleRate:) (SileroVAD.swift:145-151)."""
        if int(sample_rate) == 16000:
            return self.branch16k
        if int(sample_rate) == 8000:
            return self.branch8k
        raise SileroVADError.unsupported_sample_rate(sample_rate)

    def to_c(self) -> "_lib.SileroVadConfigC":
        return _lib.SileroVadConfigC(self.branch16k.to_c(), self.branch8k.to_c(), self.max_batch, self.max_chunks)


def silero_vad_sanitize(weights: dict) -> dict:
    """sanitize (SileroVAD.swift:331-344): val_* dropped, vad_16k. -> branch16k., vad_8k. -> branch8k."""
    out = {}
    for k, v in weights.items():
        if k.startswith("val_"):
            continue
        if k.startswith("vad_16k."):
            k = "branch16k." + k[len("vad_16k."):]
        elif k.startswith("vad_8k."):
            k = "branch8k." + k[len("vad_8k."):]
        out[k] = v
    return out


def silero_vad_expected_shapes(config: SileroVADConfig) -> dict:
    """name -> shape of every parameter of SileroVAD(config): what update(parameters:verify: .all) accepts (:374).  MLX conv weights are
    [out, kernel, in]."""
    s = {}
    for prefix, b in (("branch16k.", config.branch16k), ("branch8k.", config.branch8k)):
        s[prefix + "stft_conv.weight"] = (2 * b.cutoff, b.filter_length, 1)
        for i, (cin, cout) in enumerate(((b.cutoff, 128), (128, 64), (64, 64), (64, 128)), 1):
            s[f"{prefix}conv{i}.weight"], s[f"{prefix}conv{i}.bias"] = (cout, 3, cin), (cout,)
        s[prefix + "lstm.Wx"], s[prefix + "lstm.Wh"], s[prefix + "lstm.bias"] = (512, 128), (512, 128), (512,)
        s[prefix + "final_conv.weight"], s[prefix + "final_conv.bias"] = (1, 1, 128), (1,)
    return s


def silero_vad_check_weights(config: SileroVADConfig, weights: dict):
    want = silero_vad_expected_shapes(config)
    unknown, missing = sorted(set(weights) - set(want)), sorted(set(want) - set(weights))
    if unknown or missing:
        raise AudioGenerationError(3, f"Silero VAD checkpoint: unexpected keys {unknown[:4]}, missing keys {missing[:4]}")
    bad = [k for k in want if tuple(weights[k].shape) != want[k]]
    if bad:
        raise AudioGenerationError(3, f"Silero VAD checkpoint: {bad[0]} has shape {tuple(weights[bad[0]].shape)}, expected {want[bad[0]]}")


def silero_vad_read_directory(model_dir: str, **workspace):
    """config.json and every *.safetensors of a model directory (fromModelDirectory, :357-377) -> (SileroVADConfig, sanitized weights),
    all keys verified.  No device is touched."""
    path = os.path.join(model_dir, "config.json")
    if not os.path.isfile(path):
        raise AudioGenerationError(3, "Silero VAD: config.json not found in model directory")
    with open(path) as f:
        cfg = SileroVADConfig.from_dict(json.load(f), **workspace)
    weights = silero_vad_sanitize(read_safetensors_dir(model_dir, missing_code=(3, "Silero VAD: no *.safetensors in model directory")))
    silero_vad_check_weights(cfg, weights)
    return cfg, weights


def silero_vad_chunk_samples(sample_rate: int) -> int:
    """The chunk the host-side thresholding assumes (probsToTimestamps :276, detectSpeechRuns :47): 512 at 16 kHz, else 256."""
    return 512 if int(sample_rate) == 16000 else 256


def silero_vad_probs_to_timestamps(probabilities, audio_len: int, sample_rate: int, threshold: float, min_speech_duration_ms: int,
                                   min_silence_duration_ms: int, speech_pad_ms: int) -> list:
    """probsToTimestamps (SileroVAD.swift:265-329) -> [(start_sample, end_sample)]; a 2-D input gives its first row.  The thresholds and
    the minimum durations are numpy.float32 where the Swift uses Float."""
    probs = np.asarray(probabilities, _F)
    if probs.ndim == 2:
        probs = probs[0]
    chunk = silero_vad_chunk_samples(sample_rate)
    thr = _F(threshold)
    min_speech = _F(sample_rate) * _F(min_speech_duration_ms) / _F(1000)
    min_silence = _F(sample_rate) * _F(min_silence_duration_ms) / _F(1000)
    pad = int(_F(sample_rate) * _F(speech_pad_ms) / _F(1000))
    neg = max(thr - _F(0.15), _F(0.01))
    speeches, triggered, start, temp_end = [], False, 0, 0
    for idx, p in enumerate(probs):
        at = idx * chunk
        if p >= thr and not triggered:
            triggered, start, temp_end = True, at, 0
            continue
        if triggered and p >= thr:
            temp_end = 0
            continue
        if triggered and p < neg:
            if temp_end == 0:
                temp_end = at
            if _F(at - temp_end) >= min_silence:
                if _F(temp_end - start) >= min_speech:
                    speeches.append((start, temp_end))
                triggered, temp_end = False, 0
    if triggered:
        end = min(int(audio_len), len(probs) * chunk)
        if _F(end - start) >= min_speech:
            speeches.append((start, end))
    out = []
    for a, b in speeches:
        a, b = max(0, a - pad), min(int(audio_len), b + pad)
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


@dataclass
class SileroVADStreamingState:
    """SileroVADStreamingState (SileroVAD.swift:17-27): lstm_state f32 [2, batch, 128] or None, context f32 [batch, context_size]."""
    lstm_state: np.ndarray | None
    context: np.ndarray
    sample_rate: int


class SileroVAD(NativeHandle):
    """callAsFunction / initialState / feed / predictProba / getSpeechTimestamps of the reference class, plus ragged batches; one handle,
    1..max_batch rows a call, rows of any length (the engine walks them in passes of max_chunks with the LSTM state kept on the device)."""
    _prefix = "mis_silero_vad"
    STAGES = ("magnitude", "conv1", "conv2", "conv3", "conv4", "gates", "probs")

    def __init__(self, config: SileroVADConfig | None = None, device: int = 0):
        self.config = config if config is not None else SileroVADConfig()
        self.device = device
        self._create(self.config.to_c(), device)

    @classmethod
    def from_weights(cls, config: SileroVADConfig, weights: dict, device: int = 0) -> "SileroVAD":
        """weights: sanitized names (what silero_vad_sanitize returns), all of them and no others."""
        silero_vad_check_weights(config, weights)
        m = cls(config, device)
        for name, arr in weights.items():
            m.set_tensor(name, arr)
        m.finalize()
        return m

    @classmethod
    def synthetic(cls, config: SileroVADConfig | None = None, device: int = 0, seed: int = 777) -> "SileroVAD":
        m = cls(config, device)
        check(_lib.lib().mis_silero_vad_init_synthetic(m._h, seed))
        m.finalize()
        return m

    @classmethod
    def from_model_directory(cls, model_dir: str, device: int = 0, **workspace) -> "SileroVAD":
        cfg, weights = silero_vad_read_directory(model_dir, **workspace)
        return cls.from_weights(cfg, weights, device)

    @classmethod
    def from_pretrained(cls, path: str, device: int = 0, **workspace) -> "SileroVAD":
        """fromPretrained (:346-355) for a local path; this package downloads nothing."""
        p = os.path.expanduser(path)
        if not os.path.isdir(p):
            raise SileroVADError.invalid_repository_id(f"{path} (no local model directory; nothing is downloaded)")
        return cls.from_model_directory(p, device, **workspace)

    sanitize = staticmethod(silero_vad_sanitize)
    probs_to_timestamps = staticmethod(silero_vad_probs_to_timestamps)

    @property
    def launches(self) -> int:
        return int(_lib.lib().mis_silero_vad_launches(self._h))

    # -- one chunk -----------------------------------------------------------------------------------
    def _state_arg(self, state, batch):
        if state is None:
            return None
        st = np.ascontiguousarray(state, _F)
        if st.shape != (2, batch, 128):
            raise AudioGenerationError(3, f"Silero VAD: expected state shape (2, {batch}, 128), got {st.shape}")
        return st

    def __call__(self, x, state=None, sample_rate: int = 16000):
        """callAsFunction (:153-160): windows [n] or [batch, n], n = context_size + chunk_size, state [2, batch, 128] or None ->
        (prob [batch, 1], new state [2, batch, 128])."""
        b = self.config.branch(sample_rate)
        w = np.ascontiguousarray(x, _F)
        if w.ndim == 1:
            w = w[None]
        if w.ndim != 2:
            raise AudioGenerationError(3, f"Silero VAD: windows must be [batch, samples], got shape {w.shape}")
        if w.shape[1] <= b.pad:
            raise SileroVADError.insufficient_reflect_pad_input(w.shape[1], b.pad)
        if w.shape[1] != b.window:
            raise AudioGenerationError(3, f"Silero VAD: a window of {w.shape[1]} samples; the engine serves context_size + chunk_size = {b.window}")
        B = w.shape[0]
        st = self._state_arg(state, B)
        prob, new = np.zeros((B, 1), _F), np.zeros((2, B, 128), _F)
        check(_lib.lib().mis_silero_vad_forward(self._h, w.ctypes.data, B, int(sample_rate), None if st is None else st.ctypes.data,
                                                prob.ctypes.data, new.ctypes.data))
        return prob, new

    def initial_state(self, batch_size: int = 1, sample_rate: int = 16000) -> SileroVADStreamingState:
        b = self.config.branch(sample_rate)
        return SileroVADStreamingState(None, np.zeros((batch_size, b.context_size), _F), int(sample_rate))

    def feed(self, chunk, state: SileroVADStreamingState | None = None, sample_rate: int = 16000):
        """feed (:168-190): chunk [chunk_size] or [batch, chunk_size] -> (prob [batch, 1], the next streaming state)."""
        b = self.config.branch(sample_rate)
        c = np.asarray(chunk, _F)
        if c.ndim == 1:
            c = c[None]
        if c.shape[-1] != b.chunk_size:
            raise SileroVADError.unexpected_chunk_size(b.chunk_size, c.shape[-1])
        st = state if state is not None else self.initial_state(c.shape[0], sample_rate)
        if st.sample_rate != int(sample_rate):
            raise SileroVADError.state_sample_rate_mismatch(st.sample_rate, int(sample_rate))
        prob, lstm = self(np.concatenate([st.context, c], axis=-1), st.lstm_state, sample_rate)
        return prob, SileroVADStreamingState(lstm, c[:, c.shape[-1] - b.context_size:].copy(), int(sample_rate))

    # -- whole rows ----------------------------------------------------------------------------------
    def chunks(self, lens, sample_rate: int = 16000) -> np.ndarray:
        lens = np.ascontiguousarray(lens, np.int64)
        out = np.zeros(len(lens), np.int32)
        check(_lib.lib().mis_silero_vad_chunks(self._h, lens.ctypes.data, len(lens), int(sample_rate), out.ctypes.data))
        return out

    def predict_proba_batch(self, waveforms, sample_rate: int = 16000, state=None, junk: float | None = None, return_state: bool = False):
        """Ragged list of 1-D waveforms -> one float32 array of probabilities per row (an empty row gives an empty array); with
        return_state also the LSTM state [2, B, 128] behind every row's last chunk.  state: the state to start from, or None."""
        self.config.branch(sample_rate)
        rows = [np.asarray(w, _F) for w in waveforms]
        if not rows or any(r.ndim != 1 for r in rows):
            raise AudioGenerationError(3, "Silero VAD: a non-empty list of one-dimensional waveforms is expected")
        pcm, lens = pack_rows(rows, junk)
        B, stride = pcm.shape
        st = self._state_arg(state, B)
        nc = self.chunks(lens, sample_rate) if B <= self.config.max_batch else np.zeros(B, np.int32)
        cols = max(1, int(nc.max()))
        probs, new = np.zeros((B, cols), _F), np.zeros((2, B, 128), _F)
        check(_lib.lib().mis_silero_vad_predict(self._h, pcm.ctypes.data, lens.ctypes.data, B, stride, int(sample_rate), probs.ctypes.data, cols,
                                                None if st is None else st.ctypes.data, new.ctypes.data))
        out = [probs[b, : nc[b]].copy() for b in range(B)]
        return (out, new) if return_state else out

    def predict_proba(self, audio, sample_rate: int = 16000) -> np.ndarray:
        """predictProba (:192-241): audio [n] -> [chunks], audio [B, n] -> [B, chunks]; no samples give no chunks."""
        self.config.branch(sample_rate)
        a = np.asarray(audio, _F)
        if a.ndim not in (1, 2):
            raise AudioGenerationError(3, f"Silero VAD: audio must be [samples] or [batch, samples], got shape {a.shape}")
        if a.shape[-1] == 0:
            return np.zeros(a.shape, _F)
        out = np.stack(self.predict_proba_batch(list(a[None] if a.ndim == 1 else a), sample_rate))
        return out[0] if a.ndim == 1 else out

    def get_speech_timestamps(self, audio, sample_rate: int = 16000, threshold=None, min_speech_duration_ms=None, min_silence_duration_ms=None,
                              speech_pad_ms=None) -> list:
        """getSpeechTimestamps (:243-263) -> [(start_sample, end_sample)]."""
        a = np.asarray(audio, _F)
        c = self.config
        return silero_vad_probs_to_timestamps(
            self.predict_proba(a, sample_rate), a.shape[-1], sample_rate, c.threshold if threshold is None else threshold,
            c.min_speech_duration_ms if min_speech_duration_ms is None else min_speech_duration_ms,
            c.min_silence_duration_ms if min_silence_duration_ms is None else min_silence_duration_ms,
            c.speech_pad_ms if speech_pad_ms is None else speech_pad_ms)

    def tap(self, stage) -> np.ndarray:
        """Tensors of the last pass of the last call, [B, P, frames, width] (P the pass's chunks; zeros behind a row's own): 0 magnitude,
        1..4 conv1..conv4, 5 gate pre-activations Wx x + bias, 6 probabilities [B, P].  A stage may be given by its name in STAGES."""
        stage = self.STAGES.index(stage) if isinstance(stage, str) else int(stage)
        dims = (C.c_int64 * 3)()
        check(_lib.lib().mis_silero_vad_tap(self._h, stage, None, 0, dims))
        out = np.zeros(tuple(int(d) for d in dims), _F)
        check(_lib.lib().mis_silero_vad_tap(self._h, stage, out.ctypes.data, out.size, dims))
        if stage == 6:
            return out[:, :, 0]
        P = self.tap(6).shape[1]
        return out.reshape(out.shape[0], P, out.shape[1] // P, out.shape[2])

    def timing(self):
        """Device milliseconds of the last call: (front end, recurrence)."""
        ms = (C.c_float * 2)()
        check(_lib.lib().mis_debug_silero_vad_timing(self._h, ms))
        return float(ms[0]), float(ms[1])


# ------------------------------------------------------------------------------------------------------------ segmentSpeech
@dataclass
class SpeechSegmentConfig:
    """SpeechSegmentConfig (SpeechSegmenter.swift:6-29)."""
    threshold: float = 0.5
    min_speech_ms: int = 250
    min_silence_ms: int = 100
    speech_pad_ms: int = 30
    merge_gap_s: float = 1.0
    max_chunk_s: float = 30.0


_BLOCKS_PER_256MS = 8


def speech_runs_from_probs(probs, n_samples: int, sample_rate: int, config: SpeechSegmentConfig | None = None) -> list:
    """The part of detectSpeechRuns (SpeechSegmenter.swift:47-112) behind predictProba: per-chunk probabilities -> [(start_sample,
    end_sample)].  Eight chunks form a ~256 ms block of probability 1 - prod(1 - p) in float32; the minimum durations round UP."""
    cfg = config if config is not None else SpeechSegmentConfig()
    p32 = np.asarray(probs, _F).ravel()
    block_samples = silero_vad_chunk_samples(sample_rate) * _BLOCKS_PER_256MS
    block_s = _F(block_samples) / _F(sample_rate)
    nb = len(p32) // _BLOCKS_PER_256MS
    if nb == 0:
        return []
    one = _F(1.0)
    p256 = np.zeros(nb, _F)
    for i in range(nb):
        prod = one
        for k in range(_BLOCKS_PER_256MS):
            prod = _F(prod * _F(one - p32[i * _BLOCKS_PER_256MS + k]))
        p256[i] = one - prod
    pad_blocks = max(0, int(_F(cfg.speech_pad_ms) / _F(1000) / block_s))
    min_speech = max(1, int(np.ceil(_F(cfg.min_speech_ms) / _F(1000) / block_s)))
    min_silence = max(1, int(np.ceil(_F(cfg.min_silence_ms) / _F(1000) / block_s)))
    thr = _F(cfg.threshold)
    runs, in_speech, seg_start, last_speech, silent = [], False, 0, -1, 0

    def close(seg_end):
        if seg_end - seg_start >= min_speech:
            s, e = seg_start * block_samples, min(seg_end * block_samples, int(n_samples))
            if s < e:
                runs.append((s, e))

    for idx, p in enumerate(p256):
        if p >= thr:
            if not in_speech:
                seg_start, in_speech = max(0, idx - pad_blocks), True
            last_speech, silent = idx, 0
        elif in_speech:
            silent += 1
            if silent >= min_silence:
                close(min(last_speech + 1 + pad_blocks, nb))
                in_speech, silent, last_speech = False, 0, -1
    if in_speech:
        close(min(nb, last_speech + 1 + pad_blocks))
    return runs


def _mono(audio) -> np.ndarray:
    a = np.asarray(audio, _F)
    return a.mean(axis=-1, dtype=_F) if a.ndim > 1 else a


def detect_speech_runs(audio, sample_rate: int, vad_model, config: SpeechSegmentConfig | None = None) -> list:
    """detectSpeechRuns (SpeechSegmenter.swift:38-113): vad_model.predict_proba, then speech_runs_from_probs."""
    a = _mono(audio)
    return speech_runs_from_probs(vad_model.predict_proba(a, sample_rate), len(a), sample_rate, config)


def segment_speech(audio, sample_rate: int, vad_model, config: SpeechSegmentConfig | None = None) -> list:
    """segmentSpeech (SpeechSegmenter.swift:162-183) -> [(segment, offset_s)]: silence dropped, runs within merge_gap_s merged, long runs
    cut at max_chunk_s (merge_runs, shared with chunks_from_segments); the whole buffer at offset 0 when no speech is found.  audio with
    more than one dimension is averaged over its last."""
    cfg = config if config is not None else SpeechSegmentConfig()
    a = _mono(audio)
    raw = detect_speech_runs(a, sample_rate, vad_model, cfg)
    if not raw:
        return [(a, 0.0)]
    return [(a[s:e], float(_F(s) / _F(sample_rate))) for s, e in merge_runs(raw, sample_rate, cfg.merge_gap_s, cfg.max_chunk_s)]
