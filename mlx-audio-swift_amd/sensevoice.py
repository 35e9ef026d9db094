"""SenseVoice speech-to-text, host mirror of `SenseVoiceModel` (Sources/MLXAudioSTT/Models/SenseVoice/SenseVoiceModel.swift),
`SenseVoiceConfig` (SenseVoiceConfig.swift) and `SenseVoiceTokenizer` (SenseVoiceTokenizer.swift).  Configuration, checkpoint key
handling, CMVN and tokenizer loading, the ragged-batch packing and the id -> name maps stay on the host; the fbank front end, the LFR /
CMVN / query intake, the SAN-M encoder, the CTC head with its fused arg-max and the greedy collapse run in libmi_speech.so
(csrc/sensevoice.hip).  No tensor arithmetic happens here."""
from __future__ import annotations

import ctypes as C
import json
import os
import struct
import time
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._handle import NativeHandle, pack_rows, read_safetensors_dir
from .generation import AudioGenerationError, check
from .lasr import SentencePieceTokenizer
from .stt import STTGenerateParameters, STTOutput
from .vad import parse_kaldi_cmvn

_F = np.float32

LID_IDS = {"auto": 0, "zh": 3, "en": 4, "yue": 7, "ja": 11, "ko": 12, "nospeech": 13}                    # lidDict (:301-311)
TEXTNORM_IDS = {"withitn": 14, "woitn": 15}                                                              # textnormDict (:313-318)
LID_MAP = {24884: "zh", 24885: "en", 24888: "yue", 24892: "ja", 24896: "ko", 24992: "nospeech"}          # extractRichInfo (:412-436)
EMO_MAP = {25001: "happy", 25002: "sad", 25003: "angry", 25004: "neutral", 25005: "fearful", 25006: "disgusted", 25007: "surprised",
           25008: "other", 25009: "unk"}
EVENT_MAP = {24993: "Speech", 24995: "BGM", 24997: "Laughter", 24999: "Applause"}

_ENC_KEYS = ("output_size", "attention_heads", "linear_units", "num_blocks", "tp_blocks", "dropout_rate", "positional_dropout_rate",
             "attention_dropout_rate", "kernel_size", "sanm_shift", "normalize_before")
_FRONT_KEYS = ("fs", "window", "n_mels", "frame_length", "frame_shift", "lfr_m", "lfr_n")


@dataclass
class SenseVoiceEncoderConfig:
    """SenseVoiceEncoderConfig (SenseVoiceConfig.swift:3-73), every field and default."""
    output_size: int = 512
    attention_heads: int = 4
    linear_units: int = 2048
    num_blocks: int = 50
    tp_blocks: int = 20
    dropout_rate: float = 0.1
    positional_dropout_rate: float = 0.1
    attention_dropout_rate: float = 0.1
    kernel_size: int = 11
    sanm_shift: int = 0
    normalize_before: bool = True

    @classmethod
    def from_dict(cls, d: dict) -> "SenseVoiceEncoderConfig":
        """init(from:) (:57-72): missing or null keys take the defaults; `sanm_shfit` (sic) is read when `sanm_shift` is absent."""
        kw = {k: d[k] for k in _ENC_KEYS if d.get(k) is not None}
        if "sanm_shift" not in kw and d.get("sanm_shfit") is not None:
            kw["sanm_shift"] = d["sanm_shfit"]
        return cls(**kw)


@dataclass
class SenseVoiceFrontendConfig:
    """SenseVoiceFrontendConfig (SenseVoiceConfig.swift:75-122), every field and default."""
    fs: int = 16000
    window: str = "hamming"
    n_mels: int = 80
    frame_length: int = 25
    frame_shift: int = 10
    lfr_m: int = 7
    lfr_n: int = 6

    @classmethod
    def from_dict(cls, d: dict) -> "SenseVoiceFrontendConfig":
        return cls(**{k: d[k] for k in _FRONT_KEYS if d.get(k) is not None})


@dataclass
class SenseVoiceConfig:
    """SenseVoiceConfig (SenseVoiceConfig.swift:124-173).  max_batch / max_seconds / head_rows size the engine's workspace (rows a call,
    the longest row, the frames a chunk of forward's logits scratch) and are not part of a checkpoint."""
    model_type: str = "sensevoice"
    vocab_size: int = 25055
    input_size: int = 560
    encoder_conf: SenseVoiceEncoderConfig = field(default_factory=SenseVoiceEncoderConfig)
    frontend_conf: SenseVoiceFrontendConfig = field(default_factory=SenseVoiceFrontendConfig)
    cmvn_means: list | None = None
    cmvn_istd: list | None = None
    max_batch: int = 8
    max_seconds: int = 30
    head_rows: int = 2048

    @classmethod
    def from_dict(cls, d: dict, **workspace) -> "SenseVoiceConfig":
        kw = {k: d[k] for k in ("model_type", "vocab_size", "input_size", "cmvn_means", "cmvn_istd") if d.get(k) is not None}
        if isinstance(d.get("encoder_conf"), dict):
            kw["encoder_conf"] = SenseVoiceEncoderConfig.from_dict(d["encoder_conf"])
        if isinstance(d.get("frontend_conf"), dict):
            kw["frontend_conf"] = SenseVoiceFrontendConfig.from_dict(d["frontend_conf"])
        return cls(**kw, **workspace)

    @property
    def num_layers(self) -> int:
        return 1 + max(self.encoder_conf.num_blocks - 1, 0) + self.encoder_conf.tp_blocks

    def to_c(self) -> "_lib.SenseVoiceConfigC":
        e, f = self.encoder_conf, self.frontend_conf
        return _lib.SenseVoiceConfigC(self.vocab_size, self.input_size, e.output_size, e.attention_heads, e.linear_units, e.num_blocks, e.tp_blocks,
                                      e.kernel_size, e.sanm_shift, int(e.normalize_before), f.fs, f.n_mels, f.frame_length, f.frame_shift,
                                      f.lfr_m, f.lfr_n, int("hann" in f.window.lower()), self.max_batch, self.max_seconds, self.head_rows)


def sensevoice_layer_prefixes(config: SenseVoiceConfig) -> list:
    """The layers in the order they run: encoders0.0, encoders.N, tp_encoders.N."""
    e = config.encoder_conf
    return (["encoder.encoders0.0"] + [f"encoder.encoders.{i}" for i in range(max(e.num_blocks - 1, 0))]
            + [f"encoder.tp_encoders.{i}" for i in range(e.tp_blocks)])


def sensevoice_expected_shapes(config: SenseVoiceConfig) -> dict:
    """name -> shape of every parameter of SenseVoiceModel(config): what update(parameters:verify: .all) accepts (:553-556).  The
    depthwise weight is in MLX's layout [channels, kernel, 1], which is what the engine takes."""
    e = config.encoder_conf
    D, Fd = e.output_size, e.linear_units
    s = {"embed.weight": (16, config.input_size)}

    def lin(p, o, i):
        s[p + ".weight"], s[p + ".bias"] = (o, i), (o,)

    for n, q in enumerate(sensevoice_layer_prefixes(config)):
        cin = config.input_size if n == 0 else D
        s[q + ".norm1.weight"], s[q + ".norm1.bias"] = (cin,), (cin,)
        s[q + ".norm2.weight"], s[q + ".norm2.bias"] = (D,), (D,)
        lin(q + ".self_attn.linear_q_k_v", 3 * D, cin)
        lin(q + ".self_attn.linear_out", D, D)
        s[q + ".self_attn.fsmn_block.weight"] = (D, e.kernel_size, 1)
        lin(q + ".feed_forward.w_1", Fd, D)
        lin(q + ".feed_forward.w_2", D, Fd)
    for q in ("encoder.after_norm", "encoder.tp_norm"):
        s[q + ".weight"], s[q + ".bias"] = (D,), (D,)
    lin("ctc_lo", config.vocab_size, D)
    return s


def sensevoice_expected_keys(config: SenseVoiceConfig) -> set:
    return set(sensevoice_expected_shapes(config))


def sensevoice_sanitize(weights: dict, config: SenseVoiceConfig | None = None) -> dict:
    """SenseVoiceModel.sanitize (:515-531): `ctc.ctc_lo.` -> `ctc_lo.`; a 3-D `fsmn_block.weight` in torch's layout [channels, 1, kernel]
    is transposed (0, 2, 1) to MLX's [channels, kernel, 1], the layout the engine takes.  The layout is told by the shape: a weight
    whose last dimension is 1 already is MLX's and passes through (the reference transposes whatever it gets, so it cannot load its own
    converted checkpoints twice; both hold the same values in the same order)."""
    out = {}
    for key, v in weights.items():
        key = key.replace("ctc.ctc_lo.", "ctc_lo.")
        if "fsmn_block.weight" in key and v.ndim == 3 and not (v.shape[2] == 1 and v.shape[1] != 1):
            v = v.transpose(0, 2, 1) if isinstance(v, np.ndarray) else v.permute(0, 2, 1)
        out[key] = v
    return out


def sensevoice_check_weights(config: SenseVoiceConfig, weights: dict):
    want = sensevoice_expected_shapes(config)
    unknown, missing = sorted(set(weights) - set(want)), sorted(set(want) - set(weights))
    if unknown or missing:
        raise AudioGenerationError(3, f"SenseVoice checkpoint: unexpected keys {unknown[:4]}, missing keys {missing[:4]}")
    bad = [k for k in want if tuple(weights[k].shape) != want[k]]
    if bad:
        raise AudioGenerationError(3, f"SenseVoice checkpoint: {bad[0]} has shape {tuple(weights[bad[0]].shape)}, expected {want[bad[0]]}")


def normalized_language(language) -> str:
    """normalizedLanguage (:337-355)."""
    if language is None:
        return "auto"
    return {"zh": "zh", "chinese": "zh", "mandarin": "zh", "en": "en", "english": "en", "yue": "yue", "cantonese": "yue", "ja": "ja",
            "japanese": "ja", "ko": "ko", "korean": "ko", "nospeech": "nospeech"}.get(str(language).lower(), "auto")


def rich_info(lid: int, emo: int, event: int) -> dict:
    """extractRichInfo (:407-443) on the three arg-max ids."""
    return {"language": LID_MAP.get(int(lid), "unknown"), "emotion": EMO_MAP.get(int(emo), f"token_{int(emo)}"),
            "event": EVENT_MAP.get(int(event), f"token_{int(event)}")}


# ------------------------------------------------------------------------------------------------------------ tokenizer
def read_sentencepiece_pieces(data: bytes) -> list:
    """The piece list of a SentencePiece ModelProto: [(piece, score, type)] from every field 1 (SentencePiece: 1 piece, 2 score, 3 type;
    type defaults to 1 NORMAL).  A plain protobuf wire reader; nothing else of the model is read."""

    def varint(buf, at):
        v = shift = 0
        while True:
            if at >= len(buf):
                raise AudioGenerationError(3, "SentencePiece model: truncated varint")
            b = buf[at]
            at += 1
            v |= (b & 0x7F) << shift
            if not b & 0x80:
                return v, at
            shift += 7
            if shift > 63:
                raise AudioGenerationError(3, "SentencePiece model: bad varint")

    def fields(buf):
        at = 0
        while at < len(buf):
            tag, at = varint(buf, at)
            num, wt = tag >> 3, tag & 7
            if wt == 0:
                v, at = varint(buf, at)
            elif wt == 1:
                v, at = buf[at: at + 8], at + 8
            elif wt == 2:
                n, at = varint(buf, at)
                v, at = buf[at: at + n], at + n
            elif wt == 5:
                v, at = buf[at: at + 4], at + 4
            else:
                raise AudioGenerationError(3, f"SentencePiece model: wire type {wt}")
            if at > len(buf):
                raise AudioGenerationError(3, "SentencePiece model: truncated field")
            yield num, wt, v

    pieces = []
    for num, wt, v in fields(bytes(data)):
        if num != 1 or wt != 2:
            continue
        piece, score, kind = "", 0.0, 1
        for n2, w2, v2 in fields(v):
            if n2 == 1 and w2 == 2:
                piece = v2.decode("utf-8", errors="replace")
            elif n2 == 2 and w2 == 5:
                score = struct.unpack("<f", v2)[0]
            elif n2 == 3 and w2 == 0:
                kind = int(v2)
        pieces.append((piece, score, kind))
    return pieces


class SenseVoiceTokenizer:
    """SenseVoiceTokenizer (SenseVoiceTokenizer.swift): tokenizer.json, else the first *.model in name order, else tokens.json, else the
    ids joined by spaces.  `tokenizer` is a SentencePieceTokenizer or None, `token_list` a list of pieces or None."""

    def __init__(self, tokenizer=None, token_list=None):
        self.tokenizer, self.token_list = tokenizer, token_list

    @classmethod
    def from_model_directory(cls, model_dir: str) -> "SenseVoiceTokenizer":
        tokenizer = None
        tj = os.path.join(model_dir, "tokenizer.json")
        models = sorted(fn for fn in os.listdir(model_dir) if fn.endswith(".model"))
        if os.path.isfile(tj):
            tokenizer = SentencePieceTokenizer.from_tokenizer_json(tj)
        elif models:
            with open(os.path.join(model_dir, models[0]), "rb") as f:
                pieces = read_sentencepiece_pieces(f.read())
            tokenizer = SentencePieceTokenizer([p for p, _, _ in pieces], {i for i, (_, _, k) in enumerate(pieces) if k in (3, 5)})
        token_list = None
        tk = os.path.join(model_dir, "tokens.json")
        if os.path.isfile(tk):
            with open(tk, encoding="utf-8") as f:
                token_list = [str(t) for t in json.load(f)]
        return cls(tokenizer, token_list)

    def decode(self, ids) -> str:
        if self.tokenizer is not None:
            return self.tokenizer.decode(ids)
        if self.token_list is not None:
            return "".join(self.token_list[int(i)] for i in ids if 0 <= int(i) < len(self.token_list)).replace("▁", " ").strip(" \t")
        return " ".join(str(int(i)) for i in ids)


def sensevoice_read_directory(model_dir: str, **workspace):
    """config.json, every *.safetensors in name order, am.mvn (else the config's lists, else none) and the tokenizer of a model directory
    (fromDirectory :533-560, loadAssets :498-513) -> (config, sanitized weights, cmvn or None, tokenizer or None).  No device is touched."""
    path = os.path.join(model_dir, "config.json")
    if not os.path.isfile(path):
        raise AudioGenerationError(3, "SenseVoice: config.json not found in model directory")
    with open(path) as f:
        cfg = SenseVoiceConfig.from_dict(json.load(f), **workspace)
    weights = sensevoice_sanitize(read_safetensors_dir(model_dir, missing_code=(3, "SenseVoice: no *.safetensors in model directory")))
    sensevoice_check_weights(cfg, weights)
    cmvn = None
    mvn = os.path.join(model_dir, "am.mvn")
    if os.path.isfile(mvn):
        with open(mvn, "rb") as f:
            cmvn = parse_kaldi_cmvn(f.read())
    elif cfg.cmvn_means is not None and cfg.cmvn_istd is not None:
        cmvn = (np.asarray(cfg.cmvn_means, _F), np.asarray(cfg.cmvn_istd, _F))
    tokenizer = None
    try:                                                              # `try?`: a tokenizer that does not load is no error
        t = SenseVoiceTokenizer.from_model_directory(model_dir)
        if t.tokenizer is not None or t.token_list is not None:
            tokenizer = t
    except Exception:
        tokenizer = None
    return cfg, weights, cmvn, tokenizer


# ------------------------------------------------------------------------------------------------------------ the model
class SenseVoiceModel(NativeHandle):
    """generate / generateStream / callAsFunction of the reference class, plus ragged batches; one handle, 1..max_batch rows a call."""
    _prefix = "mis_sensevoice"

    def __init__(self, config: SenseVoiceConfig, tokenizer: SenseVoiceTokenizer | None = None, device: int = 0):
        self.config, self.tokenizer, self.device = config, tokenizer, device
        self.has_cmvn = False
        self._create(config.to_c(), device)

    default_generation_parameters = STTGenerateParameters(max_tokens=0, temperature=0.0, language="auto")        # :283-292
    sanitize = staticmethod(sensevoice_sanitize)
    normalized_language = staticmethod(normalized_language)

    @classmethod
    def from_weights(cls, config: SenseVoiceConfig, weights: dict, cmvn=None, tokenizer=None, device: int = 0) -> "SenseVoiceModel":
        """weights: sanitized names (what sensevoice_sanitize returns), all of them and no others; cmvn: (means, istd) or None."""
        sensevoice_check_weights(config, weights)
        m = cls(config, tokenizer, device)
        for name, arr in weights.items():
            m.set_tensor(name, arr)
        if cmvn is not None:
            m.set_tensor("cmvn.shift", np.ascontiguousarray(cmvn[0], _F))
            m.set_tensor("cmvn.scale", np.ascontiguousarray(cmvn[1], _F))
            m.has_cmvn = True
        m.finalize()
        return m

    @classmethod
    def synthetic(cls, config: SenseVoiceConfig, device: int = 0, seed: int = 777) -> "SenseVoiceModel":
        m = cls(config, None, device)
        check(_lib.lib().mis_sensevoice_init_synthetic(m._h, seed))
        m.has_cmvn = True
        m.finalize()
        return m

    @classmethod
    def from_model_directory(cls, model_dir: str, device: int = 0, **workspace) -> "SenseVoiceModel":
        cfg, weights, cmvn, tokenizer = sensevoice_read_directory(model_dir, **workspace)
        return cls.from_weights(cfg, weights, cmvn, tokenizer, device)

    @classmethod
    def from_pretrained(cls, path: str, device: int = 0, **workspace) -> "SenseVoiceModel":
        """fromPretrained (:562-581) for a local path; this package downloads nothing."""
        p = os.path.expanduser(path)
        if not os.path.isdir(p):
            raise AudioGenerationError(3, f"SenseVoice: {path} is no local model directory (nothing is downloaded)")
        return cls.from_model_directory(p, device, **workspace)

    @property
    def launches(self) -> int:
        return int(_lib.lib().mis_sensevoice_launches(self._h))

    # -- inputs --------------------------------------------------------------------------------------
    @staticmethod
    def _mono(audio) -> np.ndarray:
        """computeFbank :17-21: audio with more than one dimension is averaged over its last, then flattened."""
        a = np.asarray(audio, _F)
        if a.ndim > 1:
            a = a.mean(axis=-1, dtype=_F)
        return np.ascontiguousarray(a.reshape(-1), _F)

    def _pack(self, audios, junk=None):
        rows = [self._mono(w) for w in audios]
        if not rows:
            raise AudioGenerationError(3, "SenseVoice: no rows")
        return pack_rows(rows, junk)

    @staticmethod
    def _query(language, use_itn):
        return LID_IDS.get(language if language in LID_IDS else normalized_language(language), 0), TEXTNORM_IDS["withitn" if use_itn else "woitn"]

    def frames(self, lens):
        """Sample counts -> (fbank frames F, sequence rows T = 4 + ceil(F / lfr_n)), int32 arrays."""
        lens = np.ascontiguousarray(lens, np.int64)
        F, T = np.zeros(len(lens), np.int32), np.zeros(len(lens), np.int32)
        check(_lib.lib().mis_sensevoice_frames(self._h, lens.ctypes.data, len(lens), F.ctypes.data, T.ctypes.data))
        return F, T

    # -- calls ---------------------------------------------------------------------------------------
    def features(self, audios, junk=None):
        """extractFeatures (:320-335) for a ragged list: (features [B, Rmax, input_size], R [B]), zeros behind a row's own R = T - 4."""
        pcm, lens = self._pack(audios, junk)
        _, T = self.frames(lens)
        R = T - 4
        out = np.zeros((len(lens), max(1, int(R.max())), self.config.input_size), _F)
        check(_lib.lib().mis_sensevoice_features(self._h, pcm.ctypes.data, lens.ctypes.data, len(lens), pcm.shape[1], out.ctypes.data, out.shape[1]))
        return out[:, : int(R.max())], R

    def forward(self, audios, language="auto", use_itn: bool = False, junk=None):
        """Front end + callAsFunction for a ragged list: (log-probabilities [B, Tmax, vocab], T [B]), zeros behind a row's own T."""
        pcm, lens = self._pack(audios, junk)
        lid, tn = self._query(language, use_itn)
        _, T = self.frames(lens)
        out = np.zeros((len(lens), int(T.max()), self.config.vocab_size), _F)
        check(_lib.lib().mis_sensevoice_forward(self._h, pcm.ctypes.data, lens.ctypes.data, len(lens), pcm.shape[1], lid, tn, out.ctypes.data))
        return out, T

    def __call__(self, feats, language="auto", use_itn: bool = False, counts=None) -> np.ndarray:
        """callAsFunction (:377-390): features [B, R, input_size] (or [R, input_size]) -> log-probabilities [B, 4 + R, vocab];
        counts[B]: valid rows each."""
        f = np.ascontiguousarray(feats, dtype=_F)
        if f.ndim == 2:
            f = f[None]
        if f.ndim != 3 or f.shape[2] != self.config.input_size:
            raise AudioGenerationError(3, f"SenseVoice: features of shape {f.shape}, expected [batch, rows, {self.config.input_size}]")
        B, R = f.shape[0], f.shape[1]
        cn = None if counts is None else np.ascontiguousarray(counts, dtype=np.int32)
        if cn is not None and cn.shape != (B,):
            raise AudioGenerationError(3, "SenseVoice: one row count per batch row is expected")
        lid, tn = self._query(language, use_itn)
        out = np.zeros((B, 4 + R, self.config.vocab_size), _F)
        check(_lib.lib().mis_sensevoice_forward_features(self._h, f.ctypes.data, None if cn is None else cn.ctypes.data, B, R, lid, tn,
                                                         out.ctypes.data))
        return out

    def generate_tokens(self, audios, language="auto", use_itn: bool = False, junk=None):
        """Greedy CTC ids and the three rich ids of a ragged list, decoded on the device: ([ids] per row, rich int32 [B, 3])."""
        pcm, lens = self._pack(audios, junk)
        lid, tn = self._query(language, use_itn)
        _, T = self.frames(lens)
        stride = max(1, int(T.max()) - 4)
        toks, n, rich = np.zeros((len(lens), stride), np.int32), np.zeros(len(lens), np.int32), np.zeros((len(lens), 3), np.int32)
        check(_lib.lib().mis_stt_sensevoice_generate(self._h, pcm.ctypes.data, lens.ctypes.data, len(lens), pcm.shape[1], lid, tn,
                                                     toks.ctypes.data, stride, n.ctypes.data, rich.ctypes.data))
        return [toks[b, : n[b]].tolist() for b in range(len(lens))], rich

    def decode_text(self, tokens) -> str:
        return self.tokenizer.decode(tokens) if self.tokenizer is not None else " ".join(str(t) for t in tokens)

    def _output(self, tokens, rich, seconds) -> STTOutput:
        text, info = self.decode_text(tokens), rich_info(*rich)
        return STTOutput(text=text, segments=[{"text": text, "language": info["language"], "emotion": info["emotion"], "event": info["event"]}],
                         language=info["language"], prompt_tokens=0, generation_tokens=len(tokens), total_tokens=len(tokens), prompt_tps=0.0,
                         generation_tps=len(tokens) / max(seconds, 0.001), total_time=seconds, peak_memory_usage=0.0, token_ids=[list(tokens)])

    def generate_batch(self, audios, generation_parameters=None, language=None, use_itn: bool = False) -> list:
        """generate for a ragged batch (the chunks of chunks_from_segments): one STTOutput per row."""
        start = time.perf_counter()
        if language is None:
            language = normalized_language(getattr(generation_parameters, "language", None))
        rows, rich = self.generate_tokens(audios, language, use_itn)
        seconds = time.perf_counter() - start
        return [self._output(r, rich[b], seconds) for b, r in enumerate(rows)]

    def generate(self, audio, generation_parameters=None, language=None, use_itn: bool = False, verbose: bool = False) -> STTOutput:
        """generate (:445-485): one waveform -> text, one segment with text / language / emotion / event, language."""
        out = self.generate_batch([audio], generation_parameters, language, use_itn)[0]
        if verbose:
            seg = out.segments[0]
            print(f"Language: {seg['language']}\nEmotion: {seg['emotion']}\nEvent: {seg['event']}\nText: {out.text}")
        return out

    def generate_stream(self, audio, generation_parameters=None):
        """generateStream (:487-496): one ("result", STTOutput)."""
        yield ("result", self.generate(audio, generation_parameters))

    def tap(self, stage: int) -> np.ndarray:
        """Tensors of the last call: 0 fbank [B, Fmax, n_mels], 1 intake [B, Tmax, input_size], 2 + i the encoder's stages in the order
        they run [B, Tmax, output_size]: the first stack's layers, after_norm, the tp layers, tp_norm."""
        dims = (C.c_int64 * 3)()
        check(_lib.lib().mis_sensevoice_tap(self._h, stage, None, 0, dims))
        out = np.zeros(tuple(int(d) for d in dims), _F)
        check(_lib.lib().mis_sensevoice_tap(self._h, stage, out.ctypes.data, out.size, dims))
        return out

    def timing(self):
        """Device milliseconds of the last generate / forward: (front end, encoder, head)."""
        ms = (C.c_float * 3)()
        check(_lib.lib().mis_debug_sensevoice_timing(self._h, ms))
        return float(ms[0]), float(ms[1]), float(ms[2])
