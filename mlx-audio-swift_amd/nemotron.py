"""Nemotron ASR speech-to-text (offline, and the cache-aware stream session), host mirror of `NemotronASRModel` (Sources/MLXAudioSTT/Models/NemotronASR/NemotronASRModel.swift,
NemotronASRConfig.swift, NemotronASRTokenizer.swift): the cache-aware FastConformer + RNN-T recogniser.  Configuration, checkpoint key
handling, the language -> prompt index resolution, the piece list and the token times stay on the host; the log-mel front end, the causal
stem, the chunked-limited FastConformer encoder, the prompt kernel, the joint's enc projection and the whole greedy RNN-T loop run in
libmi_speech.so (csrc/nemotron.hip; the stream session NemotronStreamSession: csrc/nemotron_stream.hip).

Refused, not approximated: quantised checkpoints, conv_norm_type other than layer_norm, att_context_style other than chunked_limited /
regular, non-causal downsampling, beam search, rows beyond max_seconds; by the stream session also per_feature normalisation, a left context that is
no multiple of right + 1 and a conv pad that is not causal."""
from __future__ import annotations

import ctypes as C
import json
import os
import time
from dataclasses import dataclass, field, replace

import numpy as np

from . import _lib
from ._handle import _ENCODER_DTYPES, NativeHandle, pack_rows, read_safetensors_dir
from .generation import AudioGenerationError, check
from .parakeet import ParakeetResult, ParakeetToken, parakeet_sanitize
from .sensevoice import read_sentencepiece_pieces

_REGULAR = (0, 1 << 30)              # one chunk holds the row: every query sees every key


def _bad(msg):
    return AudioGenerationError(3, "Nemotron: " + msg)


@dataclass
class NemotronConfig:
    """NemotronASRConfig (NemotronASRConfig.swift) flattened, with its defaults.  max_batch / max_seconds / max_tokens size the workspace and
    are not part of a checkpoint."""
    num_mel_bins: int = 128
    hidden_size: int = 1024
    num_hidden_layers: int = 24
    num_attention_heads: int = 8
    intermediate_size: int = 4096
    conv_kernel_size: int = 9
    conv_context_size: object = "causal"                                  # "causal" or (left, right)
    subsampling_factor: int = 8
    subsampling_conv_channels: int = 256
    att_context_style: str = "chunked_limited"
    att_context_size: list = field(default_factory=lambda: [[56, 13]])
    default_att_context_size: list = None                                 # None: the first listed pair
    attention_bias: bool = False
    scale_input: bool = False
    num_prompts: int = 128                                                # prompt_hidden 0: no prompt kernel
    prompt_hidden: int = 2048
    prompt_dictionary: dict = field(default_factory=dict)
    default_language: str = "auto"
    pred_hidden: int = 640
    pred_rnn_layers: int = 2
    joint_hidden: int = 640
    vocab_size: int = 1024
    max_symbols: int = None                                               # None: no bound but the output capacity
    vocabulary: list = field(default_factory=list)
    sampling_rate: int = 16000
    hop_length: int = 160
    n_fft: int = 512
    win_length: int = 400
    normalize: str = "NA"
    preemphasis: float = 0.97
    max_batch: int = 8
    max_seconds: int = 30
    max_tokens: int = 1024
    encoder_dtype: str = "float32"   # "bfloat16": the Conformer blocks in bf16 (csrc/nemotron_encoder_bf16.h); not part of a checkpoint

    @classmethod
    def from_dict(cls, d: dict, **workspace) -> "NemotronConfig":
        """NemotronASRConfig.init(from:) with its decodeIfPresent defaults."""
        if d.get("quantization") is not None or d.get("quantization_config") is not None:
            raise _bad("quantised checkpoints are not implemented")
        p, e = d.get("preprocessor") or {}, d.get("encoder") or {}
        for k in ("decoder", "joint"):
            if not isinstance(d.get(k), dict):
                raise _bad(f"Missing required Nemotron config field: {k}")
        dec, j = d["decoder"], d["joint"]
        pn, jn = dec.get("prednet") or {}, j.get("jointnet") or {}
        get = lambda a, b, k: a[k] if a.get(k) is not None else b[k]
        if e.get("conv_norm_type", "layer_norm") != "layer_norm":
            raise _bad(f"conv_norm_type {e['conv_norm_type']} is not implemented (layer_norm only)")
        style = e.get("att_context_style", "chunked_limited")
        if style not in ("chunked_limited", "regular"):
            raise _bad(f"att_context_style {style} is not implemented (chunked_limited, regular)")
        if not e.get("causal_downsampling", True):
            raise _bad("non-causal downsampling is not implemented")
        if e.get("self_attention_model", "rel_pos") != "rel_pos":
            raise _bad(f"self_attention_model {e['self_attention_model']} is not implemented (rel_pos only)")
        if get(j, jn, "activation").lower() != "relu":
            raise _bad(f"joint activation {get(j, jn, 'activation')} is not implemented (relu only)")
        if p.get("window", "hann").lower() not in ("hann", "hanning"):
            raise _bad(f"window {p['window']} is not implemented (hann only)")
        if p.get("pad_to", 0):
            raise _bad("pad_to is not implemented")
        cc = e.get("conv_context_size", "causal")
        cc = "causal" if isinstance(cc, str) and cc.lower() == "causal" else (int(cc[0]) if len(cc) > 0 else 0, int(cc[1]) if len(cc) > 1 else 0)
        contexts = [list(x) for x in e.get("att_context_size", [[56, 13]])] or [[56, 13]]
        prompt = d.get("prompt")
        sr = int(p.get("sample_rate", 16000))
        dm = e.get("d_model", 1024)
        return cls(num_mel_bins=int(p.get("features", 128)), hidden_size=dm, num_hidden_layers=e.get("n_layers", 24), num_attention_heads=e.get("n_heads", 8),
                   intermediate_size=dm * e.get("ff_expansion_factor", 4), conv_kernel_size=e.get("conv_kernel_size", 9), conv_context_size=cc,
                   subsampling_factor=e.get("subsampling_factor", 8), subsampling_conv_channels=e.get("subsampling_conv_channels", 256),
                   att_context_style=style, att_context_size=contexts, default_att_context_size=d.get("default_att_context_size"),
                   attention_bias=bool(e.get("use_bias", False)), scale_input=bool(e.get("xscaling", False)),
                   num_prompts=(prompt.get("num_prompts", 128) if prompt is not None else 0),
                   prompt_hidden=(prompt.get("prompt_hidden", 2048) if prompt is not None else 0),
                   prompt_dictionary=dict((prompt or {}).get("prompt_dictionary") or {}),
                   default_language=d.get("default_language") or ("auto" if prompt is not None else "en"),
                   pred_hidden=get(dec, pn, "pred_hidden"), pred_rnn_layers=get(dec, pn, "pred_rnn_layers"), joint_hidden=get(j, jn, "joint_hidden"),
                   vocab_size=dec["vocab_size"], max_symbols=d.get("max_symbols"), vocabulary=list(d.get("vocabulary") or j.get("vocabulary") or []),
                   sampling_rate=sr, hop_length=int(np.float32(p.get("window_stride", 0.01)) * np.float32(sr)), n_fft=int(p.get("n_fft", 512)),
                   win_length=int(np.float32(p.get("window_size", 0.025)) * np.float32(sr)), normalize=p.get("normalize", "NA"),
                   preemphasis=float(p.get("preemph", 0.97) or 0.0), **workspace)

    @property
    def conv_pads(self):
        """NemotronASRConvolution.init: (padLeft, padRight)"""
        return (self.conv_kernel_size - 1, 0) if self.conv_context_size == "causal" else tuple(self.conv_context_size)

    @property
    def contexts(self):
        """the (left, right) pairs the distance table is sized for"""
        return [_REGULAR] if self.att_context_style == "regular" else [tuple(x) for x in self.att_context_size]

    @property
    def default_context(self):
        return _REGULAR if self.att_context_style == "regular" else tuple(self.default_att_context_size or self.att_context_size[0])

    def to_c(self) -> "_lib.NemotronConfigC":
        if (self.normalize or "NA").lower() not in ("per_feature", "na", "none"):
            raise _bad(f"normalize {self.normalize} is not implemented (per_feature, NA)")
        if self.att_context_style not in ("chunked_limited", "regular"):
            raise _bad(f"att_context_style {self.att_context_style} is not implemented (chunked_limited, regular)")
        if len(self.contexts) > 8:
            raise _bad("more than 8 attention contexts")
        ctx = ((C.c_int32 * 2) * 8)(*[(C.c_int32 * 2)(*x) for x in self.contexts])
        pl, pr = self.conv_pads
        return _lib.NemotronConfigC(self.hidden_size, self.num_hidden_layers, self.num_attention_heads, self.intermediate_size, self.num_mel_bins,
                                    self.conv_kernel_size, self.subsampling_factor, self.subsampling_conv_channels, int(self.attention_bias),
                                    int(self.scale_input), pl, pr, len(self.contexts), ctx, self.num_prompts if self.prompt_hidden else 0,
                                    self.prompt_hidden, self.pred_hidden, self.pred_rnn_layers, self.joint_hidden, self.vocab_size,
                                    int(self.max_symbols or 0), self.sampling_rate, self.hop_length, self.n_fft, self.win_length,
                                    int((self.normalize or "NA").lower() == "per_feature"), self.max_batch, self.max_seconds, self.max_tokens,
                                    self.preemphasis)


def nemotron_sanitize(weights: dict) -> dict:
    """NeMo / MLX checkpoint names -> the engine's (mi_speech.h): parakeet_sanitize's renames and conv layouts told by shape (pre_encode ->
    subsampling.layers_N / linear, linear_* / pos_bias_* -> *_proj / bias_*, conv.batch_norm - here a LayerNorm - -> conv.norm, joint_net.2,
    MLX's lstm.N.{Wx,Wh,bias}), and prompt_kernel.{0,2} -> prompt_kernel.linear{0,2} (remapKey)."""
    if any(k.endswith((".scales", ".biases")) for k in weights):
        raise _bad("quantised checkpoints are not implemented")
    ren = {}
    for k, v in weights.items():
        for n in ("0", "2"):
            if k.startswith(f"prompt_kernel.{n}."):
                k = f"prompt_kernel.linear{n}." + k[len(f"prompt_kernel.{n}."):]
        ren[k] = v
    return parakeet_sanitize(ren)


def nemotron_expected_keys(config: NemotronConfig) -> set:
    keys = set()

    def lin(p, bias=True):
        keys.add(p + ".weight")
        if bias:
            keys.add(p + ".bias")

    ab = config.attention_bias
    for n in ("layers_0", "layers_2", "layers_3", "layers_5", "layers_6", "linear"):
        lin("encoder.subsampling." + n)
    for i in range(config.num_hidden_layers):
        q = f"encoder.layers.{i}."
        for n in ("norm_feed_forward1", "norm_self_att", "norm_conv", "norm_feed_forward2", "norm_out", "conv.norm"):
            lin(q + n)
        for n in ("feed_forward1.linear1", "feed_forward1.linear2", "feed_forward2.linear1", "feed_forward2.linear2", "conv.pointwise_conv1",
                  "conv.depthwise_conv", "conv.pointwise_conv2", "self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj"):
            lin(q + n, ab)
        lin(q + "self_attn.relative_k_proj", False)
        keys.update(q + "self_attn." + n for n in ("bias_u", "bias_v"))
    if config.prompt_hidden:
        lin("prompt_kernel.linear0"); lin("prompt_kernel.linear2")
    keys.add("decoder.prediction.embed.weight")
    for l in range(config.pred_rnn_layers):
        keys.update(f"decoder.prediction.dec_rnn.lstm.{n}_l{l}" for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
    for n in ("enc", "pred", "joint_net"):
        lin("joint." + n)
    return keys


def _is_special(piece: str) -> bool:
    """NemotronASRTokenizer.isSpecialToken"""
    tag = piece.startswith("<") and piece.endswith(">") and "-" in piece
    return tag or (piece.startswith("<|") and piece.endswith("|>")) or piece in ("<unk>", "<pad>")


class NemotronASR(NativeHandle):
    """generate / generateBatch of the reference class through its offline decode(); 1..max_batch ragged rows a device call, each with its own
    language."""
    _prefix = "mis_nemotron"

    def __init__(self, config: NemotronConfig, device: int = 0):
        self.config, self.device = config, device
        self._create(config.to_c(), device)
        if config.encoder_dtype != "float32":
            self.set_encoder_dtype(config.encoder_dtype)

    sanitize = staticmethod(nemotron_sanitize)

    @classmethod
    def from_weights(cls, config: NemotronConfig, weights: dict, device: int = 0, encoder_dtype: str | None = None) -> "NemotronASR":
        """weights: the engine's names (what nemotron_sanitize returns); encoder_dtype overrides the config's."""
        m = cls(replace(config, encoder_dtype=encoder_dtype) if encoder_dtype else config, device)
        for name, arr in weights.items():
            m.set_tensor(name, arr)
        m.finalize()
        return m

    @classmethod
    def synthetic(cls, config: NemotronConfig, device: int = 0, seed: int = 777, encoder_dtype: str | None = None) -> "NemotronASR":
        m = cls(replace(config, encoder_dtype=encoder_dtype) if encoder_dtype else config, device)
        check(_lib.lib().mis_nemotron_init_synthetic(m._h, seed))
        m.finalize()
        return m

    @classmethod
    def from_model_directory(cls, model_dir: str, device: int = 0, **workspace) -> "NemotronASR":
        """fromDirectory: config.json (Infinity / NaN scrubbed), every *.safetensors; the vocabulary of config.json, else the first *.model's.
        workspace: max_batch / max_seconds / max_tokens / encoder_dtype."""
        with open(os.path.join(model_dir, "config.json")) as f:
            text = f.read()
        for tok in ("-Infinity", "Infinity", "NaN"):                     # normalizedConfigData
            text = text.replace(tok, "null")
        config = NemotronConfig.from_dict(json.loads(text), **workspace)
        if not config.vocabulary:
            models = sorted(fn for fn in os.listdir(model_dir) if fn.endswith(".model"))
            if not models:
                raise _bad(f"no vocabulary in config.json and no SentencePiece model in {model_dir}")
            with open(os.path.join(model_dir, models[0]), "rb") as f:
                config.vocabulary = [p[0] for p in read_sentencepiece_pieces(f.read())]

        def on_keys(fn, keys):
            if any(k.endswith((".scales", ".biases")) for k in keys):
                raise _bad(f"{fn} is a quantised checkpoint: not implemented")

        weights = nemotron_sanitize(read_safetensors_dir(model_dir, missing_code=(2, f"No safetensors files found in {model_dir}"), on_keys=on_keys))
        unknown = sorted(set(weights) - nemotron_expected_keys(config))
        if unknown:
            raise _bad(f"checkpoint: unused keys {unknown[:4]}")
        return cls.from_weights(config, weights, device)

    @classmethod
    def from_pretrained(cls, path: str, device: int = 0, **workspace) -> "NemotronASR":
        """Local directories only: nothing is downloaded."""
        if not os.path.isdir(path):
            raise _bad(f"{path} is not a local model directory")
        return cls.from_model_directory(path, device, **workspace)

    # -- sizes ---------------------------------------------------------------------------------------
    @property
    def launches(self) -> int:
        return int(_lib.lib().mis_nemotron_launches(self._h))

    @property
    def expected_launches(self) -> dict:
        L, p = self.config.num_hidden_layers, 2 if self.config.prompt_hidden else 0
        return dict(generate=9 + 15 * L + p, encode=7 + 15 * L)

    def frames(self, lens):
        n = np.ascontiguousarray(lens, dtype=np.int64)
        F, T = np.zeros(len(n), np.int32), np.zeros(len(n), np.int32)
        check(_lib.lib().mis_nemotron_frames(self._h, n.ctypes.data, len(n), F.ctypes.data, T.ctypes.data))
        return F, T

    def frame_seconds(self, frames) -> float:
        c = self.config
        return float(frames * c.subsampling_factor * c.hop_length) / float(c.sampling_rate)

    def resolve_prompt_index(self, language=None) -> int:
        """resolvePromptIndex"""
        d = self.config.prompt_dictionary
        lang = language if language is not None else self.config.default_language
        return int(d.get(lang, d.get(self.config.default_language, 0)))

    def _context(self, att_context_size):
        if att_context_size is None:
            return self.config.default_context
        if self.config.att_context_style == "regular":
            return _REGULAR                                               # the reference builds no mask at all
        left, right = att_context_size
        return int(left), int(right)

    def _pack(self, audios, junk=None):
        rows = [np.asarray(w, np.float32) for w in audios]
        rows = [r.mean(axis=-1, dtype=np.float32) if r.ndim > 1 else r for r in rows]
        if not rows:
            raise _bad("generate_batch requires at least one audio input")
        cap = self.config.max_seconds * self.config.sampling_rate
        for i, r in enumerate(rows):
            if len(r) > cap:
                raise _bad(f"row {i}: {len(r)} samples exceed max_seconds {self.config.max_seconds}")
        return pack_rows(rows, junk)

    # -- device calls --------------------------------------------------------------------------------
    def encode(self, audios, att_context_size=None, junk=None):
        """(encoder output [B, Tmax, hidden], T [B]); zero rows behind a row's own T."""
        pcm, lens = self._pack(audios, junk)
        _, T = self.frames(lens)
        left, right = self._context(att_context_size)
        out = np.zeros((len(lens), int(T.max()), self.config.hidden_size), np.float32)
        check(_lib.lib().mis_nemotron_encode(self._h, pcm.ctypes.data, lens.ctypes.data, len(lens), pcm.shape[1], left, right, out.ctypes.data))
        return out, T

    def decode_raw(self, audios, language=None, att_context_size=None, junk=None) -> list:
        """One device call -> per row dict(tokens, frames (int32 arrays), truncated, steps).  language: one for all rows or one a row."""
        pcm, lens = self._pack(audios, junk)
        B, cap = len(lens), self.config.max_tokens
        langs = language if isinstance(language, (list, tuple)) else [language] * B
        if len(langs) != B:
            raise _bad(f"{len(langs)} languages for {B} rows")
        idx = np.asarray([self.resolve_prompt_index(l) for l in langs], np.int32)
        left, right = self._context(att_context_size)
        tok, frm = (np.zeros((B, cap), np.int32) for _ in range(2))
        cnt, flg, stp = (np.zeros(B, np.int32) for _ in range(3))
        check(_lib.lib().mis_nemotron_generate(self._h, pcm.ctypes.data, lens.ctypes.data, idx.ctypes.data, B, pcm.shape[1], left, right, tok.ctypes.data,
                                               frm.ctypes.data, cnt.ctypes.data, flg.ctypes.data, stp.ctypes.data))
        return [dict(tokens=tok[b, :cnt[b]].copy(), frames=frm[b, :cnt[b]].copy(), truncated=bool(flg[b]), steps=int(stp[b])) for b in range(B)]

    def __call__(self, audios, language=None, att_context_size=None) -> list:
        return self.decode_raw(audios, language, att_context_size)

    def tap(self, stage: int) -> np.ndarray:
        """Tensors of the last encode / generate: 0 the stem, 1..L the blocks, L + 1 the prompt kernel's output, L + 2 joint.enc of it."""
        dims = (C.c_int64 * 3)()
        check(_lib.lib().mis_nemotron_tap(self._h, stage, None, 0, dims))
        out = np.zeros(tuple(int(d) for d in dims), np.float32)
        check(_lib.lib().mis_nemotron_tap(self._h, stage, out.ctypes.data, out.size, dims))
        return out

    def enable_timing(self):
        check(_lib.lib().mis_debug_nemotron_timing(self._h, None))

    def timing(self):
        """Device milliseconds of the last generate: (front end, encoder + prompt + joint.enc, decode); enable_timing() first."""
        ms = (C.c_float * 3)()
        check(_lib.lib().mis_debug_nemotron_timing(self._h, ms))
        return tuple(float(v) for v in ms)

    # -- results -------------------------------------------------------------------------------------
    def _result(self, raw, elapsed) -> ParakeetResult:
        """decode(): special tokens leave the text, not the decoder state; start = t x frame seconds, duration one frame"""
        vocab, toks = self.config.vocabulary, []
        for t, f in zip(raw["tokens"], raw["frames"]):
            piece = vocab[t] if t < len(vocab) else f"<{t}>"
            if t < len(vocab) and _is_special(piece):
                continue
            toks.append(ParakeetToken(int(t), piece.replace("▁", " "), self.frame_seconds(int(f)), self.frame_seconds(1)))
        return ParakeetResult("".join(t.text for t in toks).strip(), toks, raw["truncated"], elapsed)

    def generate_batch(self, audios, language=None, att_context_size=None, beam_size: int = 1) -> list:
        if beam_size != 1:
            raise _bad("beam search is not implemented (greedy only)")
        start = time.perf_counter()
        raws = self.decode_raw(audios, language, att_context_size)
        elapsed = time.perf_counter() - start
        return [self._result(r, elapsed) for r in raws]

    def generate(self, audio, language=None, att_context_size=None, beam_size: int = 1) -> ParakeetResult:
        return self.generate_batch([audio], language, att_context_size, beam_size)[0]

    def generate_stream(self, audios, language=None, att_context_size=None, beam_size: int = 1):
        """Yields (row, result) as rows are done, max_batch rows a device call.  (The reference's cache-aware chunk stream is not built.)"""
        mb = self.config.max_batch
        for at in range(0, len(audios), mb):
            langs = language[at: at + mb] if isinstance(language, (list, tuple)) else language
            for i, r in enumerate(self.generate_batch(audios[at: at + mb], langs, att_context_size, beam_size)):
                yield at + i, r

    def stream_session(self, *args, **kwargs):
        """Not a method of the offline class: the cache-aware session is its own class, NemotronStreamSession (make_stream_session), as
        DeepFilterNetStreamer is; this name keeps refusing."""
        raise _bad("the cache-aware stream session is not implemented (offline decode only)")

    create_stream_session = stream_session

    def make_stream_session(self, language=None, chunk_ms=None, streams: int = 1, att_context_size=None,
                            encoder_dtype: str = "float32") -> "NemotronStreamSession":
        """makeStreamSession.  encoder_dtype is the SESSION's: "float32" (the default) needs an f32 model, "bfloat16" one finalized with
        encoder_dtype="bfloat16" (a session rounds nothing itself); the other pairing is refused."""
        return NemotronStreamSession(self, streams, language, att_context_size, chunk_ms, encoder_dtype=encoder_dtype)

    def transcribe_streaming(self, audio, language=None, chunk_ms: int = 480, on_delta=None, encoder_dtype: str = "float32") -> ParakeetResult:
        """transcribeStreaming: the audio through a session at the model's native chunk, fed chunk_ms at a time as a live caller would;
        on_delta receives every non-empty new fragment; encoder_dtype as make_stream_session's."""
        wave = np.asarray(audio, np.float32)
        wave = wave.mean(axis=-1, dtype=np.float32) if wave.ndim > 1 else wave
        chunk = max(1, self.config.sampling_rate * chunk_ms // 1000)
        # (the default goes without the keyword: callers that put a session factory of their own behind make_stream_session(language) keep working)
        s = self.make_stream_session(language) if encoder_dtype == "float32" else self.make_stream_session(language, encoder_dtype=encoder_dtype)
        start = time.perf_counter()
        for at in list(range(0, len(wave), chunk)) + [None]:
            delta = s.finish() if at is None else s.step(wave[at: at + chunk])
            if delta.text and on_delta is not None:
                on_delta(delta.text)
        out = ParakeetResult(s.text.strip(), list(s.tokens), False, time.perf_counter() - start)
        s.close()
        return out


@dataclass
class Delta:
    """NemotronASRStreamSession.Delta: what one step / finish decoded"""
    text: str = ""
    token_ids: list = field(default_factory=list)


def chunk_context(chunk_ms, default_context):
    """makeStreamSession's rounding on the 80 ms encoder frame: chunk_frames = max(1, round(chunk_ms / 80)), right = chunk_frames - 1, left
    from the default context (80 -> (56, 0), 160 -> (56, 1), 320 -> (56, 3), 560 -> (56, 6), 1120 -> (56, 13)); None: the default context"""
    if chunk_ms is None:
        return tuple(default_context)
    return int(default_context[0]), max(1, int(np.floor(chunk_ms / 80.0 + 0.5))) - 1


def nemo_tokens_to_sentences(tokens) -> list:
    """NemoAlignment.tokensToSentences + sentencesToResult(...).segments: a sentence closes behind a token that holds ! ? or their CJK forms,
    or a . that ends the tokens or is followed by a token holding a space -> [dict(text, start, end)]"""
    out, cur = [], []

    def close():
        by_start = sorted(cur, key=lambda t: t.start)
        out.append(dict(text="".join(t.text for t in cur), start=by_start[0].start, end=by_start[-1].start + by_start[-1].duration))
        cur.clear()

    for i, t in enumerate(tokens):
        cur.append(t)
        if any(c in t.text for c in "!?。？！") or ("." in t.text and (i == len(tokens) - 1 or " " in tokens[i + 1].text)):
            close()
    if cur:
        close()
    return out


@dataclass
class StreamFrames:
    """The frame bookkeeping of one stream: the pure function the device session itself runs per stream and pass (mis_nemotron_stream_plan
    in csrc/nemotron_stream.hip: streamEncodeChunks + frozenMelFrames, with up to max_chunks whole chunks a pass).  Needs no device."""
    chunk: int                                                            # C = right + 1 encoder frames
    max_chunks: int = 1
    consumed: int = 0                                                     # mel frames
    emitted: int = 0                                                      # encoder frames
    cache: int = 0                                                        # mel frames carried in front of the next window

    def advance(self, seen: int, final: bool) -> list:
        """-> the passes [(first absolute encoder frame, count)] that `seen` samples (final: all of the stream) let run"""
        state, n = (C.c_int32 * 3)(self.consumed, self.emitted, self.cache), C.c_int32(0)
        room = 2 + (1 + seen // 160) // (8 * self.chunk)
        passes = (C.c_int32 * (2 * room))()
        check(_lib.lib().mis_nemotron_stream_plan(seen, int(bool(final)), self.chunk, self.max_chunks, state, passes, room, C.byref(n)))
        self.consumed, self.emitted, self.cache = (int(v) for v in state)
        return [(int(passes[2 * i]), int(passes[2 * i + 1])) for i in range(n.value)]


class NemotronStreamSession:
    """NemotronASRStreamSession for 1..64 concurrent streams on one model (csrc/nemotron_stream.hip): step / step_batch feed samples and
    return what they decoded, finish flushes a stream's tail; the transcript equals the offline generate of the whole audio at the same
    context, token for token and frame for frame.  att_context_size / chunk_ms choose the context (chunk_context); left must be a multiple
    of right + 1.  text / tokens / segments / is_finished speak of stream 0, as the reference's one-stream session; sentences(stream), raw(stream)
    of any.  encoder_dtype="bfloat16" (on a model finalized in that mode): the blocks of csrc/nemotron_stream_bf16.h, whose yardstick is the
    offline bf16 engine of the same model."""
    _h = None

    def __init__(self, model: NemotronASR, streams: int = 1, language=None, att_context_size=None, chunk_ms=None, max_pass_frames=None,
                 encoder_dtype: str = "float32"):
        self.model, self.streams, self.encoder_dtype = model, int(streams), encoder_dtype
        if encoder_dtype not in _ENCODER_DTYPES:
            raise _bad(f"encoder_dtype {encoder_dtype!r}: only {sorted(_ENCODER_DTYPES)} are implemented")
        if att_context_size is not None and chunk_ms is not None:
            raise _bad("att_context_size and chunk_ms both choose the context: give one")
        self.context = model._context(att_context_size) if att_context_size is not None else chunk_context(chunk_ms, model.config.default_context)
        left, right = (int(v) for v in self.context)
        mp, h, cap = int(max_pass_frames or 3 * (right + 1)), C.c_void_p(), model.config.max_tokens
        if encoder_dtype == "float32":
            check(_lib.lib().mis_nemotron_stream_create(model._h, self.streams, left, right, mp, C.byref(h)))
        else:
            check(_lib.lib().mis_nemotron_stream_create_dtype(model._h, self.streams, left, right, mp, _ENCODER_DTYPES[encoder_dtype], C.byref(h)))
        self._h, self._plan = h, (right + 1, max(1, mp // (right + 1)))
        self._out = [np.zeros((self.streams, cap), np.int32) for _ in range(2)]      # a feed's tokens and frames
        self._passes = 0
        langs = language if isinstance(language, (list, tuple)) else [language] * self.streams
        self._state = [None] * self.streams
        for b in range(self.streams):
            self.reset(b, langs[b])

    def close(self):
        h, self._h = self._h, None
        if h:
            _lib.lib().mis_nemotron_stream_destroy(h)

    __del__ = close

    def reset(self, stream: int = 0, language=None):
        """stream -1: all of them"""
        check(_lib.lib().mis_nemotron_stream_reset(self._h, stream, self.model.resolve_prompt_index(language)))
        for b in range(self.streams) if stream < 0 else [stream]:
            self._state[b] = dict(ids=[], frames=[], tokens=[], text="", done=False, truncated=False, seen=0, plan=StreamFrames(*self._plan))

    @property
    def launches(self) -> int:
        return int(_lib.lib().mis_nemotron_stream_launches(self._h))

    @property
    def expected_launches_per_pass(self) -> int:
        return 9 + 16 * self.model.config.num_hidden_layers + (2 if self.model.config.prompt_hidden else 0)

    @property
    def expected_launches(self) -> int:
        """of the last feed: passes x (9 + 16 L + 2 p); a feed runs as many passes as the stream that needs the most (StreamFrames)"""
        return self._passes * self.expected_launches_per_pass

    def frames_seen(self, stream: int = 0) -> int:
        return int(_lib.lib().mis_nemotron_stream_frames_seen(self._h, stream))

    def feed_raw(self, chunks, final=None):
        """One device call: chunks[b] the samples of stream b (None / empty: nothing), final[b] ends it -> per stream (token ids, frames)"""
        S, cap = self.streams, self.model.config.max_tokens
        rows = [np.zeros(0, np.float32) if c is None else np.ascontiguousarray(c, np.float32).reshape(-1) for c in chunks]
        if len(rows) != S:
            raise _bad(f"{len(rows)} chunks for {S} streams")
        stride = max(1, max(len(r) for r in rows))
        pcm = np.zeros((S, stride), np.float32)
        for b, r in enumerate(rows):
            pcm[b, :len(r)] = r
        n = np.asarray([len(r) for r in rows], np.int64)
        fin = np.asarray([bool(f) for f in (final or [False] * S)], np.int32)
        tok, frm = self._out
        cnt, flg = (np.zeros(S, np.int32) for _ in range(2))
        self._passes = 0
        for b, st in enumerate(self._state):
            if not st["done"]:
                st["seen"] += int(n[b])
                self._passes = max(self._passes, len(st["plan"].advance(st["seen"], bool(fin[b]))))
        check(_lib.lib().mis_nemotron_stream_feed(self._h, pcm.ctypes.data, n.ctypes.data, fin.ctypes.data, stride, tok.ctypes.data, frm.ctypes.data, cap,
                                                  cnt.ctypes.data, flg.ctypes.data))
        for b in range(S):
            self._state[b]["truncated"] = bool(flg[b])
        return [(tok[b, :cnt[b]].copy(), frm[b, :cnt[b]].copy()) for b in range(S)]

    def _delta(self, b, ids, frames) -> Delta:
        """advance()'s tail: special tokens leave the text, not the decoder state; the delta is the text's new suffix"""
        st, m, vocab, new = self._state[b], self.model, self.model.config.vocabulary, []
        st["ids"] += [int(t) for t in ids]; st["frames"] += [int(f) for f in frames]
        for t, f in zip(ids, frames):
            piece = vocab[t] if t < len(vocab) else f"<{t}>"
            if t < len(vocab) and _is_special(piece):
                continue
            new.append(ParakeetToken(int(t), piece.replace("▁", " "), m.frame_seconds(int(f)), m.frame_seconds(1)))
        st["tokens"] += new
        full = "".join(t.text for t in st["tokens"])
        delta = full[len(st["text"]):] if full.startswith(st["text"]) else full
        st["text"] = full
        return Delta(delta, [t.id for t in new])

    def step_batch(self, chunks, final=None) -> list:
        final = list(final or [False] * self.streams)
        live = [not self._state[b]["done"] for b in range(self.streams)]
        raws = self.feed_raw([c if live[b] else None for b, c in enumerate(chunks)], [f and live[b] for b, f in enumerate(final)])
        out = [self._delta(b, *raws[b]) if live[b] else Delta() for b in range(self.streams)]
        for b, f in enumerate(final):
            self._state[b]["done"] |= bool(f)
        return out

    def step(self, samples, stream: int = 0) -> Delta:
        return self.step_batch([samples if b == stream else None for b in range(self.streams)])[stream]

    def finish(self, stream: int = 0) -> Delta:
        """Flushes the trailing partial chunk; a second finish returns an empty delta."""
        if self._state[stream]["done"]:
            return Delta()
        return self.step_batch([None] * self.streams, [b == stream for b in range(self.streams)])[stream]

    def enable_taps(self, frames: int):
        dims = (C.c_int64 * 3)()
        check(_lib.lib().mis_nemotron_stream_tap(self._h, 0, None, frames, dims, None))

    def tap(self, stage: int) -> list:
        """The frames the last feed brought, per stream [n_b, width]; stages as NemotronASR.tap's.  enable_taps() first."""
        dims, cnt = (C.c_int64 * 3)(), np.zeros(self.streams, np.int32)
        check(_lib.lib().mis_nemotron_stream_tap(self._h, stage, None, 0, dims, None))
        out = np.zeros(tuple(int(d) for d in dims), np.float32)
        check(_lib.lib().mis_nemotron_stream_tap(self._h, stage, out.ctypes.data, out.size, dims, cnt.ctypes.data))
        return [out[b, :cnt[b]].copy() for b in range(self.streams)]

    def timing(self) -> float:
        """Device milliseconds of the last feed, copies included."""
        ms = C.c_float()
        check(_lib.lib().mis_debug_nemotron_stream_timing(self._h, C.byref(ms)))
        return float(ms.value)

    def decode_timing(self) -> float:
        """Device milliseconds of the decode launch in the last pass of the last feed; the first call turns it on and returns -1."""
        ms = C.c_float()
        check(_lib.lib().mis_debug_nemotron_stream_decode_timing(self._h, C.byref(ms)))
        return float(ms.value)

    text = property(lambda self: self._state[0]["text"])
    tokens = property(lambda self: self._state[0]["tokens"])
    is_finished = property(lambda self: self._state[0]["done"])
    segments = property(lambda self: self.sentences(0))

    def sentences(self, stream: int = 0) -> list:
        """NemoAlignedResult.segments of what the stream has decoded: [dict(text, start, end)]"""
        return nemo_tokens_to_sentences(self._state[stream]["tokens"])

    def raw(self, stream: int = 0) -> dict:
        """every token id (specials included) and its absolute encoder frame, as decode_raw's"""
        st = self._state[stream]
        return dict(tokens=np.asarray(st["ids"], np.int32), frames=np.asarray(st["frames"], np.int32), truncated=st["truncated"])
