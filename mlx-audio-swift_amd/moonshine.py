"""Moonshine STT, host mirror of `MoonshineModel: STTGenerationModel`
(Sources/MLXAudioSTT/Models/Moonshine/MoonshineModel.swift:353-495, MoonshineConfig.swift:3-125).  The tokenizer, the checkpoint key
mapping and text decoding stay on the host as in the reference; stem, encoder, cached decoder and the greedy loop run in
libmi_speech.so (csrc/moonshine.hip)."""
from __future__ import annotations

import ctypes as C
import json
import os
import time
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._handle import NativeHandle, pack_rows, read_safetensors_dir
from .generation import AudioGenerationError, check
from .stt import STTGenerateParameters, STTOutput

MOONSHINE_SAMPLE_RATE = 16000
MOONSHINE_MIN_SAMPLES = 895          # the shortest row that still gives one encoder frame
MOONSHINE_MAX_SAMPLES = 480000       # the engine's per-row cap (30 s)


@dataclass
class MoonshineConfig:
    """MoonshineConfig.swift:3-98, every field and default."""
    model_type: str = "moonshine"
    vocab_size: int = 32768
    hidden_size: int = 288
    intermediate_size: int = 1152
    encoder_num_hidden_layers: int = 6
    decoder_num_hidden_layers: int = 6
    encoder_num_attention_heads: int = 8
    decoder_num_attention_heads: int = 8
    encoder_num_key_value_heads: int | None = None     # nil = the attention head count (:84-85,110-111)
    decoder_num_key_value_heads: int | None = None
    encoder_hidden_act: str = "gelu"
    decoder_hidden_act: str = "silu"
    max_position_embeddings: int = 512
    attention_bias: bool = False
    attention_dropout: float = 0.0
    partial_rotary_factor: float = 0.9
    rope_theta: float = 10000.0
    bos_token_id: int = 1
    eos_token_id: int = 2
    decoder_start_token_id: int = 1
    tie_word_embeddings: bool = True
    pad_head_dim_to_multiple_of: int | None = None

    def __post_init__(self):
        if self.encoder_num_key_value_heads is None:
            self.encoder_num_key_value_heads = self.encoder_num_attention_heads
        if self.decoder_num_key_value_heads is None:
            self.decoder_num_key_value_heads = self.decoder_num_attention_heads

    @classmethod
    def from_dict(cls, d: dict) -> "MoonshineConfig":
        """init(from:) (:100-124): missing or null keys take the defaults, unknown keys are ignored."""
        return cls(**{k: v for k, v in d.items() if k in cls.__dataclass_fields__ and v is not None})

    def to_c(self) -> "_lib.MoonshineConfigC":
        act = lambda name: 1 if str(name).lower() in ("silu", "swish") else 0          # moonshineActivation, :71-78
        return _lib.MoonshineConfigC(
            self.vocab_size, self.hidden_size, self.intermediate_size, self.encoder_num_hidden_layers, self.decoder_num_hidden_layers,
            self.encoder_num_attention_heads, self.decoder_num_attention_heads, self.encoder_num_key_value_heads,
            self.decoder_num_key_value_heads, act(self.encoder_hidden_act), act(self.decoder_hidden_act), self.max_position_embeddings,
            int(bool(self.attention_bias)), float(self.partial_rotary_factor), float(self.rope_theta), self.bos_token_id,
            self.eos_token_id, self.decoder_start_token_id, int(bool(self.tie_word_embeddings)))


def moonshine_rotary_dim(head_dim: int, partial_rotary_factor: float) -> int:
    """MoonshineAttention.init (:142-144): int(head_dim * factor) in float32, rounded down to even, at least 2."""
    r = int(np.float32(head_dim) * np.float32(partial_rotary_factor))
    r -= r % 2
    return max(2, r)


def moonshine_frames(n_samples: int) -> int:
    """Encoder frames of a row of n samples: three unpadded convs, k 127 / 7 / 3, stride 64 / 3 / 2 (:309-312).  0: too short."""
    t1 = (n_samples - 127) // 64 + 1 if n_samples >= 127 else 0
    t2 = (t1 - 7) // 3 + 1 if t1 >= 7 else 0
    return (t2 - 3) // 2 + 1 if t2 >= 3 else 0


class MoonshineTokenizer:
    """MoonshineTokenizer (:7-69): tokenizer.json's model.vocab and added_tokens; decode skips special and unknown ids, folds <0xNN>
    byte tokens into UTF-8 (an invalid run is dropped), turns U+2581 into a space and trims."""

    def __init__(self, model_dir: str):
        with open(os.path.join(model_dir, "tokenizer.json"), encoding="utf-8") as f:
            obj = json.load(f)
        vocab = (obj.get("model") or {}).get("vocab") if isinstance(obj, dict) else None
        if not isinstance(vocab, dict) or not vocab:
            raise AudioGenerationError(1, "Moonshine tokenizer.json does not contain a BPE vocabulary.")
        self.id_to_token = {int(i): t for t, i in vocab.items()}
        self.special_token_ids = {int(t["id"]) for t in (obj.get("added_tokens") or [])
                                  if isinstance(t, dict) and t.get("special") is True and isinstance(t.get("id"), int)}

    def decode(self, tokens) -> str:
        pieces, run = [], bytearray()

        def flush():
            if run:
                try:
                    pieces.append(bytes(run).decode("utf-8"))
                except UnicodeDecodeError:
                    pass
                run.clear()

        for i in tokens:
            i = int(i)
            tok = self.id_to_token.get(i)
            if i in self.special_token_ids or tok is None:
                continue
            if tok.startswith("<0x") and tok.endswith(">") and len(tok) == 6:
                try:
                    run.append(int(tok[3:5], 16))
                    continue
                except ValueError:
                    pass
            flush()
            pieces.append(tok)
        flush()
        return "".join(pieces).replace("▁", " ").strip()


def moonshine_sanitize(weights: dict, tie_word_embeddings: bool = True) -> dict:
    """MoonshineModel.sanitize (:443-459): "model." stripped from encoder / decoder keys, proj_out.* dropped when tied.  The reference
    also moves conv weights into MLX's [out, k, in]; the engine takes the published [out, in, k] and reorders at finalize, so they pass
    through unchanged."""
    out = {}
    for k, v in weights.items():
        nk = k
        if k.startswith("model.encoder.") or k.startswith("model.decoder."):
            nk = k[len("model."):]
        elif k.startswith("proj_out.") and tie_word_embeddings:
            continue
        out[nk] = v
    return out


class MoonshineModel(NativeHandle):
    """STTGenerationModel conformance: default_generation_parameters, generate, generate_stream."""
    _prefix = "mis_moonshine"

    def __init__(self, config: MoonshineConfig, device: int = 0, tokenizer: MoonshineTokenizer | None = None):
        self.config = config
        self.device = device
        self.tokenizer = tokenizer
        self._create(config.to_c(), device)

    @classmethod
    def from_weights(cls, config, weights: dict, device: int = 0, tokenizer=None) -> "MoonshineModel":
        m = cls(config, device, tokenizer)
        for name, arr in moonshine_sanitize(weights, config.tie_word_embeddings).items():
            m.set_tensor(name, arr)
        m.finalize()
        return m

    @classmethod
    def synthetic(cls, config, device: int = 0, seed: int = 777) -> "MoonshineModel":
        m = cls(config, device)
        check(_lib.lib().mis_moonshine_init_synthetic(m._h, seed))
        m.finalize()
        return m

    @classmethod
    def from_model_directory(cls, model_dir: str, device: int = 0) -> "MoonshineModel":
        """fromModelDirectory (:483-495): config.json, an optional tokenizer.json, every *.safetensors in name order.  The reference
        updates with noUnusedKeys and has no quantisation branch: an MLX-quantised directory (.scales keys) is rejected."""
        with open(os.path.join(model_dir, "config.json")) as f:
            cfg = MoonshineConfig.from_dict(json.load(f))
        try:
            tok = MoonshineTokenizer(model_dir)                   # `try?`: a missing or unusable tokenizer.json is not an error
        except (OSError, ValueError, AudioGenerationError):
            tok = None

        def no_quant(fn, keys):
            quant = [k for k in keys if k.endswith(".scales") or k.endswith(".biases")]
            if quant:
                raise AudioGenerationError(3, f"{fn}: MLX-quantised Moonshine checkpoints are not supported ({quant[0]}): the "
                                              "reference loads Moonshine without a quantisation branch")

        weights = read_safetensors_dir(model_dir, missing_code=(1, f"No safetensors files found in {model_dir}"), on_keys=no_quant)
        return cls.from_weights(cfg, weights, device, tok)

    @classmethod
    def from_pretrained(cls, model_name: str, device: int = 0) -> "MoonshineModel":
        """fromPretrained (:461-481) for a local directory; repository ids would need a download, which this package never does."""
        path = os.path.expanduser(model_name)
        if not os.path.isdir(path):
            raise AudioGenerationError(3, f"Moonshine: {model_name!r} is not a local model directory (downloads are not supported)")
        return cls.from_model_directory(path, device)

    @property
    def default_generation_parameters(self) -> STTGenerateParameters:      # :361-363
        return STTGenerateParameters(max_tokens=200, temperature=0.0)

    @property
    def launches_per_step(self) -> int:
        return int(_lib.lib().mis_moonshine_launches_per_step(self._h))

    # -- batching helpers ---------------------------------------------------------------------------
    @staticmethod
    def _pack(rows, junk: float | None = None):
        pcm, lens = pack_rows([np.asarray(r, np.float32).reshape(-1) for r in rows], junk)
        return pcm, lens, pcm.shape[1]

    def frames(self, lens) -> np.ndarray:
        l = np.ascontiguousarray(lens, dtype=np.int64)
        out = np.zeros(len(l), np.int32)
        check(_lib.lib().mis_moonshine_frames(self._h, l.ctypes.data, len(l), out.ctypes.data))
        return out

    # -- taps for parity tests -----------------------------------------------------------------------
    def encode(self, rows, junk: float | None = None, want_output: bool = True):
        """rows: list of 1-D waveforms (ragged) -> list of [T3_b, hidden] float32.  junk: value written behind every row's samples."""
        pcm, lens, stride = self._pack(rows, junk)
        T3 = [moonshine_frames(int(n)) for n in lens]
        out = np.zeros((len(rows), max(max(T3), 1), self.config.hidden_size), np.float32) if want_output else None
        check(_lib.lib().mis_moonshine_encode(self._h, pcm.ctypes.data, lens.ctypes.data, len(rows), stride,
                                              out.ctypes.data if want_output else None))
        return [out[b, : T3[b]].copy() for b in range(len(rows))] if want_output else None

    def stem_tap(self, rows, stage: int, junk: float | None = None):
        """Stage outputs of the stem (0 conv1 + tanh, 1 GroupNorm, 2 gelu(conv2), 3 gelu(conv3)): list of [T_b, C] float32."""
        pcm, lens, stride = self._pack(rows, junk)
        dims = (C.c_int64 * 2)()
        l = _lib.lib()
        check(l.mis_debug_moonshine_stem_tap(self._h, pcm.ctypes.data, lens.ctypes.data, len(rows), stride, stage, None, 0, dims))
        out = np.zeros((len(rows), dims[0], dims[1]), np.float32)
        check(l.mis_debug_moonshine_stem_tap(self._h, pcm.ctypes.data, lens.ctypes.data, len(rows), stride, stage, out.ctypes.data, out.size, dims))
        res = []
        for b, n in enumerate(lens):
            t1 = (int(n) - 127) // 64 + 1
            t2 = (t1 - 7) // 3 + 1
            res.append(out[b, : (t1, t1, t2, (t2 - 3) // 2 + 1)[stage]].copy())
        return res

    def decoder_reset(self, max_positions: int = 0):
        check(_lib.lib().mis_moonshine_decoder_reset(self._h, int(max_positions)))

    def decoder_forward(self, tokens, want_logits: bool = True):
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        out = np.zeros((t.shape[0], self.config.vocab_size), np.float32) if want_logits else None
        check(_lib.lib().mis_moonshine_decoder_forward(self._h, t.ctypes.data, out.ctypes.data if want_logits else None))
        return out

    # -- generate ------------------------------------------------------------------------------------
    def generate_ids(self, rows, params: STTGenerateParameters | None = None, junk: float | None = None):
        """The greedy loop for a ragged batch of waveforms -> list of generated id lists (EOS excluded)."""
        gp = params or self.default_generation_parameters
        pcm, lens, stride = self._pack(rows, junk)
        B = len(rows)
        sp = _lib.SttParamsC(int(gp.max_tokens), float(gp.temperature), int(gp.seed), int(self.config.eos_token_id), 0, None, 0, None, 0)
        toks = C.c_void_p(); ts = C.c_int64(); nt = (C.c_int32 * B)()
        check(_lib.lib().mis_stt_moonshine_generate(self._h, pcm.ctypes.data, lens.ctypes.data, B, stride, C.byref(sp), C.byref(toks),
                                                    C.byref(ts), nt))
        try:
            arr = np.ctypeslib.as_array(C.cast(toks, C.POINTER(C.c_int32)), shape=(B, max(ts.value, 1)))
            return [arr[b, : nt[b]].tolist() for b in range(B)]
        finally:
            _lib.lib().mis_free(toks)

    def decode(self, tokens) -> str:
        """decode(tokens:) (:434-441): the tokenizer, or ASCII / <id> without one."""
        if self.tokenizer is not None:
            return self.tokenizer.decode(tokens)
        return "".join(chr(int(t)) if int(t) < 128 else f"<{int(t)}>" for t in tokens)

    def _output(self, ids, elapsed: float) -> STTOutput:
        text = self.decode(ids).strip()
        el = max(elapsed, 0.001)
        # generationTokens = generated.count, totalTokens = tokens.count = start token + generated (:406-407)
        return STTOutput(text, [{"text": text, "start": 0.0, "end": 0.0}], None, 0, len(ids), len(ids) + 1, 0.0, len(ids) / el, elapsed,
                         0.0, list(ids))

    def generate(self, audio, generation_parameters: STTGenerateParameters | None = None):
        """generate(audio:generationParameters:) (:374-411).  One waveform (a 2-D array is averaged over its last axis, :376) ->
        STTOutput; a list of waveforms -> a list of STTOutput, transcribed as one ragged batch."""
        t0 = time.time()
        if isinstance(audio, (list, tuple)):
            rows = [self._mono(a) for a in audio]
            ids = self.generate_ids(rows, generation_parameters)
            el = time.time() - t0
            return [self._output(i, el) for i in ids]
        ids = self.generate_ids([self._mono(audio)], generation_parameters)[0]
        return self._output(ids, time.time() - t0)

    @staticmethod
    def _mono(audio) -> np.ndarray:
        a = np.asarray(audio, np.float32)
        return a.mean(axis=-1) if a.ndim > 1 else a

    def generate_stream(self, audio, generation_parameters: STTGenerateParameters | None = None):
        """generateStream (:413-425): ("token", text) when the text is not empty, then ("result", STTOutput)."""
        out = self.generate(audio, generation_parameters)
        if out.text:
            yield ("token", out.text)
        yield ("result", out)
