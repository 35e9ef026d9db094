"""Host mirror of SopranoModel : SpeechGenerationModel (Sources/MLXAudioTTS/Models/Soprano/Soprano.swift:201-690).

Device work (Qwen3-style token LM with hidden-state tap, Soprano sampler flavour, Vocos/ISTFT decoder) is behind
mis_soprano_* in libmi_speech.so.  Host logic mirrored here: prompt splitting, sentence merging, the
"[STOP][TEXT]...[START]" framing and the whitespace-aware tokenisation (Soprano.swift:365-575).  Text
normalisation (cleanTextForSoprano, TextUtils.swift) is injectable (`clean_text`) and defaults to a
whitespace collapse: it is string processing outside the accelerated path."""
from __future__ import annotations

import ctypes as C
import json
import os
import re
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._handle import NativeHandle
from .generation import (AudioEvent, AudioGenerationError, AudioGenerationInfo, GenerateParameters, InfoEvent, TokenEvent, check,
                         decode_audio_event, stream_events)
from .tts import MAX_BATCH, LlamaTTSConfiguration, LlamaTTSModel


@dataclass
class SopranoConfiguration:
    """SopranoConfiguration (SopranoConfig.swift:103-167, Soprano-1.1-80M defaults)."""
    hidden_size: int = 512
    num_hidden_layers: int = 17
    intermediate_size: int = 2304
    num_attention_heads: int = 4
    num_key_value_heads: int = 1
    head_dim: int = 128
    vocab_size: int = 8192
    rms_norm_eps: float = 1e-6
    rope_theta: float = 10000.0
    tie_word_embeddings: bool = False
    sample_rate: int = 32000
    decoder_num_layers: int = 8
    decoder_dim: int = 768
    decoder_intermediate_dim: int = 2304
    hop_length: int = 512
    n_fft: int = 2048
    upscale: int = 4
    input_kernel: int = 1
    dw_kernel: int = 3
    token_size: int = 2048
    stop_token_id: int = 3
    space_token_id: int = 8004           # Soprano.swift:452

    @classmethod
    def from_dict(cls, d: dict) -> "SopranoConfiguration":
        known = {f for f in cls.__dataclass_fields__}
        return cls(**{k: v for k, v in d.items() if k in known})

    @classmethod
    def from_model_config(cls, config_json: dict, repo: str) -> "SopranoConfiguration":
        """config.json as SopranoModel.fromModelDirectory reads it: SopranoConfig.swift's defaults for absent keys, then the
        pre-1.1 decoder (Soprano.swift:935-941) - decoder_dim 512, decoder_intermediate_dim 1536, input_kernel 3 - unless the
        repo name contains "soprano-1.1"."""
        cfg = cls.from_dict(config_json)
        if "soprano-1.1" not in repo.lower():
            cfg.decoder_dim, cfg.decoder_intermediate_dim, cfg.input_kernel = 512, 1536, 3
        return cfg

    def lm_configuration(self) -> LlamaTTSConfiguration:
        return LlamaTTSConfiguration(hidden_size=self.hidden_size, num_hidden_layers=self.num_hidden_layers,
                                     intermediate_size=self.intermediate_size,
                                     num_attention_heads=self.num_attention_heads,
                                     num_key_value_heads=self.num_key_value_heads, head_dim=self.head_dim,
                                     vocab_size=self.vocab_size, rms_norm_eps=self.rms_norm_eps,
                                     rope_theta=self.rope_theta, tie_word_embeddings=self.tie_word_embeddings,
                                     sample_rate=self.sample_rate, qk_norm=True, rope_plain=True)

    def to_c(self) -> "_lib.SopranoConfigC":
        return _lib.SopranoConfigC(self.lm_configuration().to_c(), self.decoder_num_layers, self.decoder_dim,
                                   self.decoder_intermediate_dim, self.hop_length, self.n_fft, self.upscale,
                                   self.input_kernel, self.dw_kernel, self.token_size, self.stop_token_id)


def _sanitize_key(key: str) -> str:
    """SopranoModel.sanitize's key map (Soprano.swift:314-360)."""
    k = key[len("model."):] if key.startswith("model.") else key
    if k.startswith("decoder."):
        return k
    if k.startswith("language_model.lm_head"):
        return k.replace("language_model.", "")
    if k.startswith("language_model."):
        return k.replace("language_model.", "model.")
    if k.startswith("lm_head"):
        return k
    return "model." + k


def soprano_checkpoint_plan(dtypes: dict, quantization: dict | None, tie_word_embeddings: bool) -> list:
    """How SopranoModel.from_model_directory sends a checkpoint's tensors to the engine (SopranoModel.fromModelDirectory,
    Soprano.swift:905-979: sanitize :314-360, then every module with a `.scales` companion quantised with its per-layer entry of
    `quantization` or the global one, :949-963).  dtypes: stored key -> safetensors dtype string; quantization: config.json's
    `quantization` / `quantization_config` entry or None.  Returns, in key order, ("dense", src_key, dst_key, as_f32) and
    ("quantized", w_key, scales_key, biases_key, dst_key, group_size, bits) entries (dst_key: the sanitized .weight key); decoder
    tensors other than packed weights and their scales / biases are cast to float32; lm_head.weight is dropped under tied embeddings.
    `.scales` / `.biases` without a quantization entry or without their companions, and a U32 / I32 weight without `.scales`, raise
    AudioGenerationError."""
    q = quantization or {}
    plan = []
    for k in sorted(dtypes):
        dst = _sanitize_key(k)
        if tie_word_embeddings and dst == "lm_head.weight":
            continue
        suf = next((s for s in (".scales", ".biases") if k.endswith(s)), None)
        if suf is not None:
            base = k[: -len(suf)]
            if not quantization:
                raise AudioGenerationError(3, f"{k}: quantised tensor in a checkpoint whose config.json has no quantization entry")
            if base + ".weight" not in dtypes or base + ".scales" not in dtypes or base + ".biases" not in dtypes:
                raise AudioGenerationError(3, f"{k}: quantised tensor without its .weight / .scales / .biases companions")
            continue                                                     # (sent with its .weight)
        if k.endswith(".weight") and k[: -len(".weight")] + ".scales" in dtypes:
            base = k[: -len(".weight")]
            if base + ".biases" not in dtypes:
                raise AudioGenerationError(3, f"{k}: quantised weight without its .biases companion")
            if not quantization:
                raise AudioGenerationError(3, f"{k}: quantised tensor in a checkpoint whose config.json has no quantization entry")
            layer = q.get(dst[: -len(".weight")])
            src = layer if isinstance(layer, dict) else q
            plan.append(("quantized", k, base + ".scales", base + ".biases", dst, int(src.get("group_size", 64)), int(src.get("bits", 4))))
        elif dtypes[k] in ("U32", "I32"):
            raise AudioGenerationError(3, f"{k}: integer tensor without .scales (a quantised checkpoint needs .scales / .biases)")
        else:
            plan.append(("dense", k, dst, dst.startswith("decoder.")))
    return plan


_SENT_SPLIT = re.compile(r"(?<=[.!?])\s+")
_SPECIAL = re.compile(r"\[(?:STOP|TEXT|START)\]")
_PRETOK = re.compile(r"\s+|\w+|[^\w\s]+")


def split_into_sentences(text: str) -> list[str]:
    """Soprano.swift:414-449"""
    return [s for s in _SENT_SPLIT.split(text) if s] or [text]


def preprocess_text(texts, min_length: int = 30, clean_text=None):
    """preprocessText (Soprano.swift:365-411): [(prompt, text_idx, sentence_idx)]."""
    clean = clean_text or (lambda t: re.sub(r"\s+", " ", t).strip())
    out = []
    for ti, text in enumerate(texts):
        items = [s for s in split_into_sentences(clean(text.strip(" \t")))]
        if min_length > 0 and len(items) > 1:
            merged, i = [], 0
            while i < len(items):
                cur = items[i]
                if len(cur) < min_length:
                    if merged:
                        merged[-1] = (merged[-1] + " " + cur).strip(" \t")
                    elif i + 1 < len(items):
                        items[i + 1] = (cur + " " + items[i + 1]).strip(" \t")
                    else:
                        merged.append(cur)
                else:
                    merged.append(cur)
                i += 1
            items = merged
        out += [(f"[STOP][TEXT]{s}[START]", ti, si) for si, s in enumerate(items)]
    return out


def split_prompt(text: str, split_pattern: str = "\n") -> list[str]:
    """Chunking at the top of generate() (Soprano.swift:594-624): split on the pattern, then chunks over 500
    characters at . ? ! : ; once 100 characters are collected (hard cut at 500)."""
    text = text.replace("\\n", "\n").replace("\\t", "\t")
    chunks = [c.strip(" \t") for c in text.split(split_pattern)]
    out = []
    for chunk in (c for c in chunks if c):
        if len(chunk) <= 500:
            out.append(chunk)
            continue
        cur = ""
        for ch in chunk:
            cur += ch
            if (ch in ".?!:;" and len(cur) >= 100) or len(cur) >= 500:
                out.append(cur.strip(" \t"))
                cur = ""
        if cur:
            out.append(cur.strip(" \t"))
    return [c for c in out if c]


class SopranoModel(NativeHandle):
    _prefix = "mis_soprano"

    def __init__(self, config: SopranoConfiguration, device: int = 0):
        self.configuration = config
        self.device = device
        self.tokenizer = None
        self.clean_text = None
        self._create(config.to_c(), device)
        # borrowed LM handle: taps (lm_forward / reset) for tests and synthetic init
        self.lm = LlamaTTSModel(config.lm_configuration(), None, device,
                                _handle=C.c_void_p(_lib.lib().mis_soprano_lm(self._h)))
        self.lm._borrowed = True

    def close(self):
        if getattr(self, "lm", None) is not None:
            self.lm._h = None                                            # borrowed: it dies with this handle
        super().close()

    @classmethod
    def from_weights(cls, config, weights: dict, device: int = 0) -> "SopranoModel":
        m = cls(config, device)
        for k, v in weights.items():
            m.set_tensor(k, v)
        m.finalize()
        return m

    @classmethod
    def synthetic(cls, config, device: int = 0, seed: int = 4321, decoder_seed: int = 99, quant_bits: int | None = None) -> "SopranoModel":
        """mis-synth-v1 LM weights; quant_bits 8 / 4: every Linear of the LM as a synthetic group-64 quantised matrix (bf16 scales),
        streamed as codes (mis_tts_init_synthetic_quantized)."""
        from .synthetic import soprano_decoder_synthetic_weights
        m = cls(config, device)
        if quant_bits:
            check(_lib.lib().mis_tts_init_synthetic_quantized(m.lm._h, seed, int(quant_bits)))
        else:
            check(_lib.lib().mis_tts_init_synthetic(m.lm._h, seed))
        for k, v in soprano_decoder_synthetic_weights(config, decoder_seed).items():
            m.set_tensor(k, v)
        m.finalize()
        return m

    @classmethod
    def from_model_directory(cls, model_dir: str, repo: str | None = None, device: int = 0) -> "SopranoModel":
        """SopranoModel.fromModelDirectory (Soprano.swift:926-979): config.json (SopranoConfiguration.from_model_config with `repo`,
        default the directory's base name) and every *.safetensors in name order, later files overriding earlier keys
        (loadSopranoWeights); soprano_checkpoint_plan says what goes to set_tensor and what to set_quantized_tensor.  The tokenizer is
        not attached (it cannot be checked offline): set `tokenizer` before generate(text); the stop id is the configuration's."""
        import torch
        from safetensors import safe_open
        with open(os.path.join(model_dir, "config.json")) as f:
            cj = json.load(f)
        repo = repo if repo is not None else os.path.basename(os.path.normpath(model_dir))
        cfg = SopranoConfiguration.from_model_config(cj, repo)
        quant = cj.get("quantization") or cj.get("quantization_config")
        files = sorted(fn for fn in os.listdir(model_dir) if fn.endswith(".safetensors"))
        where = {}                                                          # key -> file (the last one that holds it)
        for fn in files:
            with safe_open(os.path.join(model_dir, fn), framework="pt") as sf:
                for k in sf.keys():
                    where[k] = (fn, sf.get_slice(k).get_dtype())
        plan = soprano_checkpoint_plan({k: v[1] for k, v in where.items()}, quant, cfg.tie_word_embeddings)
        m = cls(cfg, device)
        handles = {fn: safe_open(os.path.join(model_dir, fn), framework="pt") for fn in files}
        try:
            get = lambda k: handles[where[k][0]].get_tensor(k)
            for e in plan:
                if e[0] == "dense":
                    _, src, dst, as_f32 = e
                    v = get(src)
                    m.set_tensor(dst, v.float() if as_f32 else v)
                else:
                    _, kw, ks, kb, dst, gs, bits = e
                    wq = get(kw).contiguous().view(torch.int32).numpy().view(np.uint32)
                    m.set_quantized_tensor(dst, wq, get(ks), get(kb), gs, bits)
        finally:
            handles.clear()
        m.finalize()
        return m

    @classmethod
    def from_pretrained(cls, model_repo: str, device: int = 0) -> "SopranoModel":
        if os.path.isdir(model_repo):
            return cls.from_model_directory(model_repo, device=device)
        raise AudioGenerationError(1, f"model repo {model_repo!r} is not a local directory (no network access)")

    # -- protocol surface ------------------------------------------------------------------------------
    @property
    def sample_rate(self) -> int:
        return self.configuration.sample_rate

    @property
    def default_generation_parameters(self) -> GenerateParameters:
        """Soprano.swift:231-239"""
        return GenerateParameters(max_tokens=1200, temperature=0.7, top_p=0.95, repetition_penalty=1.5,
                                  repetition_context_size=30, sampler_flavor=1)

    def num_samples(self, n_hidden: int) -> int:
        return int(_lib.lib().mis_soprano_num_samples(self._h, n_hidden))

    def decode(self, hidden) -> np.ndarray:
        """SopranoDecoder.callAsFunction: hidden [B, L, hidden_size] (numpy or device torch) -> [B, samples]."""
        try:
            import torch
            if isinstance(hidden, torch.Tensor):
                hidden = hidden.detach().to(torch.float32).cpu().numpy()
        except ImportError:
            pass
        h = np.ascontiguousarray(hidden, dtype=np.float32)
        B, L, Cc = h.shape
        ptr = h.ctypes.data
        if Cc != self.configuration.hidden_size:
            raise AudioGenerationError(3, "hidden width does not match the configuration")
        out = np.zeros((B, self.num_samples(L)), np.float32)
        check(_lib.lib().mis_soprano_decode(self._h, ptr, B, L, out.ctypes.data))
        return out

    def tokenize(self, text: str) -> np.ndarray:
        """Soprano.swift:461-500: special tokens as-is, one space token per whitespace character."""
        if self.tokenizer is None:
            raise AudioGenerationError(1, "Tokenizer not loaded")
        ids, pos = [], 0
        segs = []
        for m in _SPECIAL.finditer(text):
            if m.start() > pos:
                segs.append((text[pos:m.start()], False))
            segs.append((m.group(0), True))
            pos = m.end()
        if pos < len(text):
            segs.append((text[pos:], False))
        for seg, special in segs:
            if special:
                ids += list(self.tokenizer.encode(seg))
                continue
            for chunk in _PRETOK.findall(seg):
                if chunk.isspace():
                    ids += [self.configuration.space_token_id] * len(chunk)
                else:
                    ids += list(self.tokenizer.encode(chunk))
        return np.asarray(ids, np.int32)

    @property
    def lm_path(self) -> int:
        """mis_soprano_lm_path: the program that ran the LM loop of the last call - 0 launch chain (by rule), 1 batch-1 token engine,
        2 launch chain after the engine's workers could not be co-resident."""
        return int(_lib.lib().mis_soprano_lm_path(self._h))

    def generate_batch(self, prompt_rows, generation_parameters: GenerateParameters | None = None,
                       return_tokens: bool = False, replicas=None):
        """One generate per tokenised sentence prompt, batched: list of 1-D float32 arrays.  More rows than the engine's
        per-call maximum run in slices of MAX_BATCH (the reference loops sentence by sentence, Soprano.swift:637-676);
        the RNG is keyed by the global row index, so slicing does not change any row."""
        gp = generation_parameters or self.default_generation_parameters
        per_call = MAX_BATCH * (len(replicas) if replicas else 1)            # the engine's maximum is per replica
        if len(prompt_rows) > per_call:
            from dataclasses import replace
            outs, toks_all = [], []
            for i in range(0, len(prompt_rows), per_call):
                r = self.generate_batch(prompt_rows[i:i + per_call], replace(gp, row_offset=gp.row_offset + i), return_tokens, replicas)
                if return_tokens:
                    outs += r[0]; toks_all += r[1]
                else:
                    outs += r
            return (outs, toks_all) if return_tokens else outs
        flat, lens = LlamaTTSModel._flatten(prompt_rows)
        B = len(lens)
        gpc = gp.to_c()
        gpc.sampler_flavor = 1
        pcm = C.c_void_p(); stride = C.c_int64(); plens = (C.c_int64 * B)()
        toks = C.c_void_p(); tstride = C.c_int64(); ntok = (C.c_int32 * B)()
        if replicas:          # SopranoModel objects with the same weights, one per GPU: rows sharded inside the library
            hs = (C.c_void_p * len(replicas))(*[r._h for r in replicas])
            check(_lib.lib().mis_soprano_group_generate(hs, len(replicas), flat.ctypes.data, lens.ctypes.data, B, C.byref(gpc), C.byref(pcm),
                                                        C.byref(stride), plens, C.byref(toks) if return_tokens else None,
                                                        C.byref(tstride), ntok))
        else:
            check(_lib.lib().mis_soprano_generate(self._h, flat.ctypes.data, lens.ctypes.data, B, C.byref(gpc), C.byref(pcm),
                                                  C.byref(stride), plens, C.byref(toks) if return_tokens else None,
                                                  C.byref(tstride), ntok))
        try:
            arr = np.ctypeslib.as_array(C.cast(pcm, C.POINTER(C.c_float)), shape=(B, max(stride.value, 1)))
            out = [arr[b, : plens[b]].copy() for b in range(B)]
            if return_tokens:
                t = np.ctypeslib.as_array(C.cast(toks, C.POINTER(C.c_int32)), shape=(B, max(tstride.value, 1)))
                tok = [t[b, : ntok[b]].copy() for b in range(B)]
        finally:
            _lib.lib().mis_free(pcm)
            if return_tokens and toks:
                _lib.lib().mis_free(toks)
        return (out, tok) if return_tokens else out

    def generate(self, text: str, voice=None, split_pattern: str = "\n",
                 generation_parameters: GenerateParameters | None = None) -> np.ndarray:
        """generate(text:voice:splitPattern:parameters:) (Soprano.swift:577-690).  The sentence prompts of the text run
        batched, up to MAX_BATCH per engine call (the reference loops over them); parts are concatenated in order."""
        if self.tokenizer is None:
            raise AudioGenerationError(1, "Tokenizer not loaded")
        gp = generation_parameters or self.default_generation_parameters
        if generation_parameters is None:
            gp.max_tokens = 1200
        rows = []
        for chunk in split_prompt(text, split_pattern):
            rows += [self.tokenize(p) for p, _, _ in preprocess_text([chunk], clean_text=self.clean_text)]
        if not rows:
            raise AudioGenerationError(6, "No audio generated")
        parts = self.generate_batch(rows, gp)
        return np.concatenate(parts) if len(parts) > 1 else parts[0]

    def generate_stream_batch(self, prompt_rows, generation_parameters: GenerateParameters | None = None, cancel_flag=None):
        """mis_soprano_generate_stream on tokenised sentence prompts: TokenEvent while the engine generates, then per row
        InfoEvent and one AudioEvent."""
        gp = generation_parameters or GenerateParameters(max_tokens=512, temperature=0.3, top_p=0.95, repetition_penalty=1.5,
                                                         repetition_context_size=30)          # generateStream defaults (:696-702)
        flat, lens = LlamaTTSModel._flatten(prompt_rows)
        B = len(lens)
        if B > MAX_BATCH:
            raise AudioGenerationError(3, f"at most {MAX_BATCH} sentence prompts per streamed call")
        gpc = gp.to_c()
        gpc.sampler_flavor = 1

        def start(cbf, flag_addr):
            return _lib.lib().mis_soprano_generate_stream(self._h, flat.ctypes.data, lens.ctypes.data, B, C.byref(gpc), cbf, None,
                                                          flag_addr)
        yield from stream_events(start, decode_audio_event, cancel_flag)

    def generate_stream(self, text: str, voice=None, generation_parameters: GenerateParameters | None = None):
        """generateStream(text:voice:parameters:) (Soprano.swift:693-800): .token per sampled id (all sentences of the text, in
        sentence order), then ONE .info and ONE .audio = the sentences' audio concatenated (:760-787).  The sentences run
        sequentially like the reference's loop so that the token order is the reference's."""
        if self.tokenizer is None:
            raise AudioGenerationError(1, "Tokenizer not loaded")
        text = text.replace("\\n", "\n").replace("\\t", "\t")
        rows = [self.tokenize(p) for p, _, _ in preprocess_text([text], clean_text=self.clean_text)]
        parts, total, secs = [], 0, 0.0
        for row in rows:
            for ev in self.generate_stream_batch([row], generation_parameters):
                if isinstance(ev, TokenEvent):
                    yield TokenEvent(0, ev.token)
                elif isinstance(ev, InfoEvent):
                    total += ev.info.generation_token_count
                    secs += ev.info.generate_time
                elif isinstance(ev, AudioEvent):
                    parts.append(ev.audio)
        if not parts:
            raise AudioGenerationError(2, "No audio generated")
        yield InfoEvent(0, AudioGenerationInfo(0, total, 0.0, secs, total / secs if secs > 0 else 0.0, 0.0))
        yield AudioEvent(0, np.concatenate(parts) if len(parts) > 1 else parts[0])
