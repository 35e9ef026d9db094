"""Canary speech-to-text and translation, host mirror of `CanaryModel` (Sources/MLXAudioSTT/Models/Canary/CanaryModel.swift,
CanaryConfig.swift).  Configuration, checkpoint key handling, the tokenizer and the prompt stay on the host; the log-mel front end,
Parakeet's FastConformer encoder, the cross K/V and the cached greedy decode run in libmi_speech.so (csrc/canary.hip).

Refused, not approximated: temperature > 0, beam search, quantised checkpoints, decoder.hidden_size != enc_output_dim, the encoder
options Parakeet refuses, and rows beyond max_seconds (the reference's chunking above chunkDuration is not built)."""
from __future__ import annotations

import base64
import ctypes as C
import json
import os
import time
from dataclasses import dataclass, field, replace

import numpy as np

from . import _lib
from ._handle import _ENCODER_DTYPES, NativeHandle, pack_rows, read_safetensors_dir
from .generation import AudioGenerationError, check
from .lasr import SentencePieceTokenizer
from .parakeet import parakeet_sanitize, _perm
from .sensevoice import read_sentencepiece_pieces
from .stt import STTOutput

DEFAULT_LANGUAGES = ["bg", "hr", "cs", "da", "nl", "en", "et", "fi", "fr", "de", "el", "hu", "it", "lv", "lt", "mt", "pl", "pt", "ro", "sk",
                     "sl", "es", "sv", "ru", "uk"]


def _bad(msg):
    return AudioGenerationError(3, "Canary: " + msg)


def _pick(d, cls, keys):
    return cls(**{k: d[k] for k in keys if d.get(k) is not None})


@dataclass
class CanaryPreprocessConfig:
    sample_rate: int = 16000
    normalize: str = "per_feature"
    features: int = 128
    n_fft: int = 512
    window_size: float = 0.025
    window_stride: float = 0.01
    window: str = "hann"
    dither: float = 0.0
    pad_to: int = 0
    pad_value: float = 0.0
    preemph: float = 0.97


@dataclass
class CanaryEncoderConfig:
    feat_in: int = 128
    n_layers: int = 32
    d_model: int = 1024
    n_heads: int = 8
    ff_expansion_factor: int = 4
    subsampling_factor: int = 8
    self_attention_model: str = "rel_pos"
    subsampling: str = "dw_striding"
    conv_kernel_size: int = 9
    subsampling_conv_channels: int = 256
    pos_emb_max_len: int = 5000
    causal_downsampling: bool = False
    use_bias: bool = True
    xscaling: bool = True
    subsampling_conv_chunking_factor: int = 1


@dataclass
class CanaryDecoderConfig:
    num_layers: int = 8
    hidden_size: int = 1024
    num_attention_heads: int = 16
    inner_size: int = 4096
    ffn_dropout: float = 0.0
    attn_score_dropout: float = 0.0
    attn_layer_dropout: float = 0.0


@dataclass
class CanaryConfig:
    """CanaryConfig.swift's keys and defaults.  max_batch / max_seconds / max_tokens / max_prompt size the workspace and are not part of a
    checkpoint."""
    model_type: str = "canary"
    preprocessor: CanaryPreprocessConfig = field(default_factory=CanaryPreprocessConfig)
    encoder: CanaryEncoderConfig = field(default_factory=CanaryEncoderConfig)
    decoder: CanaryDecoderConfig = field(default_factory=CanaryDecoderConfig)
    vocab_size: int = 16384
    enc_output_dim: int = 1024
    startofcontext_id: int = 0
    startoftranscript_id: int = 1
    emo_undefined_id: int = 2
    endoftext_id: int = 3
    supported_languages: list = field(default_factory=lambda: list(DEFAULT_LANGUAGES))
    tokenizer_model_base64: str | None = None
    max_batch: int = 8
    max_seconds: int = 30
    max_tokens: int = 200
    max_prompt: int = 16
    encoder_dtype: str = "float32"   # "bfloat16": the encoder's Conformer blocks in bf16 (csrc/parakeet_encoder_bf16.h); not part of a checkpoint
    decoder_dtype: str = "float32"   # "bfloat16": the step's matrices and K/V stores in bf16 (mi_speech.h's contract); not part of a checkpoint

    @classmethod
    def from_dict(cls, d: dict, **workspace) -> "CanaryConfig":
        """init(from:) (CanaryConfig.swift:329-358): missing keys take the defaults; `transf_decoder` wins over `decoder`, either may nest
        its fields under `decoder`."""
        if any(d.get(k) is not None for k in ("quantization", "quantization_config")):
            raise _bad("quantised checkpoints are not implemented")
        dec = d.get("transf_decoder") if isinstance(d.get("transf_decoder"), dict) else d.get("decoder") or {}
        if isinstance(dec.get("decoder"), dict):
            dec = dec["decoder"]
        kw = {k: d[k] for k in ("model_type", "vocab_size", "enc_output_dim", "startofcontext_id", "startoftranscript_id", "emo_undefined_id",
                                "endoftext_id", "supported_languages") if d.get(k) is not None}
        tok = d.get("tokenizer")
        if isinstance(tok, dict) and tok.get("model_base64"):
            kw["tokenizer_model_base64"] = tok["model_base64"]
        return cls(preprocessor=_pick(d.get("preprocessor") or {}, CanaryPreprocessConfig, CanaryPreprocessConfig.__dataclass_fields__),
                   encoder=_pick(d.get("encoder") or {}, CanaryEncoderConfig, CanaryEncoderConfig.__dataclass_fields__),
                   decoder=_pick(dec, CanaryDecoderConfig, CanaryDecoderConfig.__dataclass_fields__), **kw, **workspace)

    def to_c(self) -> "_lib.CanaryConfigC":
        p, e, dc = self.preprocessor, self.encoder, self.decoder
        if e.self_attention_model != "rel_pos" or e.subsampling != "dw_striding" or e.causal_downsampling:
            raise _bad("only rel_pos attention behind a non-causal dw_striding stem is implemented")
        if p.normalize not in ("per_feature", "none", None):
            raise _bad(f"normalize {p.normalize} is not implemented (per_feature)")
        if dc.hidden_size != self.enc_output_dim:
            raise _bad(f"decoder.hidden_size {dc.hidden_size} differs from enc_output_dim {self.enc_output_dim}: the reference builds the embedding, "
                       "norms and head from one and the blocks from the other")
        if e.feat_in != p.features:
            raise _bad(f"encoder.feat_in {e.feat_in} differs from preprocessor.features {p.features}")
        sr = int(p.sample_rate)
        return _lib.CanaryConfigC(e.d_model, e.n_layers, e.n_heads, e.d_model * e.ff_expansion_factor, p.features, e.conv_kernel_size,
                                  e.subsampling_factor, e.subsampling_conv_channels, int(e.use_bias), int(e.xscaling), self.enc_output_dim,
                                  dc.num_layers, dc.hidden_size, dc.num_attention_heads, dc.inner_size, self.vocab_size, sr,
                                  int(np.float32(p.window_stride) * np.float32(sr)), p.n_fft, int(np.float32(p.window_size) * np.float32(sr)),
                                  int(p.normalize == "per_feature"), self.max_batch, self.max_seconds, self.max_tokens, self.max_prompt,
                                  float(p.preemph or 0.0))


# ---------------------------------------------------------------------------------------------------- checkpoint keys
_DROPPED = ("attn_dropout", "layer_dropout", "num_batches_tracked")
_NEMO_SUB = {"first_sub_layer.": ("self_attn.", {"query_net.": "q_proj.", "key_net.": "k_proj.", "value_net.": "v_proj.", "out_projection.": "out_proj."}),
             "second_sub_layer.": ("cross_attn.", {"query_net.": "q_proj.", "key_net.": "k_proj.", "value_net.": "v_proj.", "out_projection.": "out_proj."}),
             "third_sub_layer.": ("", {"dense_in.": "ff1.", "dense_out.": "ff2."})}
_MLX_SUB = {"first_sub_layer.": ("self_attn.", {"linear_q.": "q_proj.", "linear_k.": "k_proj.", "linear_v.": "v_proj.", "linear_out.": "out_proj."}),
            "second_sub_layer.": ("cross_attn.", {"linear_q.": "q_proj.", "linear_k.": "k_proj.", "linear_v.": "v_proj.", "linear_out.": "out_proj."}),
            "third_sub_layer.": ("", {"linear1.": "ff1.", "linear2.": "ff2."})}
_NORMS = {"layer_norm_1.": "self_attn_norm.", "layer_norm_2.": "cross_attn_norm.", "layer_norm_3.": "ff_norm."}


def _decoder_layer(rest: str, table: dict):
    layer, _, sub = rest.partition(".")
    if not sub:
        return None
    for pre, (head, names) in table.items():
        if sub.startswith(pre):
            sub = sub[len(pre):]
            for a, b in names.items():
                sub = sub.replace(a, b)
            return f"decoder.blocks.{layer}.{head}{sub}"
    for a, b in _NORMS.items():
        if sub.startswith(a):
            return f"decoder.blocks.{layer}.{b}{sub[len(a):]}"
    return f"decoder.blocks.{layer}.{sub}"


def _pre_encode_list(key: str):
    """remapCanaryPreEncodeConvListKey / shouldSkip...: encoder.conformer.pre_encode.conv.N -> conv0 (N = 0), depthwise_layers.b / pointwise_layers.b
    (N = 2 + 3 b, 3 + 3 b); N = 1 and the activations N = 4 + 3 b are dropped.  (key or None, dropped)"""
    p = key.split(".")
    if len(p) < 6 or p[:4] != ["encoder", "conformer", "pre_encode", "conv"] or not p[4].isdigit():
        return key, False
    n, suffix = int(p[4]), ".".join(p[5:])
    if n == 0:
        return "encoder.conformer.pre_encode.conv0." + suffix, False
    if n < 2 or (n - 2) % 3 == 2:
        return None, True
    kind = "depthwise_layers" if (n - 2) % 3 == 0 else "pointwise_layers"
    return f"encoder.conformer.pre_encode.{kind}.{(n - 2) // 3}.{suffix}", False


def canary_reference_keys(weights: dict) -> dict:
    """CanaryModel.sanitize: any of the three checkpoint layouts -> the reference module's names (encoder.conformer.*, encoder.projection.*,
    decoder.*).  Already `decoder.blocks.*`: returned as is; MLX-native `transf_decoder.layers.*` / `head.classifier`; NeMo
    `transf_decoder._decoder.layers.*` / `log_softmax.mlp.layer0`, whose conv weights are transposed to channels last."""
    if any(k.startswith("decoder.blocks.") for k in weights):
        return dict(weights)
    mlx_native = "head.classifier.weight" in weights or any(k.startswith("transf_decoder.layers.") for k in weights)
    out = {}
    for k, v in weights.items():
        if k.endswith((".scales", ".biases")):
            raise _bad("quantised checkpoints are not implemented")
        enc = k.startswith("encoder.") and not k.startswith("encoder_decoder")
        if mlx_native:
            heads = {"transf_decoder.token_embedding.": "decoder.embedding.", "transf_decoder.embedding_layer_norm.": "decoder.embedding_layer_norm.",
                     "transf_decoder.final_layer_norm.": "decoder.final_norm.", "head.classifier.": "decoder.output_proj."}
            if enc:
                nk = "encoder.conformer." + k[len("encoder."):]
            elif k.startswith("transf_decoder.layers."):
                nk = _decoder_layer(k[len("transf_decoder.layers."):], _MLX_SUB)
            else:
                nk = next((b + k[len(a):] for a, b in heads.items() if k.startswith(a)), None)
        else:
            if any(t in k for t in _DROPPED) or k == "log_softmax.mlp.log_softmax" or k.startswith("encoder_decoder_proj.") \
                    or k.startswith("transf_decoder._embedding.position_embedding."):
                continue
            heads = {"transf_decoder._embedding.token_embedding.": "decoder.embedding.", "transf_decoder._embedding.layer_norm.": "decoder.embedding_layer_norm.",
                     "transf_decoder._decoder.final_layer_norm.": "decoder.final_norm.", "log_softmax.mlp.layer0.": "decoder.output_proj."}
            if enc:
                nk = "encoder.conformer." + k[len("encoder."):]
            elif k.startswith("transf_decoder._decoder.layers."):
                nk = _decoder_layer(k[len("transf_decoder._decoder.layers."):], _NEMO_SUB)
            else:
                nk = next((b + k[len(a):] for a, b in heads.items() if k.startswith(a)), k)
        if nk is None:
            continue
        listed = nk
        nk, dropped = _pre_encode_list(nk)
        if dropped:
            continue
        if not mlx_native and "conv" in listed and nk.endswith(".weight") and v.ndim >= 3:     # (judged on the listed name: conv.N)
            v = _perm(v, (0, 2, 1)) if v.ndim == 3 else _perm(v, (0, 2, 3, 1))
        out[nk.replace(".pos_bias_u", ".posBiasU").replace(".pos_bias_v", ".posBiasV")] = v
    return out


def canary_sanitize(weights: dict) -> dict:
    """Any checkpoint layout -> the engine's names (mi_speech.h): the reference's names (canary_reference_keys) with encoder.conformer.* put
    through parakeet_sanitize (encoder.subsampling.layers_N, *_proj, bias_u / bias_v, conv.norm)."""
    ref = canary_reference_keys(weights)
    enc = {"encoder." + k[len("encoder.conformer."):]: v for k, v in ref.items() if k.startswith("encoder.conformer.")}
    out = parakeet_sanitize(enc)
    out.update({k: v for k, v in ref.items() if not k.startswith("encoder.conformer.")})
    return out


def canary_expected_keys(config: CanaryConfig) -> set:
    e, keys = config.encoder, set()

    def lin(p, bias=True):
        keys.add(p + ".weight")
        if bias:
            keys.add(p + ".bias")

    for n in ("layers_0", "layers_2", "layers_3", "layers_5", "layers_6", "linear"):
        lin("encoder.subsampling." + n)
    for i in range(e.n_layers):
        q = f"encoder.layers.{i}."
        for n in ("norm_feed_forward1", "norm_self_att", "norm_conv", "norm_feed_forward2", "norm_out"):
            lin(q + n)
        for n in ("feed_forward1.linear1", "feed_forward1.linear2", "feed_forward2.linear1", "feed_forward2.linear2", "conv.pointwise_conv1",
                  "conv.depthwise_conv", "conv.pointwise_conv2", "self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj"):
            lin(q + n, e.use_bias)
        lin(q + "self_attn.relative_k_proj", False)
        keys.update(q + "self_attn." + n for n in ("bias_u", "bias_v"))
        keys.update(q + "conv.norm." + n for n in ("weight", "bias", "running_mean", "running_var"))
    if e.d_model != config.enc_output_dim:
        lin("encoder.projection")
    keys.add("decoder.embedding.weight")
    for n in ("embedding_layer_norm", "final_norm", "output_proj"):
        lin("decoder." + n)
    for i in range(config.decoder.num_layers):
        q = f"decoder.blocks.{i}."
        for n in ("self_attn_norm", "cross_attn_norm", "ff_norm", "ff1", "ff2"):
            lin(q + n)
        for at in ("self_attn", "cross_attn"):
            for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
                lin(f"{q}{at}.{n}")
    return keys


# ---------------------------------------------------------------------------------------------------- tokenizer
def _load_token_maps(path: str):
    """loadTokenMaps (CanaryModel.swift:132-163): `token id` lines; a line that starts with a space names a token that starts with one; a
    line with the id alone names the space."""
    t2i, i2t = {}, {}
    if not os.path.exists(path):
        return t2i, i2t
    with open(path, encoding="utf-8") as f:
        for line in f.read().splitlines():
            fields = line.split()
            if len(fields) == 2 and fields[1].lstrip("-").isdigit():
                tok, i = (" " + fields[0] if line.startswith(" ") else fields[0]), int(fields[1])
            elif len(fields) == 1 and fields[0].lstrip("-").isdigit():
                tok, i = " ", int(fields[0])
            else:
                continue
            t2i[tok] = i
            i2t[i] = tok
    return t2i, i2t


class CanaryTokenizer:
    """CanaryTokenizer (CanaryModel.swift:8-164): the tokens.txt maps, a SentencePiece piece list where the directory has one."""

    def __init__(self, token_to_id=None, id_to_token=None, sentencepiece: SentencePieceTokenizer | None = None):
        self.token_to_id, self.id_to_token, self.sp = dict(token_to_id or {}), dict(id_to_token or {}), sentencepiece
        self._sp_ids = {p: i for i, p in enumerate(sentencepiece.pieces)} if sentencepiece is not None else {}

    @classmethod
    def from_model_directory(cls, model_dir: str, config: CanaryConfig):
        t2i, i2t = _load_token_maps(os.path.join(model_dir, "tokens.txt"))
        sp, spm, tj = None, os.path.join(model_dir, "tokenizer.model"), os.path.join(model_dir, "tokenizer.json")
        if os.path.exists(spm):
            with open(spm, "rb") as f:
                sp = SentencePieceTokenizer([p[0] for p in read_sentencepiece_pieces(f.read())])
        elif os.path.exists(tj):
            sp = SentencePieceTokenizer.from_tokenizer_json(tj)
        elif config.tokenizer_model_base64:
            sp = SentencePieceTokenizer([p[0] for p in read_sentencepiece_pieces(base64.b64decode(config.tokenizer_model_base64))])
        if sp is None and not t2i:
            return None
        tok = cls(t2i, i2t, sp)
        if sp is not None:
            special = ["<|startofcontext|>", "<|startoftranscript|>", "<|emo:undefined|>", "<|endoftext|>", "<|pnc|>", "<|nopnc|>", "<|noitn|>",
                       "<|notimestamp|>", "<|nodiarize|>"] + [f"<|{l}|>" for l in config.supported_languages]
            for t in special:
                if t not in tok.token_to_id and t in tok._sp_ids:
                    tok.token_to_id[t] = tok._sp_ids[t]
                    tok.id_to_token[tok._sp_ids[t]] = t
        return tok

    def _find(self, token: str):
        return self.token_to_id.get(token, self._sp_ids.get(token))

    def build_prompt_tokens(self, config: CanaryConfig, source_language: str, target_language: str, pnc: bool = True) -> list:
        """buildPromptTokens (:63-80): the three leading ids fall back to the config's; the rest are appended only if present."""
        out = []
        for t, fb in (("<|startofcontext|>", config.startofcontext_id), ("<|startoftranscript|>", config.startoftranscript_id),
                      ("<|emo:undefined|>", config.emo_undefined_id)):
            i = self._find(t)
            out.append(fb if i is None else i)
        for t in (f"<|{source_language}|>", f"<|{target_language}|>", "<|pnc|>" if pnc else "<|nopnc|>", "<|noitn|>", "<|notimestamp|>", "<|nodiarize|>"):
            i = self._find(t)
            if i is not None:
                out.append(i)
        return out

    def eos_token_id(self, config: CanaryConfig) -> int:
        i = self._find("<|endoftext|>")
        return config.endoftext_id if i is None else i

    def decode(self, ids) -> str:
        if self.sp is not None:
            return self.sp.decode([int(i) for i in ids])
        pieces = [self.id_to_token[int(i)] for i in ids if int(i) in self.id_to_token]
        return "".join(p for p in pieces if not (p.startswith("<|") and p.endswith("|>"))).replace("▁", " ").strip()


def default_prompt_tokens(config: CanaryConfig) -> list:
    return [config.startofcontext_id, config.startoftranscript_id, config.emo_undefined_id]


# ---------------------------------------------------------------------------------------------------- the model
class CanaryModel(NativeHandle):
    """generate / generateStream of the reference class, and a ragged generate_batch: 1..max_batch rows a device call."""
    _prefix = "mis_canary"

    def __init__(self, config: CanaryConfig, tokenizer: CanaryTokenizer | None = None, device: int = 0):
        self.config, self.tokenizer, self.device = config, tokenizer, device
        self._create(config.to_c(), device)
        if config.encoder_dtype != "float32":
            self.set_encoder_dtype(config.encoder_dtype)
        if config.decoder_dtype != "float32":
            self.set_decoder_dtype(config.decoder_dtype)

    sanitize = staticmethod(canary_sanitize)

    def set_decoder_dtype(self, name: str):
        """"float32" (the default) or "bfloat16", before finalize; independent of the encoder's dtype."""
        if name not in _ENCODER_DTYPES:
            raise _bad(f"decoder_dtype {name!r}: only {sorted(_ENCODER_DTYPES)} are implemented")
        check(_lib.lib().mis_canary_set_decoder_dtype(self._h, _ENCODER_DTYPES[name]))
        self.config = replace(self.config, decoder_dtype=name)

    @staticmethod
    def _with_dtypes(config, encoder_dtype, decoder_dtype):
        kw = {k: v for k, v in (("encoder_dtype", encoder_dtype), ("decoder_dtype", decoder_dtype)) if v}
        return replace(config, **kw) if kw else config

    @classmethod
    def from_weights(cls, config: CanaryConfig, weights: dict, tokenizer=None, device: int = 0, encoder_dtype: str | None = None,
                     decoder_dtype: str | None = None) -> "CanaryModel":
        """weights: the engine's names (what canary_sanitize returns); encoder_dtype / decoder_dtype override the config's."""
        m = cls(cls._with_dtypes(config, encoder_dtype, decoder_dtype), tokenizer, device)
        for name, arr in weights.items():
            m.set_tensor(name, arr)
        m.finalize()
        return m

    @classmethod
    def synthetic(cls, config: CanaryConfig, device: int = 0, seed: int = 777, encoder_dtype: str | None = None,
                  decoder_dtype: str | None = None) -> "CanaryModel":
        m = cls(cls._with_dtypes(config, encoder_dtype, decoder_dtype), None, device)
        check(_lib.lib().mis_canary_init_synthetic(m._h, seed))
        m.finalize()
        return m

    @classmethod
    def from_model_directory(cls, model_dir: str, device: int = 0, **workspace) -> "CanaryModel":
        """fromModelDirectory (:510-533): config.json, the tokenizer files, every *.safetensors; keys the model does not have are rejected.
        workspace: max_batch / max_seconds / max_tokens / max_prompt / encoder_dtype / decoder_dtype."""
        with open(os.path.join(model_dir, "config.json")) as f:
            config = CanaryConfig.from_dict(json.load(f), **workspace)

        def on_keys(fn, keys):
            if any(k.endswith((".scales", ".biases")) for k in keys):
                raise _bad(f"{fn} is a quantised checkpoint: not implemented")

        weights = canary_sanitize(read_safetensors_dir(model_dir, missing_code=(2, f"No safetensors files found in {model_dir}"), on_keys=on_keys))
        unknown = sorted(set(weights) - canary_expected_keys(config))
        if unknown:
            raise _bad(f"checkpoint: unused keys {unknown[:4]}")
        return cls.from_weights(config, weights, CanaryTokenizer.from_model_directory(model_dir, config), device)

    @classmethod
    def from_pretrained(cls, path: str, device: int = 0, **workspace) -> "CanaryModel":
        """Local directories only: nothing is downloaded."""
        p = os.path.expanduser(path)
        if not os.path.isdir(p):
            raise _bad(f"{path} is not a local model directory")
        return cls.from_model_directory(p, device, **workspace)

    # -- sizes ---------------------------------------------------------------------------------------
    @property
    def launches(self) -> int:
        return int(_lib.lib().mis_canary_launches(self._h))

    def expected_launches(self, steps: int = 0) -> dict:
        c = self.config
        enc = 7 + 15 * c.encoder.n_layers + int(c.encoder.d_model != c.enc_output_dim)
        cross = c.decoder.num_layers * (2 if c.decoder_dtype == "bfloat16" else 1)      # bf16: the f32 projection + the rounding into the store
        return dict(encode=enc, generate=enc + cross + 1 + steps * (11 * c.decoder.num_layers + 2))

    def frames(self, lens):
        n = np.ascontiguousarray(lens, dtype=np.int64)
        F, T = np.zeros(len(n), np.int32), np.zeros(len(n), np.int32)
        check(_lib.lib().mis_canary_frames(self._h, n.ctypes.data, len(n), F.ctypes.data, T.ctypes.data))
        return F, T

    def _pack(self, audios, junk=None):
        rows = [np.asarray(w, np.float32) for w in audios]
        rows = [r.mean(axis=-1, dtype=np.float32) if r.ndim > 1 else r for r in rows]
        if not rows:
            raise _bad("generate_batch requires at least one audio input")
        cap = self.config.max_seconds * self.config.preprocessor.sample_rate
        for i, r in enumerate(rows):
            if len(r) > cap:
                raise _bad(f"row {i}: {len(r)} samples exceed max_seconds {self.config.max_seconds} (long-audio chunking is not built)")
        return pack_rows(rows, junk)

    @staticmethod
    def _pack_prompts(prompts):
        plen = np.asarray([len(p) for p in prompts], np.int32)
        if plen.min() < 1:
            raise _bad("an empty prompt")
        ids = np.zeros((len(prompts), int(plen.max())), np.int32)
        for i, p in enumerate(prompts):
            ids[i, : len(p)] = p
        return ids, plen

    # -- device calls --------------------------------------------------------------------------------
    def encode(self, audios, junk=None):
        """(encoder output behind the projection [B, Tmax, enc_output_dim], T [B]); zero rows behind a row's own T."""
        pcm, lens = self._pack(audios, junk)
        _, T = self.frames(lens)
        out = np.zeros((len(lens), int(T.max()), self.config.enc_output_dim), np.float32)
        check(_lib.lib().mis_canary_encode(self._h, pcm.ctypes.data, lens.ctypes.data, len(lens), pcm.shape[1], out.ctypes.data))
        return out, T

    def decode_raw(self, audios, prompts, eos: int, max_tokens: int | None = None, junk=None) -> list:
        """One device call -> per row dict(tokens int32 array, truncated); self.last_steps holds the decode steps enqueued."""
        pcm, lens = self._pack(audios, junk)
        ids, plen = self._pack_prompts(prompts)
        if len(plen) != len(lens):
            raise _bad("one prompt a row")
        B, cap = len(lens), int(max_tokens or self.config.max_tokens)
        tok = np.zeros((B, cap), np.int32)
        cnt, flg = np.zeros(B, np.int32), np.zeros(B, np.int32)
        steps = C.c_int32(0)
        check(_lib.lib().mis_canary_generate(self._h, pcm.ctypes.data, lens.ctypes.data, B, pcm.shape[1], ids.ctypes.data, plen.ctypes.data, ids.shape[1],
                                             int(eos), cap, tok.ctypes.data, cnt.ctypes.data, flg.ctypes.data, C.byref(steps)))
        self.last_steps = int(steps.value)
        return [dict(tokens=tok[b, :cnt[b]].copy(), truncated=bool(flg[b])) for b in range(B)]

    def forward(self, prompts):
        """(logits [B, vocab] behind each row's last prompt token, hidden [B, h] in front of final_norm there) against the cross K/V of the
        last encode / generate."""
        ids, plen = self._pack_prompts(prompts)
        logits = np.zeros((len(plen), self.config.vocab_size), np.float32)
        hidden = np.zeros((len(plen), self.config.enc_output_dim), np.float32)
        check(_lib.lib().mis_canary_forward(self._h, ids.ctypes.data, plen.ctypes.data, ids.shape[1], logits.ctypes.data, hidden.ctypes.data))
        return logits, hidden

    def __call__(self, audios, prompts):
        """decoder(tokens, encoderOutput) at the last position of each row's prompt."""
        self.encode(audios)
        return self.forward(prompts)[0]

    def tap(self, stage: int) -> np.ndarray:
        """Tensors of the last encode / generate: 0 the stem, 1..L_enc the Conformer blocks, L_enc + 1 the projected output, then each
        decoder layer's cross K | V."""
        dims = (C.c_int64 * 3)()
        check(_lib.lib().mis_canary_tap(self._h, stage, None, 0, dims))
        out = np.zeros(tuple(int(d) for d in dims), np.float32)
        check(_lib.lib().mis_canary_tap(self._h, stage, out.ctypes.data, out.size, dims))
        return out

    def enable_timing(self):
        check(_lib.lib().mis_debug_canary_timing(self._h, None))

    def timing(self):
        """Device milliseconds of the last generate: (front end, encoder, cross K/V, decode steps); enable_timing() first."""
        ms = (C.c_float * 4)()
        check(_lib.lib().mis_debug_canary_timing(self._h, ms))
        return tuple(float(v) for v in ms)

    # -- results -------------------------------------------------------------------------------------
    def prompt_tokens(self, language: str = "en", target_language: str | None = None) -> list:
        if self.tokenizer is None:
            return default_prompt_tokens(self.config)
        return self.tokenizer.build_prompt_tokens(self.config, language, target_language or language)

    def decode_text(self, tokens) -> str:
        if self.tokenizer is not None:
            return self.tokenizer.decode(tokens)
        return "".join(f"<{int(t)}>" for t in tokens)

    def generate_batch(self, audios, language: str = "en", target_language: str | None = None, max_tokens: int | None = None,
                       temperature: float = 0.0, beam_size: int = 1) -> list:
        if temperature > 0:
            raise _bad("temperature > 0 is not implemented (greedy only)")
        if beam_size != 1:
            raise _bad("beam search is not implemented (greedy only)")
        prompt = self.prompt_tokens(language, target_language)
        eos = self.tokenizer.eos_token_id(self.config) if self.tokenizer is not None else self.config.endoftext_id
        start = time.perf_counter()
        raws = self.decode_raw(audios, [prompt] * len(audios), eos, max_tokens)
        secs = max(time.perf_counter() - start, 0.001)
        outs = []
        for r in raws:
            text, n = self.decode_text(r["tokens"]).strip(), len(r["tokens"])
            outs.append(STTOutput(text, [dict(text=text, start=0.0, end=0.0)], language, len(prompt), n, len(prompt) + n, len(prompt) / secs, n / secs,
                                  secs, 0.0, token_ids=[list(int(t) for t in r["tokens"])]))
        return outs

    def generate(self, audio, **kw) -> STTOutput:
        return self.generate_batch([audio], **kw)[0]

    def generate_stream(self, audio, **kw):
        """generateStream (:434-446): the text as one token event if it is not empty, then the result."""
        out = self.generate(audio, **kw)
        if out.text:
            yield "token", out.text
        yield "result", out
