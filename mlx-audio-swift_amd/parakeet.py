"""Parakeet TDT speech-to-text, host mirror of `ParakeetModel` (Sources/MLXAudioSTT/Models/Parakeet/ParakeetModel.swift, ParakeetConfig.swift,
ParakeetNemoAliases.swift, ParakeetTokenizer.swift; Sources/MLXAudioSTT/Models/Nemo/NemoAlignment.swift for the token times).
Configuration, checkpoint key handling, the piece list and the token times stay on the host; the log-mel front end, the FastConformer
encoder, the joint's enc projection and the whole greedy TDT loop run in libmi_speech.so (csrc/parakeet.hip).

Refused, not approximated: the CTC, RNNT and TDT-CTC variants, beam search, rows beyond max_seconds (the reference's chunk-and-merge of
long audio is not built) and quantised checkpoints."""
from __future__ import annotations

import ctypes as C
import json
import os
import time
from dataclasses import dataclass, field, replace

import numpy as np

from . import _lib
from ._handle import NativeHandle, pack_rows, read_safetensors_dir
from .generation import AudioGenerationError, check
from .sensevoice import read_sentencepiece_pieces

_TDT_TARGET = "nemo.collections.asr.models.rnnt_bpe_models.EncDecRNNTBPEModel"
_OTHER_TARGETS = {"nemo.collections.asr.models.hybrid_rnnt_ctc_bpe_models.EncDecHybridRNNTCTCBPEModel": "TDT-CTC",
                  "nemo.collections.asr.models.ctc_bpe_models.EncDecCTCModelBPE": "CTC"}


def _bad(msg):
    return AudioGenerationError(3, "Parakeet: " + msg)


@dataclass
class ParakeetConfig:
    """The fields of ParakeetRawConfig the engine reads, flattened.  max_batch / max_seconds / max_tokens size the workspace and are not
    part of a checkpoint."""
    num_mel_bins: int = 128
    hidden_size: int = 1024
    num_hidden_layers: int = 24
    num_attention_heads: int = 8
    intermediate_size: int = 4096
    conv_kernel_size: int = 9
    subsampling_factor: int = 8
    subsampling_conv_channels: int = 256
    attention_bias: bool = True
    scale_input: bool = False
    pred_hidden: int = 640
    pred_rnn_layers: int = 2
    joint_hidden: int = 640
    vocab_size: int = 1024
    durations: list = field(default_factory=lambda: [0, 1, 2, 3, 4])
    max_symbols: int = 10
    vocabulary: list = field(default_factory=list)
    sampling_rate: int = 16000
    hop_length: int = 160
    n_fft: int = 512
    win_length: int = 400
    normalize: str = "per_feature"
    preemphasis: float = 0.97
    max_batch: int = 8
    max_seconds: int = 30
    max_tokens: int = 1024
    encoder_dtype: str = "float32"   # "bfloat16": the Conformer blocks in bf16 (csrc/parakeet_encoder_bf16.h); not part of a checkpoint

    @classmethod
    def from_dict(cls, d: dict, **workspace) -> "ParakeetConfig":
        """ParakeetVariantResolver.resolve + ParakeetConfigParser.parseTDT (ParakeetConfig.swift:304-352)."""
        target = d.get("target") or ""
        has_tdt = (d.get("model_defaults") or {}).get("tdt_durations") is not None
        if target in _OTHER_TARGETS:
            raise _bad(f"the {_OTHER_TARGETS[target]} variant is not implemented (TDT only)")
        if target != _TDT_TARGET:
            raise _bad(f"Unsupported Parakeet model target: {target}")
        if not has_tdt:
            raise _bad("the RNNT variant is not implemented (TDT only)")
        if d.get("quantization") is not None:
            raise _bad("quantised checkpoints are not implemented")
        for k in ("preprocessor", "encoder", "decoder", "joint", "decoding"):
            if not isinstance(d.get(k), dict):
                raise _bad(f"Missing required Parakeet config field: {k}")
        p, e, dec, j, dc = d["preprocessor"], d["encoder"], d["decoder"], d["joint"], d["decoding"]
        if e.get("self_attention_model") != "rel_pos" or e.get("subsampling") != "dw_striding" or e.get("causal_downsampling"):
            raise _bad("only rel_pos attention behind a non-causal dw_striding stem is implemented")
        if (dc.get("strategy") or "greedy") not in ("greedy", "greedy_batch"):
            raise _bad(f"decoding strategy {dc.get('strategy')} is not implemented (greedy only)")
        pn, jn = dec["prednet"], j["jointnet"]
        if pn.get("rnn_hidden_size") not in (None, pn["pred_hidden"]):
            raise _bad("rnn_hidden_size different from pred_hidden is not implemented")
        if jn.get("activation", "relu").lower() != "relu":
            raise _bad(f"joint activation {jn.get('activation')} is not implemented (relu only)")
        durations = list(dc["durations"])
        if j.get("num_extra_outputs", 0) != len(durations):
            raise _bad("num_extra_outputs differs from the number of durations")
        sr = int(p["sample_rate"])
        return cls(num_mel_bins=int(p["features"]), hidden_size=e["d_model"], num_hidden_layers=e["n_layers"], num_attention_heads=e["n_heads"],
                   intermediate_size=e["d_model"] * e["ff_expansion_factor"], conv_kernel_size=e["conv_kernel_size"],
                   subsampling_factor=e["subsampling_factor"], subsampling_conv_channels=e["subsampling_conv_channels"],
                   attention_bias=bool(e.get("use_bias", True)), scale_input=bool(e.get("xscaling", False)), pred_hidden=pn["pred_hidden"],
                   pred_rnn_layers=pn["pred_rnn_layers"], joint_hidden=jn["joint_hidden"], vocab_size=dec["vocab_size"], durations=durations,
                   max_symbols=int((dc.get("greedy") or {}).get("max_symbols") or 0), vocabulary=list(j.get("vocabulary") or []),
                   sampling_rate=sr, hop_length=int(np.float32(p["window_stride"]) * np.float32(sr)), n_fft=int(p["n_fft"]),
                   win_length=int(np.float32(p["window_size"]) * np.float32(sr)), normalize=p.get("normalize", "per_feature"),
                   preemphasis=float(p.get("preemph", 0.97) or 0.0), **workspace)

    def to_c(self) -> "_lib.ParakeetConfigC":
        if self.normalize not in ("per_feature", "none", None):
            raise _bad(f"normalize {self.normalize} is not implemented (per_feature)")
        if len(self.durations) > 8:
            raise _bad("more than 8 durations")
        dur = (C.c_int32 * 8)(*self.durations)
        return _lib.ParakeetConfigC(self.hidden_size, self.num_hidden_layers, self.num_attention_heads, self.intermediate_size, self.num_mel_bins,
                                    self.conv_kernel_size, self.subsampling_factor, self.subsampling_conv_channels, int(self.attention_bias),
                                    int(self.scale_input), self.pred_hidden, self.pred_rnn_layers, self.joint_hidden, self.vocab_size,
                                    len(self.durations), self.max_symbols, dur, self.sampling_rate, self.hop_length, self.n_fft, self.win_length,
                                    int(self.normalize == "per_feature"), self.max_batch, self.max_seconds, self.max_tokens, self.preemphasis)


_ATTN = {"linear_q": "q_proj", "linear_k": "k_proj", "linear_v": "v_proj", "linear_out": "o_proj", "linear_pos": "relative_k_proj",
         "pos_bias_u": "bias_u", "pos_bias_v": "bias_v", "posBiasU": "bias_u", "posBiasV": "bias_v"}


def _perm(v, order):
    return v.transpose(*order) if isinstance(v, np.ndarray) else v.permute(*order)


def parakeet_sanitize(weights: dict) -> dict:
    """NeMo / MLX checkpoint names -> the engine's (mi_speech.h), conv layouts told by shape: pre_encode.conv.N (or the reference's conv0 /
    depthwise_layers / pointwise_layers) -> subsampling.layers_N, pre_encode.out -> subsampling.linear, linear_{q,k,v,out,pos} and
    pos_bias_{u,v} -> the *_proj / bias_* names, conv.batch_norm -> conv.norm, joint_net.2 -> joint_net, MLX's lstm.N.{Wx,Wh,bias} ->
    torch's weight_ih / weight_hh / bias_ih (+ a zero bias_hh); Conv2d (O, I, H, W) -> (O, H, W, I), Conv1d (O, I, K) -> (O, K, I);
    num_batches_tracked and the preprocessor's buffers are skipped."""
    out = {}
    for k, v in weights.items():
        if "num_batches_tracked" in k or k.startswith("preprocessor."):
            continue
        if k.endswith((".scales", ".biases")):
            raise _bad("quantised checkpoints are not implemented")
        parts = k.split(".")
        if parts[:2] == ["encoder", "pre_encode"]:
            if parts[2] == "conv" and parts[3].isdigit():
                parts = ["encoder", "subsampling", "layers_" + parts[3]] + parts[4:]
            elif parts[2] == "conv0":
                parts = ["encoder", "subsampling", "layers_0"] + parts[3:]
            elif parts[2] in ("depthwise_layers", "pointwise_layers"):
                n = 3 * int(parts[3]) + (2 if parts[2] == "depthwise_layers" else 3)
                parts = ["encoder", "subsampling", f"layers_{n}"] + parts[4:]
            elif parts[2] == "out":
                parts = ["encoder", "subsampling", "linear"] + parts[3:]
            if v.ndim == 4 and ((v.shape[1] == 1 and v.shape[-1] != 1) or (tuple(v.shape[2:]) == (1, 1) and v.shape[1] != 1)):
                v = _perm(v, (0, 2, 3, 1))
        elif parts[0] == "encoder" and "self_attn" in parts:
            parts = [_ATTN.get(p, p) for p in parts]
        elif parts[0] == "encoder" and "conv" in parts:
            parts = ["norm" if p == "batch_norm" else p for p in parts]
            if v.ndim == 3 and ((parts[-2].startswith("pointwise") and v.shape[2] == 1 and v.shape[1] != 1)
                                or (parts[-2] == "depthwise_conv" and v.shape[1] == 1 and v.shape[2] != 1)):
                v = _perm(v, (0, 2, 1))
        elif parts[:2] == ["joint", "joint_net"] and parts[2] == "2":
            parts = parts[:2] + parts[3:]
        elif "lstm" in parts and parts[-1] in ("Wx", "Wh", "bias") and parts[-2].isdigit():
            n, kind = parts[-2], parts[-1]
            head = ".".join(parts[:-2])
            out[f"{head}.{ {'Wx': 'weight_ih', 'Wh': 'weight_hh', 'bias': 'bias_ih'}[kind] }_l{n}"] = v
            if kind == "bias":
                out[f"{head}.bias_hh_l{n}"] = v * 0
            continue
        out[".".join(parts)] = v
    return out


def parakeet_expected_keys(config: ParakeetConfig) -> set:
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
        for n in ("norm_feed_forward1", "norm_self_att", "norm_conv", "norm_feed_forward2", "norm_out"):
            lin(q + n)
        for n in ("feed_forward1.linear1", "feed_forward1.linear2", "feed_forward2.linear1", "feed_forward2.linear2", "conv.pointwise_conv1",
                  "conv.depthwise_conv", "conv.pointwise_conv2", "self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj"):
            lin(q + n, ab)
        lin(q + "self_attn.relative_k_proj", False)
        keys.update(q + "self_attn." + n for n in ("bias_u", "bias_v"))
        keys.update(q + "conv.norm." + n for n in ("weight", "bias", "running_mean", "running_var"))
    keys.add("decoder.prediction.embed.weight")
    for l in range(config.pred_rnn_layers):
        keys.update(f"decoder.prediction.dec_rnn.lstm.{n}_l{l}" for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
    for n in ("enc", "pred", "joint_net"):
        lin("joint." + n)
    return keys


@dataclass
class ParakeetToken:
    id: int
    text: str
    start: float
    duration: float


@dataclass
class ParakeetResult:
    text: str
    tokens: list
    truncated: bool = False          # the row stopped at max_tokens emissions
    total_time: float = 0.0


def _is_special(piece: str) -> bool:
    """ParakeetTokenizer.isSpecialToken"""
    return (piece.startswith("<|") and piece.endswith("|>")) or piece in ("<unk>", "<pad>")


class ParakeetModel(NativeHandle):
    """generate / generateBatch / generateStream of the reference class for the TDT variant; 1..max_batch ragged rows a device call."""
    _prefix = "mis_parakeet"

    def __init__(self, config: ParakeetConfig, device: int = 0):
        self.config, self.device = config, device
        self._create(config.to_c(), device)
        if config.encoder_dtype != "float32":
            self.set_encoder_dtype(config.encoder_dtype)

    sanitize = staticmethod(parakeet_sanitize)

    @classmethod
    def from_weights(cls, config: ParakeetConfig, weights: dict, device: int = 0, encoder_dtype: str | None = None) -> "ParakeetModel":
        """weights: the engine's names (what parakeet_sanitize returns); encoder_dtype overrides the config's."""
        m = cls(replace(config, encoder_dtype=encoder_dtype) if encoder_dtype else config, device)
        for name, arr in weights.items():
            m.set_tensor(name, arr)
        m.finalize()
        return m

    @classmethod
    def synthetic(cls, config: ParakeetConfig, device: int = 0, seed: int = 777, encoder_dtype: str | None = None) -> "ParakeetModel":
        m = cls(replace(config, encoder_dtype=encoder_dtype) if encoder_dtype else config, device)
        check(_lib.lib().mis_parakeet_init_synthetic(m._h, seed))
        m.finalize()
        return m

    @classmethod
    def from_model_directory(cls, model_dir: str, device: int = 0, **workspace) -> "ParakeetModel":
        """fromDirectory (:946-1052): config.json, every *.safetensors; the vocabulary of config.json, else the first *.model's pieces.
        workspace: max_batch / max_seconds / max_tokens / encoder_dtype."""
        with open(os.path.join(model_dir, "config.json")) as f:
            text = f.read()
        for tok in ("-Infinity", "Infinity", "NaN"):                     # normalizedConfigData (:934-944)
            text = text.replace(tok, "null")
        config = ParakeetConfig.from_dict(json.loads(text), **workspace)
        if not config.vocabulary:
            models = sorted(fn for fn in os.listdir(model_dir) if fn.endswith(".model"))
            if not models:
                raise _bad(f"no vocabulary in config.json and no SentencePiece model in {model_dir}")
            with open(os.path.join(model_dir, models[0]), "rb") as f:
                config.vocabulary = [p[0] for p in read_sentencepiece_pieces(f.read())]

        def on_keys(fn, keys):
            if any(k.endswith((".scales", ".biases")) for k in keys):
                raise _bad(f"{fn} is a quantised checkpoint: not implemented")

        weights = parakeet_sanitize(read_safetensors_dir(model_dir, missing_code=(2, f"No safetensors files found in {model_dir}"), on_keys=on_keys))
        unknown = sorted(set(weights) - parakeet_expected_keys(config))
        if unknown:
            raise _bad(f"checkpoint: unused keys {unknown[:4]}")
        return cls.from_weights(config, weights, device)

    @classmethod
    def from_pretrained(cls, path: str, device: int = 0, **workspace) -> "ParakeetModel":
        """Local directories only: nothing is downloaded."""
        if not os.path.isdir(path):
            raise _bad(f"{path} is not a local model directory")
        return cls.from_model_directory(path, device, **workspace)

    # -- sizes ---------------------------------------------------------------------------------------
    @property
    def launches(self) -> int:
        return int(_lib.lib().mis_parakeet_launches(self._h))

    @property
    def expected_launches(self) -> dict:
        L = self.config.num_hidden_layers
        return dict(generate=9 + 15 * L, encode=7 + 15 * L)

    def frames(self, lens):
        n = np.ascontiguousarray(lens, dtype=np.int64)
        F, T = np.zeros(len(n), np.int32), np.zeros(len(n), np.int32)
        check(_lib.lib().mis_parakeet_frames(self._h, n.ctypes.data, len(n), F.ctypes.data, T.ctypes.data))
        return F, T

    def frame_seconds(self, frames) -> float:
        """frameTimeSeconds (:811-813)"""
        c = self.config
        return float(frames * c.subsampling_factor * c.hop_length) / float(c.sampling_rate)

    def _pack(self, audios, junk=None):
        rows = [np.asarray(w, np.float32) for w in audios]
        rows = [r.mean(axis=-1, dtype=np.float32) if r.ndim > 1 else r for r in rows]
        if not rows:
            raise _bad("generateBatch requires at least one audio input")
        cap = self.config.max_seconds * self.config.sampling_rate
        for i, r in enumerate(rows):
            if len(r) > cap:
                raise _bad(f"row {i}: {len(r)} samples exceed max_seconds {self.config.max_seconds} (long-audio chunking is not built)")
        return pack_rows(rows, junk)

    # -- device calls --------------------------------------------------------------------------------
    def encode(self, audios, junk=None):
        """(encoder output [B, Tmax, hidden], T [B]); zero rows behind a row's own T."""
        pcm, lens = self._pack(audios, junk)
        _, T = self.frames(lens)
        out = np.zeros((len(lens), int(T.max()), self.config.hidden_size), np.float32)
        check(_lib.lib().mis_parakeet_encode(self._h, pcm.ctypes.data, lens.ctypes.data, len(lens), pcm.shape[1], out.ctypes.data))
        return out, T

    def decode_raw(self, audios, junk=None) -> list:
        """One device call -> per row dict(tokens, frames, durations (int32 arrays), truncated, steps)."""
        pcm, lens = self._pack(audios, junk)
        B, cap = len(lens), self.config.max_tokens
        tok, frm, dur = (np.zeros((B, cap), np.int32) for _ in range(3))
        cnt, flg, stp = (np.zeros(B, np.int32) for _ in range(3))
        check(_lib.lib().mis_parakeet_generate(self._h, pcm.ctypes.data, lens.ctypes.data, B, pcm.shape[1], tok.ctypes.data, frm.ctypes.data,
                                               dur.ctypes.data, cnt.ctypes.data, flg.ctypes.data, stp.ctypes.data))
        return [dict(tokens=tok[b, :cnt[b]].copy(), frames=frm[b, :cnt[b]].copy(), durations=dur[b, :cnt[b]].copy(), truncated=bool(flg[b]),
                     steps=int(stp[b])) for b in range(B)]

    def __call__(self, audios, junk=None) -> list:
        return self.decode_raw(audios, junk)

    def tap(self, stage: int) -> np.ndarray:
        """Tensors of the last encode / generate: 0 the stem, 1..L the Conformer blocks, L + 1 joint.enc of the last block."""
        dims = (C.c_int64 * 3)()
        check(_lib.lib().mis_parakeet_tap(self._h, stage, None, 0, dims))
        out = np.zeros(tuple(int(d) for d in dims), np.float32)
        check(_lib.lib().mis_parakeet_tap(self._h, stage, out.ctypes.data, out.size, dims))
        return out

    def enable_timing(self):
        check(_lib.lib().mis_debug_parakeet_timing(self._h, None))

    def timing(self):
        """Device milliseconds of the last generate: (front end, encoder + joint.enc, decode); enable_timing() first."""
        ms = (C.c_float * 3)()
        check(_lib.lib().mis_debug_parakeet_timing(self._h, ms))
        return tuple(float(v) for v in ms)

    # -- results -------------------------------------------------------------------------------------
    def _result(self, raw, elapsed) -> ParakeetResult:
        vocab, toks = self.config.vocabulary, []
        for t, f, d in zip(raw["tokens"], raw["frames"], raw["durations"]):
            piece = vocab[t] if t < len(vocab) else f"<{t}>"
            if t < len(vocab) and _is_special(piece):
                continue
            toks.append(ParakeetToken(int(t), piece.replace("▁", " "), self.frame_seconds(int(f)), self.frame_seconds(int(d))))
        return ParakeetResult("".join(t.text for t in toks).strip(), toks, raw["truncated"], elapsed)

    def generate_batch(self, audios, beam_size: int = 1) -> list:
        if beam_size != 1:
            raise _bad("beam search is not implemented (greedy only)")
        start = time.perf_counter()
        raws = self.decode_raw(audios)
        elapsed = time.perf_counter() - start
        return [self._result(r, elapsed) for r in raws]

    def generate(self, audio, beam_size: int = 1) -> ParakeetResult:
        return self.generate_batch([audio], beam_size)[0]

    def generate_stream(self, audios, beam_size: int = 1):
        """Yields (row, ParakeetResult) as rows are done, max_batch rows a device call."""
        mb = self.config.max_batch
        for at in range(0, len(audios), mb):
            for i, r in enumerate(self.generate_batch(audios[at: at + mb], beam_size)):
                yield at + i, r
