"""Marvis TTS (CSM) host mirror: MarvisTTSModel (Sources/MLXAudioTTS/Models/Marvis/MarvisTTSModel.swift), CSMModelArgs and the two
Llama flavours (CSMModel.swift:306-402).  Everything that computes runs in libmi_speech.so (csrc/marvis.hip); tokenisers stay outside,
as for every family here: the entry points take text token IDS and Mimi CODES.

Deviations from the reference, stated once:
  * reference audio is encoded with Mimi.encode (whole clip); the reference calls encodeStep on 48 000-sample chunks
    (MarvisTTSModel.swift:531-541), a streaming encoder this engine does not have;
  * the voice prompt WAVs (`prompts/*.wav`) are not loaded: pass reference codes or reference audio;
  * sampling is the engine's mis-sampler-v1 stream (seed, row, frame * K + codebook), not MLX's categorical stream."""
from __future__ import annotations

import ctypes as C
import enum
import json
import os
import re
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._handle import NativeHandle
from .generation import AudioGenerationError, check, decode_audio_event, stream_events

MAX_SEQ_LEN = 2048
MAX_AUDIO_FRAMES = int(60000 / 80.0)                 # 12.5 fps, 80 ms per frame (MarvisTTSModel.swift:402)
DEFAULT_REPO = "Marvis-AI/marvis-tts-250m-v0.2-MLX-8bit"


class QualityLevel(enum.IntEnum):                   # MarvisTTSModel.swift:17-22
    low = 8
    medium = 16
    high = 24
    maximum = 32


_LLAMA3_SCALING = dict(factor=32.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=8192.0, rope_type="llama3")


@dataclass
class CSMLlamaConfiguration:                         # CSMLlamaModel.swift:313-345
    hidden_size: int
    num_hidden_layers: int
    intermediate_size: int
    num_attention_heads: int
    num_key_value_heads: int
    head_dim: int | None = None
    rms_norm_eps: float = 1e-5
    vocab_size: int = 128256
    max_position_embeddings: int | None = 2048
    rope_theta: float = 10000.0
    rope_scaling: dict | None = None

    @property
    def resolved_head_dim(self) -> int:
        return self.head_dim or self.hidden_size // self.num_attention_heads

    def rope_numbers(self):
        """(factor, low_freq_factor, high_freq_factor, original_max_position_embeddings), CSMLlamaModel.swift:46-67"""
        rs = self.rope_scaling or {}

        def num(k, d):
            try:
                return float(rs.get(k, d))
            except (TypeError, ValueError):
                return d
        return num("factor", 32.0), num("low_freq_factor", 1.0), num("high_freq_factor", 4.0), num("original_max_position_embeddings", 8192.0)

    def to_c(self) -> "_lib.LmConfigC":
        f, lo, hi, old = self.rope_numbers()
        return _lib.LmConfigC(hidden_size=self.hidden_size, num_hidden_layers=self.num_hidden_layers, intermediate_size=self.intermediate_size,
                              num_attention_heads=self.num_attention_heads, num_key_value_heads=self.num_key_value_heads,
                              head_dim=self.resolved_head_dim, vocab_size=self.vocab_size, rms_norm_eps=self.rms_norm_eps,
                              rope_theta=self.rope_theta, rope_factor=f, rope_low_freq_factor=lo, rope_high_freq_factor=hi,
                              rope_original_max_pos=old, tie_word_embeddings=0, sample_rate=24000, rope_ops_in_dtype=1)


def llama_flavor(flavor: str) -> CSMLlamaConfiguration:
    """createLlamaConfiguration(flavor:), CSMModel.swift:346-402"""
    if flavor == "llama-1B":
        return CSMLlamaConfiguration(2048, 16, 8192, 32, 8, 64, 1e-5, 128256, 2048, 500000.0, dict(_LLAMA3_SCALING))
    if flavor == "llama-100M":
        return CSMLlamaConfiguration(1024, 4, 8192, 8, 2, 128, 1e-5, 128256, 2048, 500000.0, dict(_LLAMA3_SCALING))
    raise AudioGenerationError(3, f"unknown Llama flavour {flavor!r}")


def _llama_from_dict(d: dict, vocab_key: str) -> CSMLlamaConfiguration:
    return CSMLlamaConfiguration(
        hidden_size=int(d["hidden_size"]), num_hidden_layers=int(d["num_hidden_layers"]), intermediate_size=int(d["intermediate_size"]),
        num_attention_heads=int(d["num_attention_heads"]), num_key_value_heads=int(d["num_key_value_heads"]),
        head_dim=(int(d["head_dim"]) if d.get("head_dim") else None), rms_norm_eps=float(d.get("rms_norm_eps", 1e-5)),
        vocab_size=int(d.get(vocab_key, d.get("vocab_size", 128256))), max_position_embeddings=d.get("max_position_embeddings"),
        rope_theta=float(d.get("rope_theta", 10000.0)), rope_scaling=d.get("rope_scaling"))


@dataclass
class CSMModelArgs:
    """CSMModelArgs (CSMModel.swift:134-304): `depth_decoder_config` present -> the backbone is described by the top-level Llama fields
    and the decoder by that entry (:306-344); otherwise the two flavour names pick llama-1B / llama-100M (:346-402)."""
    text_vocab_size: int
    audio_vocab_size: int
    audio_num_codebooks: int
    backbone: CSMLlamaConfiguration
    decoder: CSMLlamaConfiguration
    backbone_flavor: str | None = None
    decoder_flavor: str | None = None
    quantization: dict | None = None
    raw: dict = field(default_factory=dict, repr=False)

    @classmethod
    def from_json(cls, cj: dict) -> "CSMModelArgs":
        depth = cj.get("depth_decoder_config")
        if depth:
            back = _llama_from_dict(cj, "text_vocab_size")
            dec = _llama_from_dict(depth, "vocab_size")
        else:
            back, dec = llama_flavor(cj["backbone_flavor"]), llama_flavor(cj["decoder_flavor"])
        K = cj.get("audio_num_codebooks", (depth or {}).get("num_codebooks", cj.get("num_codebooks")))
        return cls(text_vocab_size=int(cj["text_vocab_size"]), audio_vocab_size=int(cj["audio_vocab_size"]), audio_num_codebooks=int(K),
                   backbone=back, decoder=dec, backbone_flavor=cj.get("backbone_flavor"), decoder_flavor=cj.get("decoder_flavor"),
                   quantization=cj.get("quantization") or cj.get("quantization_config"), raw=dict(cj))

    def to_c(self) -> "_lib.MarvisConfigC":
        return _lib.MarvisConfigC(self.backbone.to_c(), self.decoder.to_c(), self.text_vocab_size, self.audio_vocab_size, self.audio_num_codebooks)


# ---------------------------------------------------------------------------------------------- RoPE (host restatement, tests / tools)
def csm_rope_tables(head_dim: int, theta: float, factor: float = 32.0, low_freq_factor: float = 1.0, high_freq_factor: float = 4.0,
                    old_context_len: float = 8192.0, n_pos: int = 2048):
    """cos / sin float32 [n_pos, head_dim / 2] of CSMLlama3ScaledRoPE.ropeInit / applyScaling (CSMLlamaModel.swift:69-104), float32
    arithmetic step by step; cos / sin of the float32 angle evaluated in double and rounded (what csrc/marvis.hip does)."""
    f32 = np.float32
    idx = np.arange(0, head_dim, 2, dtype=f32)
    freqs = np.power(np.float64(f32(theta)), (idx / f32(head_dim)).astype(np.float64)).astype(f32)      # correctly rounded float32 power
    f = (f32(1.0) / freqs).astype(f32)
    wl = (f32(2.0 * np.float32(np.pi)) / f).astype(f32)
    old, lo, hi, fac = f32(old_context_len), f32(low_freq_factor), f32(high_freq_factor), f32(factor)
    low, high = old / lo, old / hi
    smooth = ((old / wl - lo) / (hi - lo)).astype(f32)
    smooth = np.minimum(np.maximum(smooth, f32(0.0)), f32(1.0))
    scaled = (f / fac).astype(f32)
    blended = (((f32(1.0) - smooth) * scaled).astype(f32) + (smooth * f).astype(f32)).astype(f32)
    th = np.where(wl < high, f, np.where(wl > low, scaled, blended)).astype(f32)
    ang = (np.arange(n_pos, dtype=f32)[:, None] * th[None, :]).astype(f32)
    return np.cos(ang.astype(np.float64)).astype(f32), np.sin(ang.astype(np.float64)).astype(f32)


def deinterleave_rows(n_rows: int, head_dim: int) -> np.ndarray:
    """Row permutation applied to q_proj / k_proj by the engine: new row h*D + i <- old row h*D + 2i, new row h*D + D/2 + i <- old row
    h*D + 2i + 1.  Interleaved rotation of q equals half rotation of q[perm]."""
    r = np.arange(n_rows)
    h, i = r // head_dim, r % head_dim
    return h * head_dim + np.where(i < head_dim // 2, 2 * i, 2 * (i - head_dim // 2) + 1)


# ---------------------------------------------------------------------------------------------- loading
def marvis_sanitize_key(raw_key: str) -> str:
    """MarvisTTSModel.sanitize's key map (MarvisTTSModel.swift:225-262)."""
    k = raw_key
    if not k.startswith("model."):
        k = "model." + k
    if "attn" in k and "self_attn" not in k:
        k = k.replace("attn", "self_attn").replace("output_proj", "o_proj")
    if "mlp" in k:
        k = k.replace("w1", "gate_proj").replace("w2", "down_proj").replace("w3", "up_proj")
    if "sa_norm" in k or "mlp_norm" in k:
        k = k.replace("sa_norm", "input_layernorm").replace("scale", "weight")
        k = k.replace("mlp_norm", "post_attention_layernorm").replace("scale", "weight")
    if "decoder.norm" in k or "backbone.norm" in k:
        k = k.replace("scale", "weight")
    return k


def marvis_sanitize(weights: dict) -> dict:
    return {marvis_sanitize_key(k): v for k, v in weights.items()}


def marvis_checkpoint_plan(dtypes: dict, quantization: dict | None) -> list:
    """How from_model_directory sends a checkpoint's tensors to the engine (MarvisTTSModel.fromPretrained :193-209).  A quantised
    checkpoint (config.json has `quantization`) keeps its keys and quantises exactly the modules that have a `.scales` key - the two
    Embeddings included, `audio_head` (a raw array) never; an unquantised one goes through marvis_sanitize.  dtypes: stored key ->
    safetensors dtype string.  Returns, in key order, ("dense", src_key, dst_key) and ("quantized", w_key, scales_key, biases_key,
    dst_key, group_size, bits).  Orphan `.scales` / `.biases`, quantised tensors without a quantization entry and integer weights
    without `.scales` raise AudioGenerationError."""
    plan = []
    q = quantization or {}
    for k in sorted(dtypes):
        if "rotary_emb.inv_freq" in k:
            continue
        suf = next((s for s in (".scales", ".biases") if k.endswith(s)), None)
        if suf is not None:
            base = k[: -len(suf)]
            if not quantization:
                raise AudioGenerationError(3, f"{k}: quantised tensor in a checkpoint whose config.json has no quantization entry")
            if any(base + s not in dtypes for s in (".weight", ".scales", ".biases")):
                raise AudioGenerationError(3, f"{k}: quantised tensor without its .weight / .scales / .biases companions")
            continue
        dst = k if quantization else marvis_sanitize_key(k)
        if k.endswith(".weight") and k[: -len(".weight")] + ".scales" in dtypes:
            base = k[: -len(".weight")]
            if base + ".biases" not in dtypes:
                raise AudioGenerationError(3, f"{k}: quantised weight without its .biases companion")
            if k.endswith("audio_head.weight"):
                raise AudioGenerationError(3, "audio_head is a raw array: it is never quantised")
            plan.append(("quantized", k, base + ".scales", base + ".biases", dst, int(q.get("group_size", 64)), int(q.get("bits", 4))))
        elif dtypes[k] in ("U32", "I32"):
            raise AudioGenerationError(3, f"{k}: integer tensor without .scales (a quantised checkpoint needs .scales / .biases)")
        else:
            plan.append(("dense", k, dst))
    return plan


# ---------------------------------------------------------------------------------------------- token frames
def tokenize_text_segment(text_ids, K: int):
    """tokenizeTextSegment (:70-100) on token ids (the ids of "[speaker]" + text): frames int32 [T, K + 1] with the id in the last
    column, mask u8 [T, K + 1] set there only."""
    ids = np.asarray(text_ids, np.int32).reshape(-1)
    frame = np.zeros((len(ids), K + 1), np.int32)
    mask = np.zeros((len(ids), K + 1), np.uint8)
    frame[:, K] = ids
    mask[:, K] = 1
    return frame, mask


def tokenize_audio(codes, K: int, add_eos: bool = True):
    """tokenizeAudio (:102-134) on Mimi codes [K, Tq]: frames [T, K + 1] holding the K codes, mask on those; add_eos appends an all-zero frame."""
    cd = np.asarray(codes, np.int32)
    if cd.ndim != 2 or cd.shape[0] != K:
        raise AudioGenerationError(3, f"reference codes must be [{K}, T], got {cd.shape}")
    if add_eos:
        cd = np.concatenate([cd, np.zeros((K, 1), np.int32)], axis=1)
    T = cd.shape[1]
    frame = np.zeros((T, K + 1), np.int32)
    mask = np.zeros((T, K + 1), np.uint8)
    frame[:, :K] = cd.T
    mask[:, :K] = 1
    return frame, mask


def tokenize_segment(text_ids, codes, K: int, add_eos: bool = True):
    """tokenizeSegment (:136-140): text positions, then audio positions."""
    t, tm = tokenize_text_segment(text_ids, K)
    a, am = tokenize_audio(codes, K, add_eos)
    return np.concatenate([t, a], 0), np.concatenate([tm, am], 0)


def text_pieces(text: str, split_pattern: str | None = r"(\n+)") -> list:
    """textPieces (:488-499): the trimmed text split on the pattern's matches (NSRegularExpression.split: the separators are dropped)."""
    if split_pattern is None:
        return [text]
    try:
        rx = re.compile(split_pattern)
    except re.error:
        return [text]
    full = text.strip()
    out, pos = [], 0
    for m in rx.finditer(full):
        out.append(full[pos:m.start()])
        pos = m.end()
    out.append(full[pos:])
    return out if out else [full]


@dataclass
class MarvisGenerateParameters:
    max_frames: int = MAX_AUDIO_FRAMES
    quality_level: int = QualityLevel.maximum      # Cb = min(K, quality_level)
    temperature: float = 0.9                         # TopPSampler(temperature: 0.9, topP: 0.8), :429
    top_p: float = 0.8
    seed: int = 0
    row_offset: int = 0


class MarvisTTSModel(NativeHandle):
    """MarvisTTSModel : SpeechGenerationModel.  A handle owns the two LMs and the CSM tables; the Mimi codec is BORROWED per call and
    stays the caller's."""

    _prefix = "mis_marvis"

    def __init__(self, args: CSMModelArgs, device: int = 0):
        self.args = args
        self.device = device
        self._create(args.to_c(), device)

    # -- loading -------------------------------------------------------------------------------------
    @classmethod
    def from_weights(cls, args: CSMModelArgs, weights: dict, device: int = 0) -> "MarvisTTSModel":
        """weights: post-sanitize names -> tensors; a (wq, scales, biases, group_size, bits) tuple sends a quantised module."""
        m = cls(args, device)
        for k, v in weights.items():
            if isinstance(v, tuple):
                m.set_quantized_tensor(k, *v)
            else:
                m.set_tensor(k, v)
        m.finalize()
        return m

    @classmethod
    def synthetic(cls, args: CSMModelArgs, device: int = 0, seed: int = 4321, quant_bits: int | None = None) -> "MarvisTTSModel":
        m = cls(args, device)
        if quant_bits:
            check(_lib.lib().mis_marvis_init_synthetic_quantized(m._h, seed, int(quant_bits)))
        else:
            check(_lib.lib().mis_marvis_init_synthetic(m._h, seed))
        m.finalize()
        return m

    @classmethod
    def from_model_directory(cls, model_dir: str, device: int = 0) -> "MarvisTTSModel":
        """config.json + model.safetensors (or every *.safetensors shard, later files overriding earlier keys; marvisLoadWeights
        :267-284) through marvis_checkpoint_plan."""
        import torch
        from safetensors import safe_open
        with open(os.path.join(model_dir, "config.json")) as f:
            args = CSMModelArgs.from_json(json.load(f))
        single = os.path.join(model_dir, "model.safetensors")
        files = ["model.safetensors"] if os.path.exists(single) else sorted(fn for fn in os.listdir(model_dir) if fn.endswith(".safetensors"))
        if not files:
            raise AudioGenerationError(1, f"no .safetensors file in {model_dir!r}")
        where = {}
        for fn in files:
            with safe_open(os.path.join(model_dir, fn), framework="pt") as sf:
                for k in sf.keys():
                    where[k] = (fn, sf.get_slice(k).get_dtype())
        plan = marvis_checkpoint_plan({k: v[1] for k, v in where.items()}, args.quantization)
        m = cls(args, device)
        handles = {fn: safe_open(os.path.join(model_dir, fn), framework="pt") for fn in files}
        try:
            get = lambda k: handles[where[k][0]].get_tensor(k)
            for e in plan:
                if e[0] == "dense":
                    m.set_tensor(e[2], get(e[1]))
                else:
                    _, kw, ks, kb, dst, gs, bits = e
                    wq = get(kw).contiguous().view(torch.int32).numpy().view(np.uint32)
                    m.set_quantized_tensor(dst, wq, get(ks), get(kb), gs, bits)
        finally:
            handles.clear()
        m.finalize()
        return m

    @classmethod
    def from_pretrained(cls, model_repo: str = DEFAULT_REPO, device: int = 0) -> "MarvisTTSModel":
        if os.path.isdir(model_repo):
            return cls.from_model_directory(model_repo, device)
        raise AudioGenerationError(1, f"model repo {model_repo!r} is not a local directory (no network access)")

    # -- protocol surface ----------------------------------------------------------------------------
    @property
    def sample_rate(self) -> int:
        return 24000

    @property
    def num_codebooks(self) -> int:
        return self.args.audio_num_codebooks

    @property
    def default_generation_parameters(self) -> MarvisGenerateParameters:
        return MarvisGenerateParameters()

    @property
    def launches_per_frame(self) -> int:
        return int(_lib.lib().mis_marvis_launches_per_frame(self._h))

    def native_quant_bits(self):
        """(backbone, decoder) x [qkv, o, gate/up, down, head]: bits of the roles streamed as codes (0 = dense)."""
        lib = _lib.lib()
        return [[lib.mis_tts_native_quant_bits(C.c_void_p(h), r) for r in range(5)]
                for h in (lib.mis_marvis_backbone(self._h), lib.mis_marvis_decoder(self._h))]

    def codebooks(self, gp: MarvisGenerateParameters) -> int:
        return min(self.num_codebooks, int(gp.quality_level))

    def _params(self, gp: MarvisGenerateParameters) -> "_lib.MarvisParamsC":
        return _lib.MarvisParamsC(int(gp.max_frames), self.codebooks(gp), float(gp.temperature), float(gp.top_p), int(gp.seed), int(gp.row_offset))

    def _marshal(self, prompts):
        """prompts: list of (frames [T, K + 1], mask [T, K + 1]) -> padded batch arrays."""
        W = self.num_codebooks + 1
        B = len(prompts)
        if B < 1:
            raise AudioGenerationError(3, "no prompts")
        lens = np.asarray([len(p[0]) for p in prompts], np.int32)
        P = max(int(lens.max()), 1)
        tok = np.zeros((B, P, W), np.int32)
        msk = np.zeros((B, P, W), np.uint8)
        for b, (t, m) in enumerate(prompts):
            t = np.asarray(t, np.int32); m = np.asarray(m, np.uint8)
            if t.ndim != 2 or t.shape[1] != W or m.shape != t.shape:
                raise AudioGenerationError(3, f"prompt {b}: frames and mask must be [T, {W}]")
            tok[b, : len(t)] = t
            msk[b, : len(t)] = m
        return tok, msk, lens, P, B

    @staticmethod
    def _caps(row_max_frames, B):
        if row_max_frames is None:
            return None, None
        caps = np.ascontiguousarray(row_max_frames, np.int32)
        if caps.shape != (B,):
            raise AudioGenerationError(3, "row_max_frames must hold one cap per row")
        return caps, caps.ctypes.data

    def generate_codes(self, prompts, generation_parameters: MarvisGenerateParameters | None = None, row_max_frames=None) -> list:
        """Frames only: per row codes int32 [n_frames, Cb]."""
        gp = generation_parameters or self.default_generation_parameters
        tok, msk, lens, P, B = self._marshal(prompts)
        gpc = self._params(gp)
        caps, caps_p = self._caps(row_max_frames, B)
        out = C.c_void_p(); stride = C.c_int64(); nf = (C.c_int32 * B)()
        check(_lib.lib().mis_marvis_generate_codes(self._h, tok.ctypes.data, msk.ctypes.data, lens.ctypes.data, P, B, C.byref(gpc), caps_p,
                                                   C.byref(out), C.byref(stride), nf))
        Cb = self.codebooks(gp)
        try:
            arr = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_int32)), shape=(B, stride.value, Cb))
            return [arr[b, : nf[b]].copy() for b in range(B)]
        finally:
            _lib.lib().mis_free(out)

    def forced_logits(self, prompts, forced, generation_parameters: MarvisGenerateParameters | None = None):
        """Debug entry: the frame loop teacher-forced along forced int32 [B, F, Cb] -> (logits f32 [B, F, Cb, audio_vocab], sampled
        int32 [B, F, Cb], n_frames [B])."""
        gp = generation_parameters or self.default_generation_parameters
        tok, msk, lens, P, B = self._marshal(prompts)
        gpc = self._params(gp)
        Cb = self.codebooks(gp)
        fc = np.ascontiguousarray(forced, np.int32)
        if fc.ndim != 3 or fc.shape[0] != B or fc.shape[2] != Cb:
            raise AudioGenerationError(3, f"forced must be [{B}, F, {Cb}]")
        F = fc.shape[1]
        logits = np.zeros((B, F, Cb, self.args.audio_vocab_size), np.float32)
        sampled = np.zeros((B, F, Cb), np.int32)
        nf = np.zeros(B, np.int32)
        check(_lib.lib().mis_debug_marvis_forced_logits(self._h, tok.ctypes.data, msk.ctypes.data, lens.ctypes.data, P, B, C.byref(gpc),
                                                        fc.ctypes.data, F, logits.ctypes.data, sampled.ctypes.data, nf.ctypes.data))
        return logits, sampled, nf

    def generate_batch(self, prompts, mimi, generation_parameters: MarvisGenerateParameters | None = None, row_max_frames=None,
                       streaming_interval: float | None = None, on_audio=None, return_codes: bool = False):
        """mis_marvis_generate for a batch of prompts: per row pcm float32 [n_frames * 1920] (and the codes).  streaming_interval +
        on_audio(row, chunk): chunks of int(streaming_interval * 12.5) frames are delivered while the loop runs."""
        gp = generation_parameters or self.default_generation_parameters
        tok, msk, lens, P, B = self._marshal(prompts)
        gpc = self._params(gp)
        caps, caps_p = self._caps(row_max_frames, B)
        Cb = self.codebooks(gp)
        pcm = C.c_void_p(); pstride = C.c_int64(); plens = (C.c_int64 * B)()
        codes = C.c_void_p(); cstride = C.c_int64(); nf = (C.c_int32 * B)()
        chunk, cbf = 0, None
        if on_audio is not None:
            chunk = max(1, int((streaming_interval if streaming_interval is not None else 0.5) * 12.5))

            def cb(user, row, kind, payload, n):
                if kind == _lib.EVENT_AUDIO:
                    on_audio(row, decode_audio_event(row, kind, payload, n).audio)
            cbf = _lib.EVENT_CB(cb)
        check(_lib.lib().mis_marvis_generate(self._h, mimi._h, tok.ctypes.data, msk.ctypes.data, lens.ctypes.data, P, B, C.byref(gpc), caps_p,
                                             C.byref(pcm), C.byref(pstride), plens, C.byref(codes), C.byref(cstride), nf, chunk, cbf, None, None))
        try:
            a = np.ctypeslib.as_array(C.cast(pcm, C.POINTER(C.c_float)), shape=(B, max(pstride.value, 1)))
            out = [a[b, : plens[b]].copy() for b in range(B)]
            cd = np.ctypeslib.as_array(C.cast(codes, C.POINTER(C.c_int32)), shape=(B, cstride.value, Cb))
            cds = [cd[b, : nf[b]].copy() for b in range(B)]
        finally:
            _lib.lib().mis_free(pcm)
            _lib.lib().mis_free(codes)
        return (out, cds) if return_codes else out

    def generate_stream_batch(self, prompts, mimi, generation_parameters: MarvisGenerateParameters | None = None, row_max_frames=None,
                              streaming_interval: float = 2.0, cancel_flag=None):
        """AudioGeneration events while the engine generates: TokenEvent (code 0 of each frame), AudioEvent chunks of
        int(streaming_interval * 12.5) frames, InfoEvent per row when the frame loop ends, then the remaining frames."""
        gp = generation_parameters or self.default_generation_parameters
        tok, msk, lens, P, B = self._marshal(prompts)
        gpc = self._params(gp)
        caps, caps_p = self._caps(row_max_frames, B)
        chunk = max(1, int(streaming_interval * 12.5))
        pcm = C.c_void_p(); pstride = C.c_int64(); plens = (C.c_int64 * B)()

        def start(cbf, flag_addr):
            st = _lib.lib().mis_marvis_generate(self._h, mimi._h, tok.ctypes.data, msk.ctypes.data, lens.ctypes.data, P, B, C.byref(gpc), caps_p,
                                                C.byref(pcm), C.byref(pstride), plens, None, None, None, chunk, cbf, None, flag_addr)
            if pcm.value:
                _lib.lib().mis_free(pcm)
            return st
        yield from stream_events(start, decode_audio_event, cancel_flag)

    # -- the reference's generate, on ids and codes --------------------------------------------------
    def _reference_codes(self, ref_codes, ref_audio, mimi):
        K = self.num_codebooks
        if ref_codes is not None:
            return np.asarray(ref_codes, np.int32).reshape(K, -1)
        if ref_audio is None or mimi is None:
            raise AudioGenerationError(3, "`ref_codes`, or `ref_audio` with a Mimi, must be specified")
        return mimi.encode(np.asarray(ref_audio, np.float32).reshape(1, -1), n_q=K)[0]     # (deviation: Mimi.encode, not chunked encodeStep)

    def prompt_for(self, text_ids, ref_codes):
        """The prompt of one text piece (:409-427): ids of "[0]" + refText + " " + text as text positions, then the reference codes as
        audio positions, no EOS frame; shorter than 2048 - 750."""
        tok, msk = tokenize_segment(text_ids, ref_codes, self.num_codebooks, add_eos=False)
        if len(tok) >= MAX_SEQ_LEN - MAX_AUDIO_FRAMES:
            raise AudioGenerationError(3, f"Inputs too long, must be below max_seq_len - max_audio_frames: {MAX_SEQ_LEN - MAX_AUDIO_FRAMES}")
        return tok, msk

    def generate(self, text_ids_per_piece, mimi, ref_codes=None, ref_audio=None, quality_level: int = QualityLevel.maximum,
                 streaming_interval: float = 0.5, generation_parameters: MarvisGenerateParameters | None = None) -> list:
        """generate (:317-338): one PCM array per yielded chunk (int(streaming_interval * 12.5) frames, then the remainder) of every
        text piece in turn.  text_ids_per_piece: the token ids of "[0]" + refText + " " + piece for every piece (text_pieces)."""
        return [e.audio for e in self.generate_stream(text_ids_per_piece, mimi, ref_codes, ref_audio, quality_level, streaming_interval,
                                                      generation_parameters) if hasattr(e, "audio")]

    def generate_stream(self, text_ids_per_piece, mimi, ref_codes=None, ref_audio=None, quality_level: int = QualityLevel.maximum,
                        streaming_interval: float = 2.0, generation_parameters: MarvisGenerateParameters | None = None):
        """generateStream: AudioGeneration events; the LM caches and the Mimi stream are reset per text piece (:412-413)."""
        gp = generation_parameters or MarvisGenerateParameters()
        gp = MarvisGenerateParameters(gp.max_frames, int(quality_level), gp.temperature, gp.top_p, gp.seed, gp.row_offset)
        codes = self._reference_codes(ref_codes, ref_audio, mimi)
        for ids in text_ids_per_piece:
            yield from self.generate_stream_batch([self.prompt_for(ids, codes)], mimi, gp, streaming_interval=streaming_interval)
