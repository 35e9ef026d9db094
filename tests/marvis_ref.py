"""Torch-CPU restatement of Marvis / CSM for the parity tests, written from the Swift (Sources/MLXAudioTTS/Models/Marvis/):
  * CSMLlama3ScaledRoPE.ropeInit / applyScaling      CSMLlamaModel.swift:69-104   (rope_init_literal, scalar float32 steps)
  * the interleaved rotation as array ops            CSMLlamaModel.swift:141-170  (CSMLlamaRef.rope; cos / sin cast to the activation dtype)
  * CSMLlamaModel (no embedding, returns norm(h))    CSMLlamaModel.swift:279-304  (oracle/llama.py's block with that rotation)
  * CSMModel.generateFrame / _embedTokens            CSMModel.swift:467-557       (CSMRef.run: forced=, want_logits=)
  * the loop's end rule and next position            MarvisTTSModel.swift:433-460
bf16 rounding points are those of oracle/llama.py (round="bf16") or none (round=None: pure float32).  The frame input is the masked sum
accumulated in float32 in codebook order and rounded once - the engine's stated choice (MLX's bf16 reduction order is unknown).
Sampling is oracle/sampler.py (mis-sampler-v1) with step = frame * K + codebook.  Test infrastructure only."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from oracle import llama as ollama
from oracle import sampler as osampler
from oracle import synth

F = np.float32


def rope_init_literal(dims: int, base: float, factor=32.0, low_freq_factor=1.0, high_freq_factor=4.0, old_context_len=8192.0, max_seq_len=2048):
    """ropeInit + applyScaling one scalar float32 operation at a time -> (cos, sin) float32 [max_seq_len, dims / 2]."""
    d2 = dims // 2
    theta = np.zeros(d2, F)
    two_pi = F(2.0 * F(np.pi))
    low = F(F(old_context_len) / F(low_freq_factor))
    high = F(F(old_context_len) / F(high_freq_factor))
    for j in range(d2):
        expo = F(F(2 * j) / F(dims))
        freq = F(math.pow(float(F(base)), float(expo)))                          # float32 power, correctly rounded (evaluated in double)
        inv = F(F(1.0) / freq)
        wl = F(two_pi / inv)
        smooth = F(F(F(F(old_context_len) / wl) - F(low_freq_factor)) / F(F(high_freq_factor) - F(low_freq_factor)))
        smooth = min(max(smooth, F(0.0)), F(1.0))
        scaled = F(inv / F(factor))
        blended = F(F(F(F(1.0) - smooth) * scaled) + F(smooth * inv))
        theta[j] = inv if wl < high else (scaled if wl > low else blended)
    ang = (np.arange(max_seq_len, dtype=F)[:, None] * theta[None, :]).astype(F)
    return np.cos(ang.astype(np.float64)).astype(F), np.sin(ang.astype(np.float64)).astype(F)


def rope_numbers(cfg: ollama.LlamaConfig):
    rs = cfg.rope_scaling or {}
    return (float(rs.get("factor", 32.0)), float(rs.get("low_freq_factor", 1.0)), float(rs.get("high_freq_factor", 4.0)),
            float(rs.get("original_max_position_embeddings", 8192.0)))


class CSMLlamaRef(ollama.LlamaOracle):
    """CSMLlamaModel: the Llama block of oracle/llama.py with CSM's rotation - pairs (2i, 2i + 1), CSM's tables, every array op rounded."""

    def __init__(self, cfg: ollama.LlamaConfig, weights: dict, round: str | None = "bf16", max_seq_len: int = 2048):
        super().__init__(cfg, weights, round=round)
        c, s = rope_init_literal(cfg.resolved_head_dim, cfg.rope_theta, *rope_numbers(cfg), max_seq_len=max_seq_len)
        self.cos, self.sin = torch.from_numpy(c), torch.from_numpy(s)

    def rope(self, x, positions):
        c, s = self.r(self.cos[positions]), self.r(self.sin[positions])           # _cosF32.asType(dtype)
        xe, xo = x[..., 0::2], x[..., 1::2]
        ye = self.r(self.r(xe * c) - self.r(xo * s))
        yo = self.r(self.r(xo * c) + self.r(xe * s))
        return torch.stack([ye, yo], dim=-1).reshape(x.shape)


@dataclass
class CSMConfig:
    backbone: ollama.LlamaConfig
    decoder: ollama.LlamaConfig
    text_vocab_size: int
    audio_vocab_size: int
    audio_num_codebooks: int


def _lm(d, L, ff, H, Hkv, D, vocab):
    return ollama.LlamaConfig(hidden_size=d, num_hidden_layers=L, intermediate_size=ff, num_attention_heads=H, num_key_value_heads=Hkv,
                              head_dim=D, vocab_size=vocab, rope_theta=500000.0, tie_word_embeddings=True, max_position_embeddings=2048)


# tiny configs within the LM engine's width rules (multiples of 64, head_dim 64 / 128); the audio vocabulary is no multiple of 16
TINY = CSMConfig(_lm(256, 2, 512, 4, 2, 64, 300), _lm(128, 2, 256, 1, 1, 128, 83), 300, 83, 12)
LLAMA_1B = _lm(2048, 16, 8192, 32, 8, 64, 128256)
LLAMA_100M = _lm(1024, 4, 8192, 8, 2, 128, 128256)


def make_weights(cfg: CSMConfig, seed: int = 4321) -> dict:
    """Post-sanitize key names, bf16 tensors (mis-synth-v1)."""
    W = {}
    for name, lc, sd in (("backbone", cfg.backbone, seed), ("decoder", cfg.decoder, seed + 1)):
        for k, v in ollama.make_synthetic_weights(lc, seed=sd).items():
            if k in ("model.embed_tokens.weight", "lm_head.weight"):
                continue
            W["model." + name + "." + k[len("model."):]] = v
    d, dd, K, Va = cfg.backbone.hidden_size, cfg.decoder.hidden_size, cfg.audio_num_codebooks, cfg.audio_vocab_size

    def mat(key, shape, amp):
        return torch.from_numpy(synth.synth_tensor(seed * 100000 + 70000 + key, shape, amp)).to(torch.bfloat16)
    W["model.text_embeddings.weight"] = mat(1, (cfg.text_vocab_size, d), 0.5 * math.sqrt(3.0))
    W["model.audio_embeddings.weight"] = mat(2, (K * Va, d), 0.5 * math.sqrt(3.0) / math.sqrt(K))
    W["model.projection.weight"] = mat(3, (dd, d), math.sqrt(3.0 / d))
    W["model.codebook0_head.weight"] = mat(4, (Va, d), math.sqrt(3.0 / d) * 2.0)
    W["model.audio_head"] = mat(5, (K - 1, dd, Va), math.sqrt(3.0 / dd) * 2.0)
    return W


def raw_key(k: str) -> str:
    """A post-sanitize key in the raw spelling of the unquantised checkpoints (inverse of the key map, MarvisTTSModel.swift:225-262)."""
    k = k[len("model."):]
    k = k.replace("self_attn.o_proj", "attn.output_proj").replace("self_attn", "attn")
    k = k.replace("mlp.gate_proj", "mlp.w1").replace("mlp.down_proj", "mlp.w2").replace("mlp.up_proj", "mlp.w3")
    k = k.replace("input_layernorm.weight", "sa_norm.scale").replace("post_attention_layernorm.weight", "mlp_norm.scale")
    if k in ("backbone.norm.weight", "decoder.norm.weight"):
        k = k.replace("weight", "scale")
    return k


class CSMRef:
    def __init__(self, cfg: CSMConfig, W: dict, round: str | None = "bf16"):
        self.cfg = cfg
        self.r = ollama._rounder(round)
        f32 = {k: torch.as_tensor(v).to(torch.float32) for k, v in W.items()}
        sub = lambda pre: {"model." + k[len(pre):]: v for k, v in f32.items() if k.startswith(pre)}
        self.backbone = CSMLlamaRef(cfg.backbone, sub("model.backbone."), round=round)
        self.decoder = CSMLlamaRef(cfg.decoder, sub("model.decoder."), round=round)
        self.text_emb, self.audio_emb = f32["model.text_embeddings.weight"], f32["model.audio_embeddings.weight"]
        self.proj, self.head0 = f32["model.projection.weight"], f32["model.codebook0_head.weight"]
        self.heads = f32["model.audio_head"]                                     # [K - 1, Dd, Va], used as x @ W[i]

    def embed_positions(self, tok, msk):
        """_embedTokens + masked sum (CSMModel.swift:476-478,534-557): float32 accumulation in codebook order then text, one rounding."""
        tok, msk = np.asarray(tok), np.asarray(msk)
        K, Va = tok.shape[1] - 1, self.cfg.audio_vocab_size
        out = torch.zeros(tok.shape[0], self.text_emb.shape[1])
        for t in range(tok.shape[0]):
            for i in range(K):
                if msk[t, i]:
                    out[t] += self.audio_emb[i * Va + int(tok[t, i])]
            if msk[t, K]:
                out[t] += self.text_emb[int(tok[t, K])]
        return self.r(out)

    def project(self, x):
        return self.r(x @ self.proj.t())

    def run(self, tok, msk, n_frames: int, Cb: int, temperature: float, top_p: float, seed: int, row: int, forced=None,
            want_logits: bool = False):
        """The generate loop for one row (MarvisTTSModel.swift:433-460 around generateFrame): returns (codes [n, Cb] the loop continued
        from, sampled [n', Cb], logits [n', Cb, Va] if want_logits).  forced [F, Cb]: the loop samples as usual but continues from the
        forced codes; an all-zero (continued) frame ends the row and is not kept."""
        K, Va = self.cfg.audio_num_codebooks, self.cfg.audio_vocab_size
        self.backbone.reset(1)
        x = self.embed_positions(tok, msk)
        kept, sampled, logits = [], [], []
        with torch.no_grad():
            for f in range(n_frames):
                l0 = self.backbone.forward_embeds(0, x, head=self.head0)[-1].numpy()
                last_h = self.backbone.last_hidden[-1]
                fl, fs, fc = [l0], [], []
                c = osampler.sample(l0, temperature, top_p, seed, row, f * K + 0)
                fs.append(c)
                c = int(forced[f][0]) if forced is not None else c
                fc.append(c)
                self.decoder.reset(1)
                cur = torch.stack([self.project(last_h), self.project(self.audio_emb[0 * Va + c])])
                for i in range(1, Cb):
                    li = self.decoder.forward_embeds(0, cur, head=self.heads[i - 1].t())[-1].numpy()
                    fl.append(li)
                    c = osampler.sample(li, temperature, top_p, seed, row, f * K + i)
                    fs.append(c)
                    c = int(forced[f][i]) if forced is not None else c
                    fc.append(c)
                    cur = self.project(self.audio_emb[i * Va + c])[None]
                sampled.append(fs); logits.append(np.stack(fl))
                if sum(fc) == 0:
                    break
                kept.append(fc)
                nxt = np.zeros((1, K + 1), np.int64); m = np.zeros((1, K + 1), np.uint8)
                nxt[0, :Cb] = fc; m[0, :Cb] = 1
                x = self.embed_positions(nxt, m)
        out = (np.asarray(kept, np.int32).reshape(-1, Cb), np.asarray(sampled, np.int32))
        return out + (np.stack(logits),) if want_logits else out
