"""CPU specification of Canary (csrc/canary.hip, mlx-audio-swift_amd/canary.py).  The encoder is parakeet_ref.Encoder under Canary's
config; the decoder is plain torch, float64 or float32 by `dtype`, in two forms: the reference's (the whole prefix under a causal mask at
every token, CanaryDecoder.callAsFunction) and a cached step.  One row at a time."""
import math
import types

import numpy as np
import torch
import torch.nn.functional as F

import parakeet_ref as P
import sortformer_ref as R

EOS = 3


def case_config(h, heads, inner=None, vocab=203, d_model=None, max_batch=4, max_seconds=4, max_tokens=12, max_prompt=8):
    import mlx_audio_swift_amd as mas
    return mas.CanaryConfig(preprocessor=mas.CanaryPreprocessConfig(features=16),
                            encoder=mas.CanaryEncoderConfig(feat_in=16, n_layers=2, d_model=d_model or h, n_heads=2, ff_expansion_factor=2,
                                                            subsampling_conv_channels=16),
                            decoder=mas.CanaryDecoderConfig(num_layers=2, hidden_size=h, num_attention_heads=heads, inner_size=inner or 2 * h),
                            vocab_size=vocab, enc_output_dim=h, max_batch=max_batch, max_seconds=max_seconds, max_tokens=max_tokens, max_prompt=max_prompt)


def encoder_view(cfg):
    """the fields of a CanaryConfig that parakeet_ref.Encoder reads"""
    e = cfg.encoder
    return types.SimpleNamespace(hidden_size=e.d_model, num_hidden_layers=e.n_layers, num_attention_heads=e.n_heads,
                                 intermediate_size=e.d_model * e.ff_expansion_factor, num_mel_bins=cfg.preprocessor.features,
                                 conv_kernel_size=e.conv_kernel_size, subsampling_conv_channels=e.subsampling_conv_channels, attention_bias=e.use_bias,
                                 scale_input=e.xscaling)


def make_decoder(seed, h, inner, vocab, layers=2, head_gain=6.0):
    """the decoder's tensors under the engine's names, float32.  head_gain spreads the logits: test_canary_cpu.test_decision_margin holds the
    margin the token comparisons need."""
    rng = np.random.default_rng(seed)
    u = lambda shape, amp: rng.uniform(-amp, amp, shape).astype(np.float32)
    W = {"decoder.embedding.weight": u((vocab, h), 1.0)}

    def lin(p, o, i, gain=1.0):
        W[p + ".weight"], W[p + ".bias"] = u((o, i), gain * math.sqrt(3.0 / i)), u((o,), 0.05)

    def norm(p):
        W[p + ".weight"], W[p + ".bias"] = 1 + u((h,), 0.1), u((h,), 0.05)

    norm("decoder.embedding_layer_norm"); norm("decoder.final_norm")
    for l in range(layers):
        q = f"decoder.blocks.{l}."
        for n in ("self_attn_norm", "cross_attn_norm", "ff_norm"):
            norm(q + n)
        for at in ("self_attn.", "cross_attn."):
            for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
                lin(q + at + n, h, h, 0.5 if n == "out_proj" else 1.0)
        lin(q + "ff1", inner, h); lin(q + "ff2", h, inner, 0.5)
    lin("decoder.output_proj", vocab, h, head_gain)
    return W


def make_weights(cfg, seed):
    W = {k.replace("fc_encoder.", "encoder.", 1): v for k, v in R.synthetic_weights(P.sf_config(encoder_view(cfg)), seed).items() if k.startswith("fc_encoder.")}
    if cfg.encoder.d_model != cfg.enc_output_dim:
        rng = np.random.default_rng(seed + 1)
        W["encoder.projection.weight"] = (rng.uniform(-1, 1, (cfg.enc_output_dim, cfg.encoder.d_model)) * math.sqrt(3.0 / cfg.encoder.d_model)).astype(np.float32)
        W["encoder.projection.bias"] = rng.uniform(-0.05, 0.05, cfg.enc_output_dim).astype(np.float32)
    W.update(make_decoder(seed + 2, cfg.enc_output_dim, cfg.decoder.inner_size, cfg.vocab_size, cfg.decoder.num_layers))
    return W


def position_table(h, dtype, rows=1024):
    """CanaryFixedPositionalEncoding: sin | cos interleaved over frequency 10000^(-c / h), all over sqrt(h); formed in double (the engine's
    table) and taken to `dtype`"""
    pos = torch.arange(rows, dtype=torch.float64)[:, None]
    div = torch.exp(-math.log(10000.0) * torch.arange(0, h, 2, dtype=torch.float64) / h)
    t = torch.zeros(rows, h, dtype=torch.float64)
    t[:, 0::2] = torch.sin(pos * div)
    t[:, 1::2] = torch.cos(pos * div)[:, : h // 2]
    return (t / math.sqrt(h)).to(torch.float32).to(dtype)             # rounded once to f32, as the engine's


class Decoder:
    def __init__(self, W, heads, dtype, layers=2):
        self.W = {k: torch.as_tensor(np.asarray(v, np.float32)).to(dtype) for k, v in W.items() if k.startswith(("decoder.", "encoder.projection"))}
        self.H, self.L, self.dtype = heads, layers, dtype
        self.h = self.W["decoder.embedding.weight"].shape[1]
        self.table = position_table(self.h, dtype)

    def lin(self, p, x):
        return F.linear(x, self.W[p + ".weight"], self.W[p + ".bias"])

    def norm(self, p, x):
        return F.layer_norm(x, (self.h,), self.W[p + ".weight"], self.W[p + ".bias"], 1e-5)

    def project(self, enc):
        x = torch.as_tensor(np.asarray(enc, np.float32)).to(self.dtype) if not torch.is_tensor(enc) else enc.to(self.dtype)
        return self.lin("encoder.projection", x) if "encoder.projection.weight" in self.W else x

    def embed(self, tokens, start=0):
        pos = [min(start + i, self.table.shape[0] - 1) for i in range(len(tokens))]
        return self.norm("decoder.embedding_layer_norm", self.W["decoder.embedding.weight"][list(tokens)] + self.table[pos])

    def attend(self, p, x, kv, mask=None):
        """CanaryAttention on [T, h] / [S, h]; mask additive [T, S]"""
        sp = lambda y: y.reshape(y.shape[0], self.H, -1).transpose(0, 1)
        q, k, v = sp(self.lin(p + ".q_proj", x)), sp(self.lin(p + ".k_proj", kv)), sp(self.lin(p + ".v_proj", kv))
        s = q @ k.transpose(1, 2) * (q.shape[-1] ** -0.5)
        if mask is not None:
            s = s + mask
        return self.lin(p + ".out_proj", (torch.softmax(s, -1) @ v).transpose(0, 1).reshape(x.shape[0], -1))

    def block(self, l, x, enc, mask):
        q = f"decoder.blocks.{l}."
        n = self.norm(q + "self_attn_norm", x)
        x = x + self.attend(q + "self_attn", n, n, mask)
        x = x + self.attend(q + "cross_attn", self.norm(q + "cross_attn_norm", x), enc)
        return x + self.lin(q + "ff2", torch.relu(self.lin(q + "ff1", self.norm(q + "ff_norm", x))))

    def prefix(self, tokens, enc):
        """the reference's form: the whole prefix, causal mask -> (logits [T, V], hidden [T, h] in front of final_norm)"""
        T = len(tokens)
        x = self.embed(tokens)
        mask = torch.triu(torch.full((T, T), -1e9, dtype=self.dtype), 1) if T > 1 else None
        for l in range(self.L):
            x = self.block(l, x, enc, mask)
        return self.lin("decoder.output_proj", self.norm("decoder.final_norm", x)), x

    def step(self, token, pos, enc, cache):
        """the cached form: one token at position pos; cache[l] = the self_attn_norm outputs of the positions so far"""
        x = self.embed([token], pos)
        for l in range(self.L):
            q = f"decoder.blocks.{l}."
            n = self.norm(q + "self_attn_norm", x)
            cache[l] = n if cache[l] is None else torch.cat([cache[l], n])
            x = x + self.attend(q + "self_attn", n, cache[l])
            x = x + self.attend(q + "cross_attn", self.norm(q + "cross_attn_norm", x), enc)
            x = x + self.lin(q + "ff2", torch.relu(self.lin(q + "ff1", self.norm(q + "ff_norm", x))))
        return self.lin("decoder.output_proj", self.norm("decoder.final_norm", x))[0], x[0]

    def generate(self, prompt, enc, eos, max_tokens, follow=None):
        """CanaryModel.generate's loop on the cached step -> dict(tokens, logits (one vector per decision), gap (smallest top-2 gap)).
        follow: the decisions of another run to take instead of the own arg-max."""
        cache, out = [None] * self.L, dict(tokens=[], logits=[], gap=math.inf)
        for i, t in enumerate(prompt):
            lg, _ = self.step(t, i, enc, cache)
        pos = len(prompt)
        for i in range(max_tokens):
            out["logits"].append(lg)
            top = torch.topk(lg, 2).values
            out["gap"] = min(out["gap"], float(top[0] - top[1]))
            nxt = int(torch.argmax(lg)) if follow is None else follow[i]
            if nxt == eos:
                break
            out["tokens"].append(nxt)
            if i + 1 < max_tokens:
                lg, _ = self.step(nxt, pos, enc, cache)
            pos += 1
        return out


# ---------------------------------------------------------------------------------------------------- the decode cases of both test files
PROMPTS = ([0, 1, 2], [0, 1, 2, 7, 9], [0, 1, 2, 11])
MAX_TOKENS = 6


def decode_cases(W, vocab):
    """name -> the head's bias.  plain: as made (eos pushed away, every row runs to MAX_TOKENS); eos_first: eos wins at once (0 tokens);
    eos_ragged: a moderate eos bias, chosen on the CPU so that the rows end at different steps."""
    b = W["decoder.output_proj.bias"]
    e = np.zeros(vocab, np.float32); e[EOS] = 1.0
    return dict(plain=b - 60.0 * e, eos_first=b + 60.0 * e, eos_ragged=b + EOS_RAGGED_BIAS * e)


EOS_RAGGED_BIAS = np.float32(9.0)    # test_canary_cpu.test_decision_margin asserts what it must give
