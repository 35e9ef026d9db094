"""Torch-CPU restatement of the reference Moonshine model (Sources/MLXAudioSTT/Models/Moonshine/MoonshineModel.swift:71-411), written
from the Swift - the parity reference of csrc/moonshine.hip.

round="bf16": the engine's rounding points - f32 from the waveform through GroupNorm, one rounding there, then bf16 after every
primitive (LayerNorm, Linear + bias, GELU, RoPE, attention output, residual add, SiLU, gate product); logits stay f32; weights are bf16
except conv1 and the GroupNorm affine.  round=None: no rounding anywhere (the distance between the two is the cost of running an f32
checkpoint in bf16).  acc=torch.float64: same graph and rounding points with every contraction, statistic and softmax accumulated in
float64 - the noise floor two exact realisations of one specification have between them.

Weights are taken in the PUBLISHED key layout ("model.encoder.conv1.weight" [d, 1, 127], conv weights [out, in, k], "proj_out.weight"),
as make_weights() produces them and transformers' MoonshineForConditionalGeneration names them."""
import math

import torch
import torch.nn.functional as F


def rotary_dim(head_dim, factor):                                   # :142-144
    r = int(torch.tensor(float(head_dim), dtype=torch.float32) * torch.tensor(float(factor), dtype=torch.float32))
    r -= r % 2
    return max(2, r)


def frames(n):                                                      # unpadded convs k 127/7/3, stride 64/3/2 (:309-312)
    t1 = (n - 127) // 64 + 1 if n >= 127 else 0
    t2 = (t1 - 7) // 3 + 1 if t1 >= 7 else 0
    return (t2 - 3) // 2 + 1 if t2 >= 3 else 0


def make_weights(cfg, seed=0):
    """Random weights for a mas.MoonshineConfig-like cfg, published keys, float32."""
    g = torch.Generator().manual_seed(seed)
    d, f, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    W = {}

    def u(shape, amp, plus=0.0):
        return (torch.rand(shape, generator=g) * 2 - 1) * amp + plus

    def lin(p, o, i, bias, gain=1.0):
        W[p + ".weight"] = u((o, i), gain * math.sqrt(3.0 / i))
        if bias:
            W[p + ".bias"] = u((o,), 0.05)

    def attn(p, H, Hk):
        hd = d // H
        lin(p + ".q_proj", H * hd, d, cfg.attention_bias); lin(p + ".k_proj", Hk * hd, d, cfg.attention_bias)
        lin(p + ".v_proj", Hk * hd, d, cfg.attention_bias); lin(p + ".o_proj", d, H * hd, False, 0.5)

    E, D = "model.encoder", "model.decoder"
    W[E + ".conv1.weight"] = u((d, 1, 127), 4.0 * math.sqrt(3.0 / 127))
    W[E + ".groupnorm.weight"] = u((d,), 0.1, 1.0); W[E + ".groupnorm.bias"] = u((d,), 0.05)
    W[E + ".conv2.weight"] = u((2 * d, d, 7), math.sqrt(3.0 / (7 * d))); W[E + ".conv2.bias"] = u((2 * d,), 0.05)
    W[E + ".conv3.weight"] = u((d, 2 * d, 3), math.sqrt(3.0 / (6 * d))); W[E + ".conv3.bias"] = u((d,), 0.05)
    for i in range(cfg.encoder_num_hidden_layers):
        q = f"{E}.layers.{i}"
        attn(q + ".self_attn", cfg.encoder_num_attention_heads, cfg.encoder_num_key_value_heads)
        W[q + ".input_layernorm.weight"] = u((d,), 0.1, 1.0); W[q + ".post_attention_layernorm.weight"] = u((d,), 0.1, 1.0)
        lin(q + ".mlp.fc1", f, d, True); lin(q + ".mlp.fc2", d, f, True, 0.5)
    W[E + ".layer_norm.weight"] = u((d,), 0.1, 1.0)
    W[D + ".embed_tokens.weight"] = u((V, d), 0.5)
    for i in range(cfg.decoder_num_hidden_layers):
        q = f"{D}.layers.{i}"
        attn(q + ".self_attn", cfg.decoder_num_attention_heads, cfg.decoder_num_key_value_heads)
        attn(q + ".encoder_attn", cfg.decoder_num_attention_heads, cfg.decoder_num_key_value_heads)
        for n in ("input_layernorm", "post_attention_layernorm", "final_layernorm"):
            W[f"{q}.{n}.weight"] = u((d,), 0.1, 1.0)
        lin(q + ".mlp.fc1", 2 * f, d, True); lin(q + ".mlp.fc2", d, f, True, 0.5)
    W[D + ".norm.weight"] = u((d,), 0.1, 1.0)
    if not cfg.tie_word_embeddings:
        W["proj_out.weight"] = u((V, d), 0.5)
    return W


def pad_heads(cfg, W, to=64):
    """The engine's load-time transform: every head's q/k/v rows (and biases) zero-padded to `to`, the matching o_proj columns too."""
    out = dict(W)
    d = cfg.hidden_size

    def rows(w, H, hd):
        w = w.reshape(H, hd, *w.shape[1:])
        pad = torch.zeros(H, to - hd, *w.shape[2:], dtype=w.dtype)
        return torch.cat([w, pad], 1).reshape(H * to, *w.shape[2:])

    for side, H, Hk, L, kinds in (("encoder", cfg.encoder_num_attention_heads, cfg.encoder_num_key_value_heads, cfg.encoder_num_hidden_layers,
                                   ("self_attn",)),
                                  ("decoder", cfg.decoder_num_attention_heads, cfg.decoder_num_key_value_heads, cfg.decoder_num_hidden_layers,
                                   ("self_attn", "encoder_attn"))):
        hd = d // H
        for i in range(L):
            for kind in kinds:
                p = f"model.{side}.layers.{i}.{kind}"
                for proj, n in (("q_proj", H), ("k_proj", Hk), ("v_proj", Hk)):
                    out[f"{p}.{proj}.weight"] = rows(W[f"{p}.{proj}.weight"], n, hd)
                    if f"{p}.{proj}.bias" in W:
                        out[f"{p}.{proj}.bias"] = rows(W[f"{p}.{proj}.bias"], n, hd)
                o = W[f"{p}.o_proj.weight"].reshape(d, H, hd)
                out[f"{p}.o_proj.weight"] = torch.cat([o, torch.zeros(d, H, to - hd)], 2).reshape(d, H * to)
    return out


class MoonshineRef:
    def __init__(self, cfg, W, round="bf16", acc=torch.float32):
        self.cfg, self.round, self.acc = cfg, round, acc
        keep = ("model.encoder.conv1.weight", "model.encoder.groupnorm.weight", "model.encoder.groupnorm.bias")
        self.w = {k: (v.float() if (round is None or k in keep) else v.float().bfloat16().float()) for k, v in W.items()}
        self.d = cfg.hidden_size
        self.caches = None

    # ---- primitives
    def r(self, x):
        x = x.float()
        return x.bfloat16().float() if self.round == "bf16" else x

    def linear(self, x, p):
        y = x.to(self.acc) @ self.w[p + ".weight"].to(self.acc).t()
        if p + ".bias" in self.w:
            y = y + self.w[p + ".bias"].to(self.acc)
        return self.r(y)

    def ln(self, x, p):                                              # LayerNorm(bias: false), eps 1e-5 (:247)
        xa = x.to(self.acc)
        m = xa.mean(-1, keepdim=True)
        v = ((xa - m) ** 2).mean(-1, keepdim=True)
        return self.r((xa - m) / torch.sqrt(v + 1e-5) * self.w[p + ".weight"].to(self.acc))

    def gelu(self, x):
        xa = x.to(self.acc)
        return self.r(0.5 * xa * (1.0 + torch.erf(xa / math.sqrt(2.0))))

    def rope(self, x, rot, pos):                                     # x [H, T, hd]; interleaved pairs of the first rot columns (:80-110,165-178)
        inv = 1.0 / torch.pow(torch.tensor(float(self.cfg.rope_theta), dtype=torch.float32), torch.arange(0, rot, 2, dtype=torch.float32) / rot)
        a = (pos.float()[:, None] * inv[None]).double()
        cos = torch.cos(a).float().repeat_interleave(2, -1).to(self.acc)
        sin = torch.sin(a).float().repeat_interleave(2, -1).to(self.acc)
        xr = x[..., :rot].to(self.acc)
        pairs = xr.reshape(*xr.shape[:-1], rot // 2, 2)
        half = torch.stack([-pairs[..., 1], pairs[..., 0]], -1).reshape(xr.shape)
        return torch.cat([self.r(xr * cos + half * sin), x[..., rot:]], -1)

    def attention(self, p, x, src, H, Hk, causal, q_pos=None, cross=False, kv=None):
        """x [T, d], src [S, d] -> [T, d] (:155-195).  The head size stored in the weights may be padded; scale and rotary_dim come
        from the real head size hidden / heads."""
        real = self.d // H
        rot = rotary_dim(real, self.cfg.partial_rotary_factor)
        T = x.shape[0]
        q = self.linear(x, p + ".q_proj")
        hs = q.shape[-1] // H
        q = q.reshape(T, H, hs).transpose(0, 1)
        if kv is None:
            S = src.shape[0]
            k = self.linear(src, p + ".k_proj").reshape(S, Hk, hs).transpose(0, 1)
            v = self.linear(src, p + ".v_proj").reshape(S, Hk, hs).transpose(0, 1)
            if not cross:
                k = self.rope(k, rot, q_pos)
        else:
            k, v = kv
        if not cross:
            q = self.rope(q, rot, q_pos)
        new_kv = (k, v)
        if H // Hk > 1:
            k = k.repeat_interleave(H // Hk, 0); v = v.repeat_interleave(H // Hk, 0)
        s = (q.to(self.acc) @ k.to(self.acc).transpose(1, 2)) * (float(real) ** -0.5)
        if causal and T > 1:
            s = s + torch.triu(torch.full((T, k.shape[1]), float("-inf"), dtype=self.acc), diagonal=1 + k.shape[1] - T)
        o = self.r(torch.softmax(s, -1) @ v.to(self.acc))
        return self.linear(o.transpose(0, 1).reshape(T, H * hs), p + ".o_proj"), new_kv

    # ---- encoder
    def stem(self, audio):
        """audio [n] -> dict of the four stage outputs [T, C] (:318-324)"""
        w, E = self.w, "model.encoder"
        x = torch.as_tensor(audio, dtype=torch.float32).reshape(1, 1, -1).to(self.acc)
        c1 = torch.tanh(F.conv1d(x, w[E + ".conv1.weight"].to(self.acc), stride=64))[0].float()          # [d, T1], f32 kept
        xa = c1.to(self.acc)
        m = xa.mean()
        v = ((xa - m) ** 2).mean()
        gn = self.r((xa - m) / torch.sqrt(v + 1e-5) * w[E + ".groupnorm.weight"].to(self.acc)[:, None] + w[E + ".groupnorm.bias"].to(self.acc)[:, None])
        c2 = self.gelu(self.r(F.conv1d(gn[None].to(self.acc), w[E + ".conv2.weight"].to(self.acc), w[E + ".conv2.bias"].to(self.acc), stride=3)[0]))
        c3 = self.gelu(self.r(F.conv1d(c2[None].to(self.acc), w[E + ".conv3.weight"].to(self.acc), w[E + ".conv3.bias"].to(self.acc), stride=2)[0]))
        return {0: c1.t().contiguous(), 1: gn.t().contiguous(), 2: c2.t().contiguous(), 3: c3.t().contiguous()}

    def encode(self, audio):
        c = self.cfg
        h = self.stem(audio)[3]
        pos = torch.arange(h.shape[0])
        for i in range(c.encoder_num_hidden_layers):
            q = f"model.encoder.layers.{i}"
            x = self.ln(h, q + ".input_layernorm")
            a, _ = self.attention(q + ".self_attn", x, x, c.encoder_num_attention_heads, c.encoder_num_key_value_heads, False, pos)
            h = self.r(a + h)
            x = self.ln(h, q + ".post_attention_layernorm")
            h = self.r(self.linear(self.gelu(self.linear(x, q + ".mlp.fc1")), q + ".mlp.fc2") + h)
        return self.ln(h, "model.encoder.layer_norm")

    # ---- decoder
    def _dec_layer(self, i, h, enc, pos, self_kv=None, cross_kv=None):
        c, q = self.cfg, f"model.decoder.layers.{i}"
        H, Hk = c.decoder_num_attention_heads, c.decoder_num_key_value_heads
        x = self.ln(h, q + ".input_layernorm")
        if self_kv is None:
            a, kv = self.attention(q + ".self_attn", x, x, H, Hk, True, pos)
        else:                                                        # cached: one new position appended
            real = self.d // H
            rot = rotary_dim(real, c.partial_rotary_factor)
            k = self.linear(x, q + ".self_attn.k_proj"); hs = k.shape[-1] // Hk
            k = self.rope(k.reshape(1, Hk, hs).transpose(0, 1), rot, pos)
            v = self.linear(x, q + ".self_attn.v_proj").reshape(1, Hk, hs).transpose(0, 1)
            kv = (torch.cat([self_kv[0], k], 1), torch.cat([self_kv[1], v], 1)) if self_kv[0] is not None else (k, v)
            a, _ = self.attention(q + ".self_attn", x, None, H, Hk, False, pos, kv=kv)
        h = self.r(a + h)
        x = self.ln(h, q + ".post_attention_layernorm")
        a, ckv = self.attention(q + ".encoder_attn", x, enc, H, Hk, False, cross=True, kv=cross_kv)
        h = self.r(a + h)
        x = self.ln(h, q + ".final_layernorm")
        y = self.linear(x, q + ".mlp.fc1")
        a_, g = y[..., : y.shape[-1] // 2], y[..., y.shape[-1] // 2:]
        ga = g.to(self.acc)
        act = self.r(self.r(ga * torch.sigmoid(ga)).to(self.acc) * a_.to(self.acc))      # fc2(silu(b) * a), b the second half (:223-227)
        return self.r(self.linear(act, q + ".mlp.fc2") + h), kv, ckv

    def logits(self, h):                                             # logitsForHidden(norm(x)) (:349,427-432); f32, not rounded
        p = "model.decoder.embed_tokens.weight" if self.cfg.tie_word_embeddings else "proj_out.weight"
        return (self.ln(h, "model.decoder.norm").to(self.acc) @ self.w[p].to(self.acc).t()).float()

    def decode_all(self, tokens, enc):
        """No cache: the whole decoder over all tokens -> logits [T, V] (what the reference recomputes every step, :383-386)."""
        h = self.w["model.decoder.embed_tokens.weight"][torch.as_tensor(tokens, dtype=torch.long)]
        pos = torch.arange(h.shape[0])
        for i in range(self.cfg.decoder_num_hidden_layers):
            h, _, _ = self._dec_layer(i, h, enc, pos)
        return self.logits(h)

    def reset(self, enc):
        L = self.cfg.decoder_num_hidden_layers
        self.caches = dict(enc=enc, pos=0, self_kv=[(None, None)] * L, cross_kv=[None] * L)

    def step(self, token):
        """Cached decoding: one token -> logits [V]."""
        cch = self.caches
        h = self.w["model.decoder.embed_tokens.weight"][torch.as_tensor([int(token)])]
        pos = torch.tensor([cch["pos"]])
        for i in range(self.cfg.decoder_num_hidden_layers):
            h, cch["self_kv"][i], cch["cross_kv"][i] = self._dec_layer(i, h, cch["enc"], pos, cch["self_kv"][i], cch["cross_kv"][i])
        cch["pos"] += 1
        return self.logits(h)[0]

    def generate(self, audio, max_tokens=200, cached=False):
        """generate (:374-399): full recompute per step as the reference does, or through the caches.  -> (generated ids, total tokens)"""
        enc = self.encode(audio)
        tokens, generated = [self.cfg.decoder_start_token_id], []
        if cached:
            self.reset(enc)
        for _ in range(max_tokens):
            lg = self.step(tokens[-1]) if cached else self.decode_all(tokens, enc)[-1]
            nxt = int(lg.argmax())
            if nxt == self.cfg.eos_token_id:
                break
            tokens.append(nxt); generated.append(nxt)
        return generated, len(tokens)
