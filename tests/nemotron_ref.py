"""CPU specification of Nemotron ASR (csrc/nemotron.hip, mlx-audio-swift_amd/nemotron.py), float64 or float32 by `dtype`, one row at a time.
What Parakeet's and Sortformer's specifications hold is imported; added here: the literal chunked-limited mask (additive -1e9 over the full
literal rel-shift scores), the causal stem, the conv module with torch's layer_norm, the prompt kernel as a literal concatenation and a
transliteration of NemotronASRModel.decode's loop."""
import math

import numpy as np
import torch
import torch.nn.functional as Fn

import parakeet_ref as P
import sortformer_ref as R

LANGS = {"en-US": 0, "de-DE": 3, "auto": 5}


def context(left, right):
    C = max(right + 1, 1)
    return C, (left // C if left >= 0 else 1_000_000)


def mask(T, left, right):
    """createChunkedLimitedMask: [T, T] additive, 0 where 0 <= q / C - k / C <= L, else -1e9"""
    C, L = context(left, right)
    ch = np.arange(T) // C
    diff = ch[:, None] - ch[None]
    return np.where((diff >= 0) & (diff <= L), 0.0, -1e9)


def half(n):
    return n // 2 + 1


def frames(F):
    return half(half(half(F)))


# ---------------------------------------------------------------------------------------------------- encoder
def case_config(hidden, layers=2, bias=True, prompt=True, contexts=((56, 13), (4, 1)), conv="causal", taps=9, rnn_layers=2, max_symbols=3, **ws):
    import mlx_audio_swift_amd as mas
    ws = dict(dict(max_batch=4, max_seconds=4, max_tokens=256), **ws)
    return mas.NemotronConfig(num_mel_bins=16, hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=2, intermediate_size=2 * hidden,
                              conv_kernel_size=taps, conv_context_size=conv, subsampling_conv_channels=16, att_context_size=[list(c) for c in contexts],
                              attention_bias=bias, num_prompts=8 if prompt else 0, prompt_hidden=48 if prompt else 0, prompt_dictionary=dict(LANGS),
                              pred_hidden=32, pred_rnn_layers=rnn_layers, joint_hidden=32, vocab_size=40, max_symbols=max_symbols,
                              vocabulary=[f"▁t{i}" for i in range(38)] + ["<en-US>", "<|nospeech|>"], **ws)


def make_decoder(seed, P_, J, vocab, layers=2, gain=4.0):
    W = P.make_decoder(seed, P_, J, vocab, D=0, gain=gain)
    return {k: v for k, v in W.items() if layers == 2 or not k.endswith("_l1")}


def make_weights(cfg, seed):
    """every tensor of the engine: Sortformer's generator for the blocks (BatchNorm statistics dropped: conv.norm is a LayerNorm), the stem's
    linear at the causal width, the prompt kernel, joint.enc and the decoder"""
    W = {k.replace("fc_encoder.", "encoder.", 1): v for k, v in R.synthetic_weights(P.sf_config(cfg), seed).items()
         if k.startswith("fc_encoder.") and "running_" not in k}
    if not cfg.attention_bias:
        W = {k: v for k, v in W.items() if not (k.endswith(".bias") and any(n in k for n in ("feed_forward", "_proj", "pointwise", "depthwise")) and "norm" not in k)}
    rng = np.random.default_rng(seed + 1)
    u = lambda shape, amp: rng.uniform(-amp, amp, shape).astype(np.float32)
    d, K = cfg.hidden_size, cfg.subsampling_conv_channels * frames(cfg.num_mel_bins)
    W["encoder.subsampling.linear.weight"], W["encoder.subsampling.linear.bias"] = u((d, K), math.sqrt(3.0 / K)), u((d,), 0.05)
    W["joint.enc.weight"], W["joint.enc.bias"] = u((cfg.joint_hidden, d), math.sqrt(3.0 / d)), u((cfg.joint_hidden,), 0.05)
    if cfg.prompt_hidden:
        PH, NP = cfg.prompt_hidden, cfg.num_prompts
        W["prompt_kernel.linear0.weight"], W["prompt_kernel.linear0.bias"] = u((PH, d + NP), math.sqrt(3.0 / d)), u((PH,), 0.05)
        W["prompt_kernel.linear2.weight"], W["prompt_kernel.linear2.bias"] = u((d, PH), math.sqrt(3.0 / PH)), u((d,), 0.05)
    W.update(make_decoder(seed + 2, cfg.pred_hidden, cfg.joint_hidden, cfg.vocab_size, cfg.pred_rnn_layers))
    return W


def causal_conv(x, w, b, groups=1):
    """pad (2, 1) in time and frequency, k3 s2; x NCHW, w [O, 3, 3, I / groups]"""
    return Fn.conv2d(Fn.pad(x, (2, 1, 2, 1)), w.permute(0, 3, 1, 2), b, stride=2, groups=groups)


def conv_module(W, q_, x, pads):
    """NemotronASRConvolution: GLU -> pad (left, right) -> depthwise conv -> LayerNorm over channels -> SiLU -> pointwise conv; x [T, d]"""
    h = Fn.linear(x, W[q_ + "pointwise_conv1.weight"][:, 0], W.get(q_ + "pointwise_conv1.bias"))
    a, b = h.chunk(2, dim=-1)
    h = Fn.pad((a * torch.sigmoid(b)).t()[None], pads)
    h = Fn.conv1d(h, W[q_ + "depthwise_conv.weight"].permute(0, 2, 1), W.get(q_ + "depthwise_conv.bias"), groups=h.shape[1])[0].t()
    dw = h
    h = Fn.silu(Fn.layer_norm(h, h.shape[-1:], W[q_ + "norm.weight"], W[q_ + "norm.bias"], 1e-5))
    return Fn.linear(h, W[q_ + "pointwise_conv2.weight"][:, 0], W.get(q_ + "pointwise_conv2.bias")), dw


class Encoder(P.Encoder):
    def __init__(self, cfg, weights, dtype, ctx=None):
        super().__init__(cfg, weights, dtype)
        self.n, self.ctx = cfg, tuple(ctx or cfg.default_context)

    def features(self, wave):
        return R.features(wave, self.n.num_mel_bins, self.dtype, peak_normalize=False, normalize=(self.n.normalize or "NA").lower() == "per_feature", pad_to=0)

    def pre_encode(self, feats):
        W, S, C = self.W, "fc_encoder.subsampling.", self.n.subsampling_conv_channels
        pw = lambda n, x: Fn.conv2d(x, W[S + n + ".weight"].permute(0, 3, 1, 2), W[S + n + ".bias"])
        h = torch.relu(causal_conv(feats[None, None], W[S + "layers_0.weight"], W[S + "layers_0.bias"]))
        h = torch.relu(pw("layers_3", causal_conv(h, W[S + "layers_2.weight"], W[S + "layers_2.bias"], C)))
        h = torch.relu(pw("layers_6", causal_conv(h, W[S + "layers_5.weight"], W[S + "layers_5.bias"], C)))
        return self.lin(S + "linear", h[0].permute(1, 0, 2).reshape(h.shape[2], -1))

    def fc_attn(self, q_, x, band=False):
        T, H = x.shape[0], self.n.num_attention_heads
        hd = self.n.hidden_size // H
        sp = lambda y: y.reshape(-1, H, hd).transpose(0, 1)
        q, k, v = (sp(self.lin(q_ + n, x)) for n in ("q_proj", "k_proj", "v_proj"))
        p = sp(Fn.linear(self.pos_emb(T), self.W[q_ + "relative_k_proj.weight"]))
        s = self.rel_scores(q, k, p, self.W[q_ + "bias_u"], self.W[q_ + "bias_v"]) + torch.as_tensor(mask(T, *self.ctx)).to(self.dtype)
        return self.lin(q_ + "o_proj", (torch.softmax(s, dim=-1) @ v).transpose(0, 1).reshape(T, H * hd))

    def conv_module(self, q_, x):
        l, r = self.n.conv_pads
        return conv_module(self.W, q_, x, (l, r))[0]

    def prompt(self, x, index):
        """applyPrompt, literally: the one-hot is concatenated"""
        if not self.n.prompt_hidden:
            return x
        hot = torch.zeros(x.shape[0], self.n.num_prompts, dtype=self.dtype)
        hot[:, index] = 1.0
        return self.lin("prompt_kernel.linear2", torch.relu(self.lin("prompt_kernel.linear0", torch.cat([x, hot], dim=1))))

    def stage_after(self, stage, prev, index=0):
        """device stage `stage` (mis_nemotron_tap numbering, >= 1) from the DEVICE's stage - 1 tensor of one row"""
        x = torch.as_tensor(np.asarray(prev, np.float32)).to(self.dtype)
        L = self.n.num_hidden_layers
        if stage == L + 1:
            return self.prompt(x, index)
        if stage == L + 2:
            return self.joint_enc(x)
        return self.fc_layer(stage - 1, self.intake(x) if stage == 1 else x)


def attention(qkv, table, u, v, n, H, hd, Tcap, ctx, dtype, band=False):
    """one row of k_nm_attn: qkv [T, 3 H hd] (n live rows), table [2 Tcap - 1, H hd] by distance (row dist + Tcap - 1) -> [n, H hd].
    Literal: the full rel-shift scores + the additive mask.  band: the device's form - only distances -(C - 1) .. L C + C - 1 are taken from
    the table (others count as 0) and an unseen key is excluded."""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dtype)
    x = t(qkv[:n])
    sp = lambda y: y.reshape(-1, H, hd).transpose(0, 1)
    q, k, val = (sp(x[:, i * H * hd:(i + 1) * H * hd]) for i in range(3))
    m = torch.as_tensor(mask(n, *ctx))
    if band:
        C, L = context(*ctx)
        dist = torch.arange(n)[:, None] - torch.arange(n)[None]
        inb = (dist >= -(C - 1)) & (dist <= L * C + C - 1)
        tab = torch.nan_to_num(t(table))
        pd = sp(tab[(dist + Tcap - 1).clamp(0, 2 * Tcap - 2).reshape(-1)]).reshape(H, n, n, hd) * inb[None, :, :, None]
        s = ((q + t(u)[:, None]) @ k.transpose(1, 2) + torch.einsum("hid,hijd->hij", q + t(v)[:, None], pd)) / math.sqrt(hd)
        s = s.masked_fill(m[None] != 0, -math.inf)
    else:
        p = sp(t(table)[[Tcap - 1 + d for d in range(n - 1, -n, -1)]])
        s = object.__new__(R.Ref).rel_scores(q, k, p, t(u), t(v)) + m.to(dtype)
    return (torch.softmax(s, dim=-1) @ val).transpose(0, 1).reshape(n, H * hd).numpy()


# ---------------------------------------------------------------------------------------------------- decoder
def predict(W, token, blank, h, c):
    """-> (joint.pred of the top layer's new h, new h [layers, P], new c); a blank feeds zeros (blank_as_pad)"""
    x = np.zeros_like(h[0]) if token == blank else W["decoder.prediction.embed.weight"][token]
    hs, cs = [], []
    for l in range(h.shape[0]):
        x, c2 = P.lstm_cell(W, l, x, h[l], c[l])
        hs.append(x); cs.append(c2)
    return W["joint.pred.weight"] @ x + W["joint.pred.bias"], np.stack(hs), np.stack(cs)


def rnnt_decode(W32, encp, vocab, max_symbols, cap, dtype=np.float64, follow=None):
    """NemotronASRModel.decode's loop with NemoDecodingLogic.rnntStep on projected frames encp [T, J], one statement at a time: the
    prediction network runs at EVERY step from the committed state.  Added: the output capacity (flag) and the step count.  follow: the
    decisions of another run to take instead of the own arg-max."""
    W = {k: v.astype(dtype) for k, v in W32.items()}
    encp = np.asarray(encp, dtype)
    blank, Pn = vocab, W["joint.pred.weight"].shape[1]
    layers = sum(1 for k in W if "weight_ih_l" in k)
    out = dict(tokens=[], frames=[], flag=0, steps=0, gap=np.inf, logits=[], decisions=[])
    last_token, state = blank, (np.zeros((layers, Pn), dtype), np.zeros((layers, Pn), dtype))
    time, new_symbols = 0, 0
    while time < encp.shape[0]:
        pred, hidden, cell = predict(W, last_token, blank, state[0], state[1])
        lg = P.logits(W, encp[time], pred)
        top = np.sort(lg)[::-1]
        out["gap"] = min(out["gap"], float(top[0] - top[1]))
        out["logits"].append(lg)
        token = int(np.argmax(lg)) if follow is None else follow[out["steps"]]
        out["decisions"].append(token)
        out["steps"] += 1
        if token == blank:
            time, new_symbols = time + 1, 0
            continue
        if len(out["tokens"]) >= cap:
            out["flag"] = 1
            break
        last_token, state = token, (hidden, cell)
        out["tokens"].append(token); out["frames"].append(time)
        next_symbols = new_symbols + 1
        if max_symbols is not None and next_symbols >= max_symbols:
            time, new_symbols = time + 1, 0
        else:
            new_symbols = next_symbols
    return out


# ---------------------------------------------------------------------------------------------------- the decode cases of both test files
RNNT = dict(P=32, J=32, vocab=40, max_symbols=3, cap=20, Tp=24)
RNNT_SEED = 12                     # chosen on the CPU: test_nemotron_cpu holds the margin it must keep


def rnnt_cases(layers):
    """-> (W, rows): rows = [(name, encp [Tp, J] float32 with NaN junk behind T, T, joint_net bias override, max_symbols)]; a case with an
    override is its own launch"""
    c = RNNT
    W = make_decoder(RNNT_SEED + layers, c["P"], c["J"], c["vocab"], layers)
    rng = np.random.default_rng(RNNT_SEED + 100)

    def row(T):
        e = np.full((c["Tp"], c["J"]), np.nan, np.float32)
        e[:T] = rng.uniform(-1.5, 1.5, (T, c["J"])).astype(np.float32)
        return e, T

    def bias(tok, amp=60.0):
        b = W["joint.joint_net.bias"].copy()
        b[tok] += amp
        return b

    ms = c["max_symbols"]
    return W, [("count_1", *row(1), None, ms), ("ragged_a", *row(7), None, ms), ("ragged_b", *row(19), None, ms), ("full", *row(c["Tp"]), None, ms),
               ("all_blank", *row(9), bias(c["vocab"]), ms), ("always_emit", *row(5), bias(3), ms), ("no_max_symbols_capacity", *row(6), bias(7), None)]
