"""CPU specification of Parakeet TDT (csrc/parakeet.hip, mlx-audio-swift_amd/parakeet.py).  The encoder is the FastConformer of
tests/sortformer_ref.py (front end without the peak normalisation, stem, block with the LITERAL rel-shift) under Parakeet's names; the
decoder (torch.nn.LSTM-ordered cells, joint, the greedy TDT loop) is numpy, float64 or float32 by `dtype`.  One row at a time."""
import math
import types

import numpy as np
import torch

import sortformer_ref as R

DURATIONS = (0, 1, 2, 3, 4)


# ---------------------------------------------------------------------------------------------------- encoder
def case_config(hidden, heads=2, layers=2, mels=16, channels=16, ffn=None, pred=32, joint=32, vocab=40, max_batch=4, max_seconds=4, max_tokens=256):
    import mlx_audio_swift_amd as mas
    return mas.ParakeetConfig(num_mel_bins=mels, hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads,
                              intermediate_size=ffn or 2 * hidden, conv_kernel_size=9, subsampling_conv_channels=channels, pred_hidden=pred,
                              joint_hidden=joint, vocab_size=vocab, durations=list(DURATIONS), max_symbols=3, vocabulary=[f"▁t{i}" for i in range(vocab)],
                              max_batch=max_batch, max_seconds=max_seconds, max_tokens=max_tokens)


def sf_config(cfg):
    """the view of a ParakeetConfig that sortformer_ref.Ref and synthetic_weights read"""
    e = types.SimpleNamespace(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                              num_key_value_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size, num_mel_bins=cfg.num_mel_bins,
                              conv_kernel_size=cfg.conv_kernel_size, subsampling_conv_channels=cfg.subsampling_conv_channels,
                              attention_bias=cfg.attention_bias, scale_input=cfg.scale_input)
    t = types.SimpleNamespace(d_model=8, encoder_layers=0, encoder_attention_heads=1, encoder_ffn_dim=8, max_source_positions=8, k_proj_bias=False,
                              layer_norm_eps=1e-5)
    return types.SimpleNamespace(fc_encoder_config=e, tf_encoder_config=t, modules_config=types.SimpleNamespace(num_speakers=1))


def make_decoder(seed, P, J, vocab, D=len(DURATIONS), gain=4.0):
    """the decoder's tensors under the engine's names, float32"""
    rng = np.random.default_rng(seed)
    u = lambda shape, amp: rng.uniform(-amp, amp, shape).astype(np.float32)
    W = {"decoder.prediction.embed.weight": u((vocab + 1, P), 1.0)}
    for l in range(2):
        for n, shape in (("weight_ih", (4 * P, P)), ("weight_hh", (4 * P, P)), ("bias_ih", (4 * P,)), ("bias_hh", (4 * P,))):
            W[f"decoder.prediction.dec_rnn.lstm.{n}_l{l}"] = u(shape, math.sqrt(3.0 / P) if n[0] == "w" else 0.05)
    W["joint.pred.weight"], W["joint.pred.bias"] = u((J, P), math.sqrt(3.0 / P)), u((J,), 0.05)
    W["joint.joint_net.weight"], W["joint.joint_net.bias"] = u((vocab + 1 + D, J), gain * math.sqrt(3.0 / J)), u((vocab + 1 + D,), 0.05)
    return W


def make_weights(cfg, seed):
    """every tensor of the engine: the encoder's (sortformer_ref's generator, renamed), joint.enc and the decoder"""
    W = {k.replace("fc_encoder.", "encoder.", 1): v for k, v in R.synthetic_weights(sf_config(cfg), seed).items() if k.startswith("fc_encoder.")}
    rng = np.random.default_rng(seed + 1)
    W["joint.enc.weight"] = rng.uniform(-1, 1, (cfg.joint_hidden, cfg.hidden_size)).astype(np.float32) * np.float32(math.sqrt(3.0 / cfg.hidden_size))
    W["joint.enc.bias"] = rng.uniform(-0.05, 0.05, cfg.joint_hidden).astype(np.float32)
    W.update(make_decoder(seed + 2, cfg.pred_hidden, cfg.joint_hidden, cfg.vocab_size))
    return W


class Encoder(R.Ref):
    def __init__(self, cfg, weights, dtype):
        super().__init__(sf_config(cfg), {k.replace("encoder.", "fc_encoder.", 1): v for k, v in weights.items()}, dtype)

    def features(self, wave):
        return R.features(wave, self.cfg.fc_encoder_config.num_mel_bins, self.dtype, peak_normalize=False, pad_to=0)

    def joint_enc(self, x):
        return self.lin("joint.enc", x)

    def stage_after(self, stage, prev):
        """device stage `stage` (mis_parakeet_tap numbering, >= 1) from the DEVICE's stage - 1 tensor of one row"""
        x = torch.as_tensor(np.asarray(prev, np.float32)).to(self.dtype)
        L = self.cfg.fc_encoder_config.num_hidden_layers
        if stage == L + 1:
            return self.joint_enc(x)
        return self.fc_layer(stage - 1, self.intake(x) if stage == 1 else x)


def attention(qkv, table, u, v, n, H, hd, Tcap, dtype):
    """one row of kernel A: qkv [T, 3 H hd] (n live rows), table [2 Tcap - 1, H hd] by distance -> [n, H hd], the literal rel-shift"""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dtype)
    x = t(qkv[:n])
    sp = lambda y: y.reshape(-1, H, hd).transpose(0, 1)
    q, k, val = (sp(x[:, i * H * hd:(i + 1) * H * hd]) for i in range(3))
    p = sp(t(table)[[Tcap - 1 + dist for dist in range(n - 1, -n, -1)]])
    ref = object.__new__(R.Ref)
    s = ref.rel_scores(q, k, p, t(u), t(v))
    return (torch.softmax(s, dim=-1) @ val).transpose(0, 1).reshape(n, H * hd).numpy()


# ---------------------------------------------------------------------------------------------------- decoder
def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def lstm_cell(W, l, x, h, c):
    """torch.nn.LSTM's cell: gates i, f, g, o"""
    p = "decoder.prediction.dec_rnn.lstm."
    g = W[p + f"weight_ih_l{l}"] @ x + W[p + f"bias_ih_l{l}"] + W[p + f"weight_hh_l{l}"] @ h + W[p + f"bias_hh_l{l}"]
    i, f, gg, o = np.split(g, 4)
    c2 = _sig(f) * c + _sig(i) * np.tanh(gg)
    return _sig(o) * np.tanh(c2), c2


def predict(W, token, blank, h, c):
    """-> (joint.pred of the top layer's new h, new h [2, P], new c); a blank feeds zeros (the reference masks its embedding)"""
    x = np.zeros_like(h[0]) if token == blank else W["decoder.prediction.embed.weight"][token]
    h0, c0 = lstm_cell(W, 0, x, h[0], c[0])
    h1, c1 = lstm_cell(W, 1, h0, h[1], c[1])
    return W["joint.pred.weight"] @ h1 + W["joint.pred.bias"], np.stack([h0, h1]), np.stack([c0, c1])


def logits(W, encp_t, pp):
    return W["joint.joint_net.weight"] @ np.maximum(encp_t + pp, 0) + W["joint.joint_net.bias"]


def tdt_decode(W32, encp, vocab, durations, max_symbols, cap, dtype=np.float64, follow=None):
    """The kernel's loop on projected frames encp [T, J]: the proposal is computed once per emission.  -> dict(tokens, frames, durations,
    flag, steps, gap, logits).  gap: the smallest top-2 gap of either arg-max over all steps.  follow: the decisions (token, duration
    index) of another run to take instead of the own arg-max (the float32 run follows the float64 one, so that their logits pair up)."""
    W = {k: v.astype(dtype) for k, v in W32.items()}
    encp = np.asarray(encp, dtype)
    blank, P, T = vocab, W["joint.pred.weight"].shape[1], encp.shape[0]
    h, c = np.zeros((2, P), dtype), np.zeros((2, P), dtype)
    pp, hn, cn = predict(W, blank, blank, h, c)
    out = dict(tokens=[], frames=[], durations=[], flag=0, steps=0, gap=np.inf, logits=[], decisions=[])
    t = ns = 0
    while t < T:
        lg = logits(W, encp[t], pp)
        out["logits"].append(lg)
        for part in (lg[:vocab + 1], lg[vocab + 1:]):
            top = np.sort(part)[::-1]
            if len(top) > 1:
                out["gap"] = min(out["gap"], float(top[0] - top[1]))
        tok, di = (int(np.argmax(lg[:vocab + 1])), int(np.argmax(lg[vocab + 1:]))) if follow is None else follow[out["steps"]]
        out["decisions"].append((tok, di))
        out["steps"] += 1
        jump = durations[di]
        if tok != blank:
            if len(out["tokens"]) >= cap:
                out["flag"] = 1
                break
            out["tokens"].append(tok); out["frames"].append(t); out["durations"].append(jump)
            h, c = hn, cn
            pp, hn, cn = predict(W, tok, blank, h, c)
        t += jump
        ns += 1
        if jump != 0:
            ns = 0
        elif ns >= max_symbols:
            t += 1
            ns = 0
    return out


def literal_tdt(W32, encp, vocab, durations, max_symbols):
    """decodeTDTSerial (ParakeetModel.swift:389-479) with makeCompiledTDTStep (:894-931) and NemoDecodingLogic.tdtStep (:41-67), one
    statement at a time, float64: the prediction network runs at EVERY step from the committed state."""
    W = {k: v.astype(np.float64) for k, v in W32.items()}
    encp = np.asarray(encp, np.float64)
    blank_token = vocab
    last_token, hypothesis = blank_token, []
    t, new_symbols = 0, 0
    P = W["joint.pred.weight"].shape[1]
    state = (np.zeros((2, P)), np.zeros((2, P)))
    while t < encp.shape[0]:
        pred, hidden, cell = predict(W, last_token, blank_token, state[0], state[1])
        joint_out = logits(W, encp[t], pred)
        token = int(np.argmax(joint_out[:blank_token + 1]))
        decision_index = int(np.argmax(joint_out[blank_token + 1:]))
        jump = durations[decision_index] if 0 <= decision_index < len(durations) else 1
        next_time = t + jump
        next_new_symbols = new_symbols + 1
        if jump != 0:
            next_new_symbols = 0
        elif max_symbols is not None and next_new_symbols >= max_symbols:
            next_time += 1
            next_new_symbols = 0
        if token != blank_token:
            last_token = token
            state = (hidden, cell)
            hypothesis.append((token, t, jump))
        t = next_time
        new_symbols = next_new_symbols
    return hypothesis


# ---------------------------------------------------------------------------------------------------- the decode cases of both test files
TDT = dict(P=32, J=32, vocab=40, max_symbols=3, cap=20, Tp=24)
TDT_SEED = 7                       # chosen on the CPU: test_parakeet_cpu.test_decision_margin holds the margin it must keep


def tdt_cases():
    """-> (W, rows): W the shared decoder; rows = [(name, encp [Tp, J] float32 with NaN junk behind T, T, joint_net bias override)].  Every
    case reaches its arg-max through an output bias: the bias of joint_net differs per case, so each case is its own launch."""
    c = TDT
    W = make_decoder(TDT_SEED, c["P"], c["J"], c["vocab"])
    rng = np.random.default_rng(TDT_SEED + 100)
    V, D = c["vocab"] + 1, len(DURATIONS)

    def row(T):
        e = np.full((c["Tp"], c["J"]), np.nan, np.float32)
        e[:T] = rng.uniform(-1.5, 1.5, (T, c["J"])).astype(np.float32)
        return e, T

    def bias(tok=None, dur=None, amp=60.0):
        b = W["joint.joint_net.bias"].copy()
        if tok is not None:
            b[tok] += amp
        if dur is not None:
            b[V + dur] += amp
        return b

    return W, [("one_frame", *row(1), None), ("ragged_a", *row(7), None), ("ragged_b", *row(19), None), ("full", *row(c["Tp"]), None),
               ("duration_0_always", *row(5), bias(tok=3, dur=0)), ("blank_duration_0", *row(6), bias(tok=c["vocab"], dur=0)),
               ("jump_past_end", *row(3), bias(dur=4)), ("all_blank", *row(9), bias(tok=c["vocab"])),
               ("capacity", *row(c["Tp"]), bias(tok=7, dur=1))]
