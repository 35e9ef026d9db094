"""-m gpu: the bf16 form of Canary's decoder (csrc/canary.hip: k_cn_lin_bf16, k_cn_attn_step_bf16; contract in mi_speech.h): the two
kernels through the debug entry points and the chain through CanaryModel with decoder_dtype="bfloat16".  References are float64 torch;
the rounded specification is canary_ref.Decoder with the contract's roundings.  Distances are relative rms; each gate's reasoning stands at
the gate.  MIS_CANARY_BF16_PARITY_LOG=<file> keeps every observed value (profiles/canary_bf16/parity_observed.jsonl)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
from mlx_audio_swift_amd.generation import check
import canary_ref as CR
import sortformer_ref as R

pytestmark = pytest.mark.gpu
F64, BF = torch.float64, torch.bfloat16
KEYS = (1, 31, 33, 64, 65, 129, 257)
SEED = 31            # make_weights seed: on the float64 encoder output the rounded specification alone exempts 1, 1, 0 of the 18 decisions of the chain cases
_ptr = lambda a: None if a is None else a.ctypes.data
_rb = lambda t: t.to(BF).to(F64)
_bits = lambda t: t.to(BF).contiguous().view(torch.int16).numpy().view(np.uint16)
_f32 = lambda t: np.ascontiguousarray(t.to(torch.float32).numpy())


def _rel(a, b):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    return float(torch.sqrt(torch.mean((a - b) ** 2)) / max(float(torch.sqrt(torch.mean(b ** 2))), 1e-30))


def _gate(kind, value, tol):
    name = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].split("::")[-1]
    if os.environ.get("MIS_CANARY_BF16_PARITY_LOG"):
        with open(os.environ["MIS_CANARY_BF16_PARITY_LOG"], "a") as f:
            f.write(json.dumps(dict(test=name, kind=kind, value=float(value), tol=float(tol))) + "\n")
    print(f"{name} {kind}: {value:.3e} (tol {tol:.3e})")
    return value <= tol


def _lin(x, M, w, bias, S=1, relu=0, logits=True, index=False):
    """x f64 [M, K] (NaN rows are appended), w f64 bf16-representable [N, K] -> out f64 [M, N] (, index)"""
    X = np.full((64, x.shape[1]), np.nan, np.float32)
    X[:M] = _f32(x)
    wb, bn = _bits(w), _f32(bias)
    out, idx = (np.zeros((M, w.shape[0]), np.float32) if logits else None), (np.zeros(M, np.int32) if index else None)
    check(mas._lib.lib().mis_debug_canary_lin_bf16(0, _ptr(X), 64, M, x.shape[1], w.shape[0], _ptr(wb), _ptr(bn), relu, S, _ptr(out), _ptr(idx)))
    out = None if out is None else torch.from_numpy(out).to(F64)
    return (out, idx) if index else out


@pytest.mark.parametrize("K,N", [(32, 8), (160, 203), (288, 160), (1024, 1024)])
@pytest.mark.parametrize("M", [1, 15, 17, 33, 64])
def test_contraction(M, K, N):
    g = torch.Generator().manual_seed(1000 * M + K + N)
    grid = lambda *s: torch.randint(-8, 9, s, generator=g).to(F64) / 8            # products and sums of K of them are exact in f32
    x, w, bias = grid(M, K), grid(N, K), grid(N)
    for S in [1] + [s for s in (4, 8) if N <= 4096 and K // 128 >= s]:            # a split only where every split owns a slab
        assert torch.equal(_lin(x, M, w, bias, S), x @ w.T + bias), f"S {S}"      # any fragment, tile, tail or split mistake shows here
    assert torch.equal(_lin(x, M, w, bias, 1, relu=1), torch.relu(x @ w.T + bias))
    # arbitrary f32 x: the device rounds the same x from f32; a flipped tie moves an error from -d to +d ("ln load" of the encoder test)
    xf, wr = (1.5 * torch.randn(M, K, generator=g, dtype=F64) + 0.3).float().to(F64), _rb(torch.randn(N, K, generator=g, dtype=F64) / K ** 0.5)
    exact, rounded = xf @ wr.T + bias, _rb(xf) @ wr.T + bias
    assert _gate("f32 x", _rel(_lin(xf, M, wr, bias), exact), 2 * _rel(rounded, exact) + 2.0 ** -23)


@pytest.mark.parametrize("M", [1, 17, 64])
def test_head_ties_go_to_the_lower_index(M):
    K, V = 160, 203
    g = torch.Generator().manual_seed(M)
    x, w = (torch.randint(-8, 9, s, generator=g).to(F64) / 8 for s in ((M, K), (V, K)))
    w[[40, 45, 70, 150]] = 0.0
    for rows in ((40, 45), (70, 150)):                                            # equal maxima inside one tile, then across tiles
        bias = torch.zeros(V, dtype=F64)
        bias[list(rows)] = 200.0
        logits, idx = _lin(x, M, w, bias, index=True)
        assert idx.tolist() == [rows[0]] * M and torch.equal(logits, x @ w.T + bias)
        assert _lin(x, M, w, bias, logits=False, index=True)[1].tolist() == [rows[0]] * M


@pytest.mark.parametrize("hd", [64, 80, 128])
def test_attn_step(hd):
    H, B, cap = 2, len(KEYS), max(KEYS)
    g = torch.Generator().manual_seed(hd)
    q = torch.randn(B, H * hd, generator=g).to(F64)
    kv = torch.full((B, cap, 2 * H * hd), float("nan"), dtype=F64)                # NaN stands behind each count
    for b, n in enumerate(KEYS):
        kv[b, :n] = _rb(torch.randn(n, 2 * H * hd, generator=g, dtype=F64))
    qn, kb, cnt, out = _f32(q), _bits(kv), np.asarray(KEYS, np.int32), np.zeros((B, H * hd), np.float32)
    check(mas._lib.lib().mis_debug_canary_attn_step_bf16(0, _ptr(qn), _ptr(kb), _ptr(cnt), B, cap, H, hd, _ptr(out)))

    def ref(b, n, dt):
        qq, k, v = q[b].to(dt).reshape(H, 1, hd), *(kv[b, :n, i * H * hd:(i + 1) * H * hd].to(dt).reshape(n, H, hd).transpose(0, 1) for i in range(2))
        return (torch.softmax(qq @ k.transpose(1, 2) * hd ** -0.5, -1) @ v).reshape(H * hd)

    # the kernel rounds nothing: only f32 arithmetic separates it from float64, as the float32 reference
    assert all([_gate(f"hd {hd} keys {n}", _rel(out[b], ref(b, n, F64)), 4 * _rel(ref(b, n, torch.float32), ref(b, n, F64)) + 2.0 ** -23) for b, n in enumerate(KEYS)])


class RoundedDecoder(CR.Decoder):
    """float64 with the contract's roundings: the step matrices and the head pre-rounded, x rounded in lin, K and V rounded behind their
    projections.  The cross k | v projection itself is the f32 GEMM of the unrounded encoder output: matrix and input stay as they are."""
    def __init__(self, W, heads):
        cross = lambda k: ".cross_attn.k_proj" in k or ".cross_attn.v_proj" in k
        step = lambda k, v: k.endswith(".weight") and v.ndim == 2 and (k.startswith("decoder.blocks.") and not cross(k) or k.startswith("decoder.output_proj"))
        super().__init__({k: torch.as_tensor(v).to(BF).float().numpy() if step(k, v) else v for k, v in W.items()}, heads, F64)

    def lin(self, p, x):
        y = super().lin(p, x if ".cross_attn.k_proj" in p or ".cross_attn.v_proj" in p else _rb(x))
        return _rb(y) if p.endswith(("k_proj", "v_proj")) else y


def _case(h, heads):
    cfg = CR.case_config(h, heads)
    W = CR.make_weights(cfg, SEED)
    W["decoder.output_proj.bias"] = CR.decode_cases(W, cfg.vocab_size)["plain"]
    waves = [R.test_wave(40 + i, int(16000 * s) + 37 * i) for i, s in enumerate((0.3, 1.0, 2.5))]
    return cfg, W, waves, [list(p) for p in CR.PROMPTS]


_tokens = lambda raws: [r["tokens"].tolist() for r in raws]


@pytest.mark.parametrize("h,heads", [(256, 4), (160, 2), (256, 2)])
def test_chain(h, heads):
    cfg, W, waves, prompts = _case(h, heads)
    Le, Ld = cfg.encoder.n_layers, cfg.decoder.num_layers
    m, f32 = mas.CanaryModel.from_weights(cfg, W, decoder_dtype="bfloat16"), mas.CanaryModel.from_weights(cfg, W)
    batch = m.decode_raw(waves, prompts, CR.EOS, CR.MAX_TOKENS)
    assert m.launches == m.expected_launches(m.last_steps)["generate"] == 7 + 15 * Le + 2 * Ld + 1 + m.last_steps * (11 * Ld + 2)
    logits, hidden = m.forward(prompts)
    enc, ckv, T = m.tap(Le + 1), m.tap(Le + 2), m.frames([len(w) for w in waves])[1]
    assert np.array_equal(ckv, torch.from_numpy(ckv).to(BF).float().numpy())        # the tap is the widened store
    exact, spec, ok, exempt, total = CR.Decoder(W, heads, F64), RoundedDecoder(W, heads), True, 0, 0
    for b in range(len(waves)):
        e = torch.as_tensor(enc[b, :int(T[b])]).to(F64)
        kv = torch.cat([spec.lin(f"decoder.blocks.0.cross_attn.{x}", e) for x in ("k_proj", "v_proj")], -1)
        assert _rel(ckv[b, :int(T[b])], kv) <= 2.0 ** -7 and not ckv[b, int(T[b]):].any()      # an f32 projection moves a value by one bf16 step at most
        # <= 4 x D_w + 2^-23, D_w the rounded-matrix specification's distance to the unrounded one (_block_taps_gate of the encoder test)
        for name, dev, i in (("logits", logits[b], 0), ("hidden", hidden[b], 1)):
            s, p = spec.prefix(prompts[b], e)[i][-1], exact.prefix(prompts[b], e)[i][-1]
            ok &= _gate(f"h {h} row {b} {name}", _rel(dev, s), 4 * _rel(s, p) + 2.0 ** -23)
        # every decision is the specification's arg-max unless its top-2 gap is below 8 x the rms logit difference of the two specifications
        toks = batch[b]["tokens"].tolist()
        follow = toks + [CR.EOS] * (CR.MAX_TOKENS - len(toks))
        sr, se = spec.generate(prompts[b], e, CR.EOS, CR.MAX_TOKENS, follow), exact.generate(prompts[b], e, CR.EOS, CR.MAX_TOKENS, follow)
        noise = float(torch.sqrt(torch.mean((torch.stack(sr["logits"]) - torch.stack(se["logits"])) ** 2)))
        for i, lg in enumerate(sr["logits"]):
            top = torch.topk(lg, 2).values
            total += 1
            if float(top[0] - top[1]) < 8 * noise:
                exempt += 1
            else:
                assert int(torch.argmax(lg)) == follow[i], f"row {b} decision {i}"
    assert ok and exempt * 10 <= total, f"{exempt} of {total} decisions exempt"
    # a row alone, in the batch and with NaN junk behind it: the same tokens; the f32 decoder beside it is untouched
    assert all(_tokens(m.decode_raw([w], [prompts[b]], CR.EOS, CR.MAX_TOKENS)) == [batch[b]["tokens"].tolist()] for b, w in enumerate(waves))
    assert _tokens(m.decode_raw(waves, prompts, CR.EOS, CR.MAX_TOKENS, junk=np.nan)) == _tokens(batch)
    got = f32.decode_raw(waves, prompts, CR.EOS, CR.MAX_TOKENS)
    assert f32.launches == f32.expected_launches(f32.last_steps)["generate"] == 7 + 15 * Le + Ld + 1 + f32.last_steps * (11 * Ld + 2)
    e32, d64 = f32.tap(Le + 1), CR.Decoder(W, heads, F64)
    assert _tokens(got) == [d64.generate(prompts[b], torch.as_tensor(e32[b, :int(T[b])]).to(F64), CR.EOS, CR.MAX_TOKENS)["tokens"] for b in range(len(waves))]


def test_plain_launches_give_the_same_tokens():
    cfg, W, waves, prompts = _case(160, 2)
    with_graph = _tokens(mas.CanaryModel.from_weights(cfg, W, decoder_dtype="bfloat16").decode_raw(waves, prompts, CR.EOS, CR.MAX_TOKENS))
    code = ("import sys, json; sys.path.insert(0, 'tests'); import mlx_audio_swift_amd as mas, test_gpu_canary_bf16 as t, canary_ref as CR; "
            "cfg, W, waves, prompts = t._case(160, 2); m = mas.CanaryModel.from_weights(cfg, W, decoder_dtype='bfloat16'); "
            "print(json.dumps(t._tokens(m.decode_raw(waves, prompts, CR.EOS, CR.MAX_TOKENS))))")
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), env=dict(os.environ, MIS_NO_GRAPH="1"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == with_graph


def test_refusals():
    with pytest.raises(mas.AudioGenerationError, match="enc_output_dim"):
        mas.CanaryModel.from_weights(CR.case_config(144, 2), {}, decoder_dtype="bfloat16")
    with pytest.raises(mas.AudioGenerationError, match="decoder_dtype"):
        mas.CanaryModel.from_weights(CR.case_config(256, 4), {}, decoder_dtype="float16")
    cfg, W, waves, prompts = _case(256, 4)
    m = mas.CanaryModel.from_weights(cfg, W)
    with pytest.raises(mas.AudioGenerationError, match="after finalize"):
        m.set_decoder_dtype("bfloat16")
    m.decode_raw(waves[:1], prompts[:1], CR.EOS, CR.MAX_TOKENS)                   # still usable, and still the f32 engine
    assert m.launches == m.expected_launches(m.last_steps)["generate"] == 7 + 15 * 2 + 2 + 1 + m.last_steps * (11 * 2 + 2)
