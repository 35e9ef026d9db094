"""-m gpu: Canary (csrc/canary.hip) through the C ABI against tests/canary_ref.py, which test_canary_cpu.py holds to torch's modules and to
the reference's whole-prefix form.

Gate of the float comparisons: relative rms distance of the device to the float64 specification <= 4 x the float32 specification's own
distance to the float64 one, + 2^-23.  Every stage is compared with the specification run on the device's own previous stage.  Tokens are
compared for equality, no row exempt: test_canary_cpu.test_decision_margin holds the margin that allows it.
MIS_CANARY_PARITY_LOG=<file> keeps every observed value (profiles/canary/parity_observed.jsonl)."""
import functools
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
import parakeet_ref as P
import sortformer_ref as R
from gpu_util import observe, rms

pytestmark = pytest.mark.gpu
KEYS = (1, 31, 33, 64, 65, 129, 257)
SECONDS = (0.3, 1.0, 2.5)


def _gate(kind, dev, ref64, ref32):
    rel = lambda a, b: rms(a, np.asarray(b, np.float64)) / max(float(np.sqrt(np.mean(np.asarray(b, np.float64) ** 2))), 1e-30)
    value, tol = rel(dev, ref64), 4.0 * rel(ref32, ref64) + 2.0 ** -23
    name = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].split("::")[-1]
    if os.environ.get("MIS_CANARY_PARITY_LOG"):
        with open(os.environ["MIS_CANARY_PARITY_LOG"], "a") as f:
            f.write(json.dumps(dict(test=name, kind=kind, value=float(value), tol=float(tol))) + "\n")
    print(f"{name} {kind}: {value:.3e} (tol {tol:.3e})")
    return observe(kind, value, tol)


def _ptr(a):
    return a.ctypes.data


def _lin(X, M, W, bias, S, relu=0):
    out = np.zeros((M, W.shape[0]), np.float32)
    check(mas._lib.lib().mis_debug_canary_lin(0, _ptr(X), X.shape[0], M, W.shape[1], W.shape[0], _ptr(W), _ptr(bias), relu, S, _ptr(out)))
    return out


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("K,N", [(144, 144), (256, 1024)])
@pytest.mark.parametrize("M", [1, 31, 33, 64])
def test_lin_kernel(M, K, N, S):
    rng = np.random.default_rng(1000 * M + K + S)
    X = np.full((64, K), np.nan, np.float32)                               # NaN stands in the rows beyond M
    X[:M] = rng.standard_normal((M, K)).astype(np.float32)
    W, bias = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    out = _lin(X, M, W, bias, S, relu=int(S == 1))
    ref = lambda dt: (lambda y: torch.relu(y) if S == 1 else y)(torch.as_tensor(X[:M]).to(dt) @ torch.as_tensor(W).to(dt).T + torch.as_tensor(bias).to(dt)).numpy()
    assert _gate(f"lin M {M} K {K} N {N} S {S}", out, ref(torch.float64), ref(torch.float32))
    r = M // 2
    alone = _lin(np.ascontiguousarray(X[r:r + 1]), 1, W, bias, S, relu=int(S == 1))
    assert np.array_equal(alone[0].view(np.uint32), out[r].view(np.uint32))    # a row alone and inside the batch: the same bits


@pytest.mark.parametrize("hd", [64, 72, 128])
def test_attn_step_kernel(hd):
    H, B, cap = 2, len(KEYS), max(KEYS)
    rng = np.random.default_rng(hd)
    q = rng.standard_normal((B, H * hd)).astype(np.float32)
    kv = np.full((B, cap, 2 * H * hd), np.nan, np.float32)                 # NaN stands behind each count
    for b, n in enumerate(KEYS):
        kv[b, :n] = rng.standard_normal((n, 2 * H * hd)).astype(np.float32)
    cnt, out = np.asarray(KEYS, np.int32), np.zeros((B, H * hd), np.float32)
    check(mas._lib.lib().mis_debug_canary_attn_step(0, _ptr(q), _ptr(kv), _ptr(cnt), B, cap, H, hd, _ptr(out)))

    def ref(b, n, dt):
        t = lambda a: torch.as_tensor(a).to(dt)
        qq, k, v = t(q[b]).reshape(H, 1, hd), t(kv[b, :n, :H * hd]).reshape(n, H, hd).transpose(0, 1), t(kv[b, :n, H * hd:]).reshape(n, H, hd).transpose(0, 1)
        return (torch.softmax(qq @ k.transpose(1, 2) * hd ** -0.5, -1) @ v).reshape(H * hd).numpy()

    assert all([_gate(f"attn step hd {hd} keys {n}", out[b], ref(b, n, torch.float64), ref(b, n, torch.float32)) for b, n in enumerate(KEYS)])


def test_head_argmax_ties_go_to_the_lower_index():
    M, K, V = 5, 96, 203
    rng = np.random.default_rng(9)
    xn = rng.standard_normal((M, K)).astype(np.float32)
    W, bias = (rng.standard_normal((V, K)) / np.sqrt(K)).astype(np.float32), np.zeros(V, np.float32)
    W[[40, 45, 70, 150]] *= 0.0                                            # two pairs of equal rows: one inside a tile, one across tiles
    bias[[40, 45]] = 50.0
    logits, idx, val = np.zeros((M, V), np.float32), np.zeros(M, np.int32), np.zeros(M, np.float32)
    check(mas._lib.lib().mis_debug_canary_head_argmax(0, _ptr(xn), M, K, V, _ptr(W), _ptr(bias), _ptr(logits), _ptr(idx), _ptr(val)))
    assert idx.tolist() == [40] * M == np.argmax(logits.astype(np.float64), axis=1).tolist()
    bias[[40, 45]] = 0.0
    bias[[70, 150]] = 50.0
    check(mas._lib.lib().mis_debug_canary_head_argmax(0, _ptr(xn), M, K, V, _ptr(W), _ptr(bias), _ptr(logits), _ptr(idx), _ptr(val)))
    assert idx.tolist() == [70] * M == np.argmax(logits.astype(np.float64), axis=1).tolist() and np.array_equal(val, logits[np.arange(M), idx])
    bias[:] = rng.standard_normal(V).astype(np.float32)
    idx2 = np.zeros(M, np.int32)
    check(mas._lib.lib().mis_debug_canary_head_argmax(0, _ptr(xn), M, K, V, _ptr(W), _ptr(bias), _ptr(logits), _ptr(idx), None))
    check(mas._lib.lib().mis_debug_canary_head_argmax(0, _ptr(xn), M, K, V, _ptr(W), _ptr(bias), None, _ptr(idx2), None))
    assert idx.tolist() == idx2.tolist() == np.argmax(logits.astype(np.float64), axis=1).tolist()
    r = lambda dt: (torch.as_tensor(xn).to(dt) @ torch.as_tensor(W).to(dt).T + torch.as_tensor(bias).to(dt)).numpy()
    assert _gate("head logits", logits, r(torch.float64), r(torch.float32))


@functools.lru_cache(maxsize=None)
def _model(h, heads, case):
    cfg = CR.case_config(h, heads)
    W = CR.make_weights(cfg, 31)
    W["decoder.output_proj.bias"] = CR.decode_cases(W, cfg.vocab_size)[case]
    return cfg, W, mas.CanaryModel.from_weights(cfg, W)


@functools.lru_cache(maxsize=None)
def _waves():
    return tuple(R.test_wave(50 + i, int(16000 * s) + 37 * i) for i, s in enumerate(SECONDS))


def _tokens(raws):
    return [r["tokens"].tolist() for r in raws]


@pytest.mark.parametrize("h,heads", [(256, 4), (144, 2)])
def test_end_to_end_stages_tokens_batch_invariance_and_launches(h, heads):
    cfg, W, m = _model(h, heads, "plain")
    waves, Le, Ld, prompts = list(_waves()), cfg.encoder.n_layers, cfg.decoder.num_layers, [list(p) for p in CR.PROMPTS]
    batch = m.decode_raw(waves, prompts, CR.EOS, CR.MAX_TOKENS)
    assert m.last_steps % 8 == 0 or m.last_steps == max(map(len, prompts)) + CR.MAX_TOKENS
    assert m.launches == m.expected_launches(m.last_steps)["generate"] == 7 + 15 * Le + Ld + 1 + m.last_steps * (11 * Ld + 2)
    taps = [m.tap(s) for s in range(Le + 2 + Ld)]
    logits, hidden = m.forward(prompts)
    _, T = m.frames([len(w) for w in waves])
    ev = CR.encoder_view(cfg)
    r64, r32 = P.Encoder(ev, W, torch.float64), P.Encoder(ev, W, torch.float32)
    d64, d32 = CR.Decoder(W, heads, torch.float64), CR.Decoder(W, heads, torch.float32)
    ok = True
    for b, w in enumerate(waves):
        n = int(T[b])
        ok &= _gate(f"row {b} stem", taps[0][b, :n], r64.pre_encode(r64.features(w)).numpy(), r32.pre_encode(r32.features(w)).numpy())
        for s in range(1, Le + 1):
            ok &= _gate(f"row {b} stage {s}", taps[s][b, :n], r64.stage_after(s, taps[s - 1][b, :n]).numpy(), r32.stage_after(s, taps[s - 1][b, :n]).numpy())
        assert np.array_equal(taps[Le + 1][b, :n], taps[Le][b, :n]) and not taps[Le + 1][b, n:].any()      # no projection at these widths
        enc = taps[Le + 1][b, :n]
        for l in range(Ld):
            kv = lambda d: torch.cat([d.lin(f"decoder.blocks.{l}.cross_attn.{x}", torch.as_tensor(enc).to(d.dtype)) for x in ("k_proj", "v_proj")], -1).numpy()
            ok &= _gate(f"row {b} cross kv {l}", taps[Le + 2 + l][b, :n], kv(d64), kv(d32))
        f64, f32 = (d.prefix(prompts[b], torch.as_tensor(enc).to(d.dtype)) for d in (d64, d32))
        ok &= _gate(f"row {b} first step hidden", hidden[b], f64[1][-1].numpy(), f32[1][-1].numpy())
        ok &= _gate(f"row {b} first step logits", logits[b], f64[0][-1].numpy(), f32[0][-1].numpy())
        # the decode of the device's own encoder output, by the float64 specification
        assert batch[b]["tokens"].tolist() == d64.generate(prompts[b], torch.as_tensor(enc).to(torch.float64), CR.EOS, CR.MAX_TOKENS)["tokens"]
    assert ok
    enc_all, _ = m.encode(waves)
    assert m.launches == m.expected_launches()["encode"]
    assert all(_tokens(m.decode_raw([w], [prompts[b]], CR.EOS, CR.MAX_TOKENS)) == [batch[b]["tokens"].tolist()] for b, w in enumerate(waves))
    assert _tokens(m.decode_raw(waves, prompts, CR.EOS, CR.MAX_TOKENS, junk=np.nan)) == _tokens(batch)
    for b, w in enumerate(waves):
        alone, _ = m.encode([w])
        assert np.array_equal(alone[0].view(np.uint32), enc_all[b, :alone.shape[1]].view(np.uint32))


@pytest.mark.parametrize("case", ["eos_first", "eos_ragged"])
@pytest.mark.parametrize("h,heads", [(256, 4), (144, 2)])
def test_eos_cases_equal_the_specification(h, heads, case):
    cfg, W, m = _model(h, heads, case)
    waves, prompts = list(_waves()), [list(p) for p in CR.PROMPTS]
    got = m.decode_raw(waves, prompts, CR.EOS, CR.MAX_TOKENS)
    enc, d64 = m.tap(cfg.encoder.n_layers + 1), CR.Decoder(W, heads, torch.float64)
    _, T = m.frames([len(w) for w in waves])
    want = [d64.generate(prompts[b], torch.as_tensor(enc[b, :int(T[b])]).to(torch.float64), CR.EOS, CR.MAX_TOKENS)["tokens"] for b in range(3)]
    assert _tokens(got) == want and not any(r["truncated"] for r in got)
    if case == "eos_first":
        assert want == [[], [], []]
    else:
        assert len({len(t) for t in want}) > 1


def test_graph_and_plain_launches_give_the_same_tokens():
    _, _, m = _model(144, 2, "eos_ragged")
    prompts = [list(p) for p in CR.PROMPTS]
    with_graph = _tokens(m.decode_raw(list(_waves()), prompts, CR.EOS, CR.MAX_TOKENS))
    code = ("import sys, json; sys.path.insert(0, 'tests'); import test_gpu_canary as t, canary_ref as CR; m = t._model(144, 2, 'eos_ragged')[2]; "
            "print(json.dumps(t._tokens(m.decode_raw(list(t._waves()), [list(p) for p in CR.PROMPTS], CR.EOS, CR.MAX_TOKENS))))")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, MIS_NO_GRAPH="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == with_graph


def test_refusals():
    with pytest.raises(mas.AudioGenerationError, match="max_seconds"):
        mas.CanaryModel(mas.CanaryConfig(max_batch=64, max_seconds=120))
    cfg, W, m = _model(144, 2, "plain")
    with pytest.raises(mas.AudioGenerationError, match="max_seconds"):
        m.decode_raw([np.zeros(16000 * cfg.max_seconds + 1, np.float32)], [[0, 1, 2]], CR.EOS)
    with pytest.raises(mas.AudioGenerationError, match="temperature"):
        m.generate(_waves()[0], temperature=0.7)
    with pytest.raises(mas.AudioGenerationError, match="beam"):
        m.generate(_waves()[0], beam_size=4)
    out = m.generate(_waves()[0], max_tokens=4)                            # the handle is still usable; no tokenizer: ids 0, 1, 2 and <id> text
    assert out.prompt_tokens == 3 and out.generation_tokens == 4 and out.segments == [dict(text=out.text, start=0.0, end=0.0)]
