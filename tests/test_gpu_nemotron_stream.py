"""-m gpu: the Nemotron cache-aware stream session (csrc/nemotron_stream.hip).  The yardsticks are the offline engine (bit equality) and
tests/nemotron_ref.py in float64 under test_gpu_nemotron._gate: with left % C == 0, a causal conv and NA normalisation the offline
specification is the stream's."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
from mlx_audio_swift_amd.generation import check
import nemotron_ref as N
import sortformer_ref as R
from test_gpu_nemotron import _gate, _ptr

pytestmark = pytest.mark.gpu
CONTEXTS = [(56, 13), (4, 1), (3, 0)]
LANGS = ["de-DE", "en-US", "de-DE", "auto"]
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("ctx", CONTEXTS)
@pytest.mark.parametrize("hd", [128, 96])
def test_attention_kernel_over_a_wrapped_ring(hd, ctx):
    """streams at absolute positions behind two and more wraps of the ring, one whose 32-query tile straddles the wrap; passes of 1, C and
    3 C frames; every ring row outside the visible range holds 1e30.  Against float64 and, bit for bit, against k_nm_attn on the same
    rows laid out contiguously."""
    H, w, (left, right) = 2, 2 * hd, ctx
    Cs = right + 1
    Tp = 3 * Cs
    Rr = (left + Tp + 32 + 31) // 32 * 32
    sizes = [1, Cs, 3 * Cs, 3 * Cs]
    pos = [2 * Rr + 5, (3 * Rr + Cs) // Cs * Cs, 2 * Rr - 1, (4 * Rr - Tp // 2) // Cs * Cs]     # the last: its queries straddle the wrap
    Tcap, S = max(p + n for p, n in zip(pos, sizes)), len(sizes)
    rng = np.random.default_rng(hd + right)
    table = rng.standard_normal((2 * Tcap - 1, w)).astype(np.float32)
    u, v = (rng.uniform(-0.5, 0.5, (H, hd)).astype(np.float32) for _ in range(2))
    full = np.zeros((S, Tcap, 3 * w), np.float32)
    q, ring = np.full((S, Tp, w), np.nan, np.float32), np.full((S, Rr, 2 * w), 1e30, np.float32)
    for b, (p, n) in enumerate(zip(pos, sizes)):
        full[b, :p + n] = rng.standard_normal((p + n, 3 * w)).astype(np.float32)
        q[b, :n] = full[b, p:p + n, :w]
        for key in range(max(p // Cs * Cs - left, 0), p + n):
            ring[b, key % Rr] = full[b, key, w:]
    cnt, ends, at = np.asarray(sizes, np.int32), np.asarray([p + n for p, n in zip(pos, sizes)], np.int32), np.asarray(pos, np.int32)
    out, off = np.zeros((S, Tp, w), np.float32), np.zeros((S, Tcap, w), np.float32)
    lib = mas._lib.lib()
    check(lib.mis_debug_nemotron_attn_stream(0, _ptr(q), _ptr(ring), Rr, _ptr(cnt), _ptr(at), S, Tp, H, hd, 1.0, float(np.sqrt(hd)),
                                             _ptr(u), _ptr(v), _ptr(table), w, 2 * Tcap - 1, Tcap - 1, left, right, _ptr(out), 0, None))
    check(lib.mis_debug_nemotron_attn(0, _ptr(full), 3 * w, w, 2 * w, _ptr(ends), S, Tcap, H, hd, 1.0, float(np.sqrt(hd)), _ptr(u), _ptr(v), _ptr(table), w,
                                      2 * Tcap - 1, Tcap - 1, left, right, Tcap, w, _ptr(off), 0, None))
    ok = True
    for b, (p, n) in enumerate(zip(pos, sizes)):
        assert np.array_equal(bits(out[b, :n]), bits(off[b, p:p + n])), f"stream {b} differs from the offline kernel"
        assert not out[b, n:].any()
        r64, r32 = (N.attention(full[b], table, u, v, p + n, H, hd, Tcap, ctx, dt)[p:] for dt in (torch.float64, torch.float32))
        ok &= _gate(f"attn stream hd {hd} ctx {ctx} pos {p} frames {n}", out[b, :n], r64, r32)
    assert ok


@functools.lru_cache(maxsize=None)
def _model(hidden):
    cfg = N.case_config(hidden, bias=hidden == 256, contexts=CONTEXTS, max_seconds=12)
    W = N.make_weights(cfg, 31)
    return cfg, W, mas.NemotronASR.from_weights(cfg, W)


@functools.lru_cache(maxsize=None)
def _waves():
    """ends on a chunk boundary of (56, 13) (8 x 14 x 10 + 1 mel frames, 141 encoder frames: at one chunk a pass the ring of 128 rows wraps);
    a partial last chunk; shorter than a chunk; shorter than n_fft / 2 samples"""
    return tuple(R.test_wave(60 + i, n) for i, n in enumerate((160 * 8 * 14 * 10 + 3, 16000 * 2 + 411, 160 * 8 * 5, 200)))


@functools.lru_cache(maxsize=None)
def _offline(hidden, ctx):
    cfg, W, m = _model(hidden)
    raw = m.decode_raw(list(_waves()), LANGS, ctx)
    taps = [m.tap(s) for s in range(cfg.num_hidden_layers + 3)]
    _, T = m.frames([len(w) for w in _waves()])
    return raw, taps, T


def _feeds(pattern, waves):
    """-> the feeds [[chunk of stream b]]; the final bits go with a last, empty feed"""
    if pattern == "whole":
        return [list(waves)]
    cuts = [1280] * 200 if pattern == "80ms" else [0, 1, 255, 1, 3000, 0, 17, 40000, 1279, 1281] * 20
    at, out = [0] * len(waves), []
    for c in cuts:
        out.append([w[a:a + c] for w, a in zip(waves, at)])
        at = [a + c for a in at]
        if all(a >= len(w) for w, a in zip(waves, at)):
            break
    return out


def _run(sess, feeds, stages):
    got = [[[] for _ in range(sess.streams)] for _ in range(stages)]
    for chunks, fin in [(f, None) for f in feeds] + [([None] * sess.streams, [True] * sess.streams)]:
        sess.step_batch(chunks, fin)
        assert sess.launches == sess.expected_launches, "launches of a feed: passes x (9 + 16 L + 2 p), 0 without a whole chunk"
        for s in range(stages):
            for b, x in enumerate(sess.tap(s)):
                got[s][b].append(x)
    return [[np.concatenate(x) for x in row] for row in got]


@pytest.mark.parametrize("pattern", ["80ms", "ragged", "whole"])
@pytest.mark.parametrize("ctx", CONTEXTS)
@pytest.mark.parametrize("hidden", [256, 192])
def test_stream_equals_offline(hidden, ctx, pattern):
    cfg, W, m = _model(hidden)
    L, waves = cfg.num_hidden_layers, _waves()
    raw, taps, T = _offline(hidden, ctx)
    sess = mas.NemotronStreamSession(m, 4, LANGS, att_context_size=ctx, max_pass_frames=None if pattern == "whole" else ctx[1] + 1)
    sess.enable_taps(int(T.max()) + 2)
    got = _run(sess, _feeds(pattern, waves), L + 3)
    for b in range(4):
        n = int(T[b])
        for s in range(L + 3):
            assert got[s][b].shape[0] == n and np.array_equal(bits(got[s][b]), bits(taps[s][b, :n])), f"stream {b} stage {s} differs from offline"
        mine = sess.raw(b)
        assert mine["tokens"].tolist() == raw[b]["tokens"].tolist() and mine["frames"].tolist() == raw[b]["frames"].tolist()
        assert sess.frames_seen(b) == n
    r64, r32 = N.Encoder(cfg, W, torch.float64, ctx), N.Encoder(cfg, W, torch.float32, ctx)
    assert all([_gate(f"stream ctx {ctx} row {b} last block", got[L][b], r64.stage_after(L, got[L - 1][b], 0).numpy(), r32.stage_after(L, got[L - 1][b], 0).numpy())
                for b in range(4)])
    sess.close()


def _pass(Wc, layers, ms, cap, e, pos, tok0, state, ist):
    c = N.RNNT
    lstm = lambda n: (C.c_void_p * layers)(*[_ptr(Wc[f"decoder.prediction.dec_rnn.lstm.{n}_l{l}"]) for l in range(layers)])
    e = np.ascontiguousarray(e[None], np.float32)
    tok, frm = (np.full((1, cap), -1, np.int32) for _ in range(2))
    cnt, at, t0 = (np.asarray([x], np.int32) for x in (e.shape[1], pos, tok0))
    check(mas._lib.lib().mis_debug_nemotron_rnnt_stream(0, _ptr(e), _ptr(cnt), _ptr(at), _ptr(t0), 1, e.shape[1], c["J"], c["P"], c["vocab"],
                                                        layers, ms or 0, cap, _ptr(Wc["decoder.prediction.embed.weight"]), lstm("weight_ih"), lstm("weight_hh"),
                                                        lstm("bias_ih"), lstm("bias_hh"), _ptr(Wc["joint.pred.weight"]), _ptr(Wc["joint.pred.bias"]),
                                                        _ptr(Wc["joint.joint_net.weight"]), _ptr(Wc["joint.joint_net.bias"]), _ptr(state), _ptr(ist), _ptr(tok),
                                                        _ptr(frm)))
    return tok[0], frm[0]


@pytest.mark.parametrize("layers", [1, 2])
def test_decode_kernel_resumes_at_every_cut(layers):
    """every cut of the short row, a few of the others; always_emit is cut right behind its max_symbols-forced advances; all_blank gives
    passes of blanks alone; no_max_symbols_capacity reaches the capacity in its first pass and ignores the rest"""
    c = N.RNNT
    W, rows = N.rnnt_cases(layers)
    for name, e, T, bias, ms in rows:
        Wc = dict(W, **({"joint.joint_net.bias": bias} if bias is not None else {}))
        ref = N.rnnt_decode(Wc, e[:T], c["vocab"], ms, c["cap"])
        for cuts in ([[k] for k in range(T + 1)] if T <= 7 else [[1], [T // 2], [3, 4, T - 1]]):
            state, ist, toks, frms = np.zeros((1, 4 * c["P"] + c["J"]), np.float32), np.zeros((1, 4), np.int32), [], []
            for a, b in zip([0] + cuts, cuts + [T]):
                if a == b:
                    continue
                before = int(ist[0, 1])
                tok, frm = _pass(Wc, layers, ms, c["cap"], e[a:b], a, before, state, ist)
                k = int(ist[0, 1]) - before
                toks += tok[:k].tolist(); frms += frm[:k].tolist()
                assert (tok[k:] == -1).all()
            assert (toks, frms, int(ist[0, 1]), int(ist[0, 2]), int(ist[0, 3])) == (ref["tokens"], ref["frames"], len(ref["tokens"]), ref["flag"], ref["steps"]), (name, cuts)


def test_slot_independence_reset_launches_and_refusals():
    """joint.enc and the last block, bit for bit, and the tokens: slot 0 alone = slot 3 among busy neighbours while one of them is reset
    mid-stream = slot 3 again after a reset that follows that utterance.  Every feed's launches equal the formula."""
    cfg, W, m = _model(256)
    w, other = _waves()[1], _waves()[0][:40000]
    L = cfg.num_hidden_layers
    per_pass = 9 + 16 * L + 2

    def run(sess, slot, neighbours, reset_at=None):
        taps, passes = [[], []], 0
        feeds = [(at, False) for at in range(0, len(w), 4000)] + [(None, True)]
        for i, (at, fin) in enumerate(feeds):
            chunks = [None if fin or not neighbours else other[at:at + 4000]] * sess.streams
            chunks[slot] = None if fin else w[at:at + 4000]
            sess.step_batch(chunks, [fin and b == slot for b in range(sess.streams)])
            assert sess.launches == sess.expected_launches and sess.launches % per_pass == 0
            passes += sess.launches // per_pass
            for k, stage in enumerate((L, L + 2)):
                taps[k].append(sess.tap(stage)[slot])
            if reset_at == i:
                sess.reset(0)
        assert sess.finish(slot) == mas.Delta() and passes >= len(feeds) - 2
        return sess.raw(slot), [np.concatenate(t) for t in taps]

    one = mas.NemotronStreamSession(m, 1, "de-DE", att_context_size=(4, 1))
    one.enable_taps(64)
    one.step_batch([w[:100]])
    assert one.launches == 0 == one.expected_launches                   # no whole chunk yet
    one.reset(0, "de-DE")
    alone, taps_alone = run(one, 0, False)
    off = m.decode_raw([w], "de-DE", (4, 1))[0]
    assert alone["tokens"].tolist() == off["tokens"].tolist() and alone["frames"].tolist() == off["frames"].tolist() and len(off["tokens"]) > 0
    assert np.array_equal(bits(taps_alone[1]), bits(m.tap(L + 2)[0]))
    four = mas.NemotronStreamSession(m, 4, ["en-US", "en-US", "auto", "de-DE"], att_context_size=(4, 1))
    four.enable_taps(64)
    busy = run(four, 3, True, reset_at=2)                                   # a neighbour is reset mid-stream
    four.reset(3, "de-DE")                                                 # the slot again, behind another utterance
    again = run(four, 3, True)
    for r, taps in (busy, again):
        assert r["tokens"].tolist() == alone["tokens"].tolist() and r["frames"].tolist() == alone["frames"].tolist()
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(taps, taps_alone))
    one.close(); four.close()
    for kwargs, msg in ((dict(att_context_size=(5, 1)), "left"), (dict(att_context_size=(56, 27)), "listed contexts"), (dict(streams=65), "streams")):
        with pytest.raises(mas.AudioGenerationError, match=msg):
            mas.NemotronStreamSession(m, **kwargs)
    for kw, msg in ((dict(normalize="per_feature"), "NA mel normalization"), (dict(conv=(5, 3)), "causal pad")):
        norm = kw.pop("normalize", "NA")
        c2 = N.case_config(256, **kw)
        c2.normalize = norm
        m2 = mas.NemotronASR.from_weights(c2, N.make_weights(c2, 31))
        with pytest.raises(mas.AudioGenerationError, match=msg):
            mas.NemotronStreamSession(m2)
        m2.close()
