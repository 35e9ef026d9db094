"""-m gpu: Llama decode-step kernels (packed-weight MFMA GEMMs, fused attention, norms) vs the oracle.

Tolerance (stated): the engine and the oracle both round to bf16 at every MLX primitive boundary but
accumulate in different orders, so individual bf16 roundings may differ by one ulp and propagate.
Teacher-forced logits must satisfy  max|dev - ref| <= 0.016 * max|ref| (two bf16 ulps of the largest logit; observed: one)  and  rms(dev - ref) <=
0.008 * rms(ref), and the greedy token must agree whenever the oracle's top-2 margin exceeds that
error bound."""
import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
from gpu_util import lm_host_config, lm_pair, observe, rms, teacher_forced
from oracle import llama as ollama

pytestmark = pytest.mark.gpu


TOL_MAX, TOL_RMS = 0.016, 0.008          # observed on MI355X (profiles/r03_parity_observed.json): max <= 0.0078, rms <= 0.0069


def _check(pairs):
    for dev_l, ref_l in pairs:
        assert dev_l.shape == ref_l.shape
        scale = float(np.abs(ref_l).max())
        err = float(np.abs(dev_l - ref_l).max())
        assert observe("logits_max_rel", err / scale, TOL_MAX), (err, scale)
        assert observe("logits_rms_rel", rms(dev_l, ref_l) / float(np.sqrt(np.mean(ref_l.astype(np.float64) ** 2))), TOL_RMS)
        # bf16-valued logits
        t = torch.from_numpy(dev_l)
        assert torch.equal(t, t.to(torch.bfloat16).to(torch.float32))
        top2 = np.sort(ref_l, axis=1)[:, -2:]
        margin = top2[:, 1] - top2[:, 0]
        sure = margin > 2 * err
        assert sure.sum() > 0
        assert np.array_equal(dev_l.argmax(1)[sure], ref_l.argmax(1)[sure])


TINY_Q3TTS = ollama.LlamaConfig(**{**ollama.TINY_QWEN3.__dict__, "rope_theta": 1e6, "rope_ops_in_dtype": True, "head_dim": 64,
                                    "num_attention_heads": 8, "num_key_value_heads": 4})


@pytest.mark.parametrize("cfg", [ollama.TINY, ollama.TINY64, ollama.TINY_QWEN3, TINY_Q3TTS],
                         ids=["d128-gqa3", "d64-mha", "qwen3-qknorm", "qwen3tts-rope-ops"])
def test_teacher_forced_logits_match_oracle(cfg):
    W, oracle, dev = lm_pair(cfg)
    rng = np.random.default_rng(1)
    rows = [rng.integers(0, cfg.vocab_size, n).astype(np.int32) for n in (37, 5, 20)]   # ragged, > 32 keys
    _check(teacher_forced(oracle, dev, rows, max_context=64))


def test_untied_lm_head_and_long_context():
    cfg = ollama.LlamaConfig(**{**ollama.TINY.__dict__, "tie_word_embeddings": False, "num_hidden_layers": 1})
    W, oracle, dev = lm_pair(cfg)
    rng = np.random.default_rng(2)
    rows = [rng.integers(0, cfg.vocab_size, 300).astype(np.int32)]                     # 10 key tiles, all 8 waves busy
    pairs = teacher_forced(oracle, dev, rows, max_context=320)
    _check([(pairs[0][0][-40:], pairs[0][1][-40:])])


def test_context_beyond_the_first_tile_pair():
    # > 512 keys: the waves go round their tile loop a second time (in-loop loads), and the tile holding the new key - patched in
    # registers, never read back from the cache - is one of those later tiles
    cfg = ollama.LlamaConfig(**{**ollama.TINY.__dict__, "num_hidden_layers": 1})
    W, oracle, dev = lm_pair(cfg)
    rng = np.random.default_rng(12)
    rows = [rng.integers(0, cfg.vocab_size, 560).astype(np.int32)]                     # 18 key tiles at the end
    pairs = teacher_forced(oracle, dev, rows, max_context=576)
    _check([(pairs[0][0][-48:], pairs[0][1][-48:])])                                   # positions 512..559


@pytest.mark.parametrize("batch", [33, 64], ids=["mt3", "mt4"])
def test_wide_batches(batch):
    # 33 rows -> 3 MFMA column tiles, 64 -> 4 (the widest the weight-streaming GEMM takes)
    cfg = ollama.LlamaConfig(**{**ollama.TINY.__dict__, "num_hidden_layers": 2})
    W, oracle, dev = lm_pair(cfg)
    rng = np.random.default_rng(13)
    rows = [rng.integers(0, cfg.vocab_size, 6).astype(np.int32) for _ in range(batch)]
    pairs = teacher_forced(oracle, dev, rows, max_context=64)
    _check([pairs[0], pairs[batch // 2], pairs[batch - 1]])


def test_batch_row_equals_single_row_bitwise():
    # Tests/ParakeetBatchParityTests.swift pattern: generateBatch(rows)[r] == generate(rows[r])
    cfg = ollama.TINY
    W, oracle, dev = lm_pair(cfg)
    rng = np.random.default_rng(3)
    rows = [rng.integers(0, cfg.vocab_size, 9).astype(np.int32) for _ in range(5)]
    dev.lm_reset(5, 64)
    batch_logits = [dev.lm_forward(np.asarray([r[t] for r in rows], np.int32)) for t in range(9)]
    for r in (0, 4):
        dev.lm_reset(1, 64)
        for t in range(9):
            one = dev.lm_forward(np.asarray([rows[r][t]], np.int32))
            assert np.array_equal(one[0], batch_logits[t][r]), (r, t)
    # 17 rows -> Mpad 32 (two MFMA column tiles): same numbers again
    dev.lm_reset(17, 64)
    rows17 = rows + [rows[0]] * 12
    for t in range(9):
        lg = dev.lm_forward(np.asarray([r[t] for r in rows17], np.int32))
        assert np.array_equal(lg[:5], batch_logits[t])
        assert np.array_equal(lg[16], batch_logits[t][0])


def test_device_synthetic_init_equals_oracle_weights():
    cfg = ollama.TINY
    W, oracle, dev = lm_pair(cfg, seed=4321)
    syn = mas.LlamaTTSModel.synthetic(lm_host_config(cfg), seed=4321)
    ids = np.asarray([3, 999], np.int32)
    dev.lm_reset(2, 64); syn.lm_reset(2, 64)
    for _ in range(3):
        a = dev.lm_forward(ids); b = syn.lm_forward(ids)
        assert np.array_equal(a, b)          # identical weights => identical logits


def test_inactive_rows_do_not_advance_and_errors():
    cfg = ollama.TINY
    W, oracle, dev = lm_pair(cfg)
    dev.lm_reset(2, 64)
    a0 = dev.lm_forward(np.asarray([5, 6], np.int32), np.asarray([1, 0], np.uint8))
    a1 = dev.lm_forward(np.asarray([7, 6], np.int32), np.asarray([1, 1], np.uint8))
    dev.lm_reset(1, 64)
    b = dev.lm_forward(np.asarray([6], np.int32))
    assert np.array_equal(a1[1], b[0])       # row 1 saw token 6 at position 0 exactly once
    with pytest.raises(mas.AudioGenerationError):
        dev.lm_reset(65, 64)
    m = mas.LlamaTTSModel(lm_host_config(cfg))
    with pytest.raises(mas.AudioGenerationError) as e:
        m.finalize()
    assert e.value.case == "modelNotInitialized"
    del a0


def test_hidden_state_tap_matches_oracle():
    # forwardWithHiddenStates (Soprano.swift:254-275): model.norm(h) of the fed token
    cfg = ollama.TINY_QWEN3
    W, oracle, dev = lm_pair(cfg)
    rng = np.random.default_rng(6)
    ids = rng.integers(0, cfg.vocab_size, 12).astype(np.int32)
    dev.lm_reset(1, 64)
    oracle.reset(1)
    for t in range(12):
        lg, hid = dev.lm_forward(ids[t:t + 1], want_hidden=True)
        oracle.forward([ids[t:t + 1]])
        ref = oracle.last_hidden.numpy()[-1]
        assert np.abs(hid[0] - ref).max() <= 0.04 * np.abs(ref).max()


@pytest.mark.parametrize("ocfg", [ollama.TINY, ollama.TINY_QWEN3, ollama.TINY64], ids=["llama3-rope", "qwen3-qknorm", "head64"])
def test_batched_prefill_matches_oracle_and_the_position_by_position_path(ocfg, monkeypatch):
    """`model(inputIds, cache:)` (LlamaTTS.swift:711): the prompt as one [positions x rows] pass (csrc/lm_prefill.hip) against (i) the
    oracle's next-token logits, (ii) the same prompts fed position by position (MIS_PREFILL_SEQ=1: same rounding points, other float32
    summation order), and (iii) continuation: a decode step behind the batched prefill uses the caches it filled.  Ragged rows
    (left padding: a row starts when its first token arrives), 37 rows = a partial 128-row tile, prompts up to 70 tokens.
    Tolerance: logits max <= 0.016 max|ref|; rms over the 74 (row, position) pairs: mean <= 0.008 rms(ref) (the per-row bound of the
    other LM tests), worst <= 0.016 - single rows scatter around the bf16 noise floor (observed worst 0.007-0.011, 0.0069 for the
    decode path at Orpheus width, profiles/r02_parity_observed.json); batched and sequential prefill differ by the same amount."""
    from gpu_util import logits_errors, record
    W, oracle, dev = lm_pair(ocfg, seed=97)
    rng = np.random.default_rng(12)
    lens = [70, 1, 33, 64, 2] + [5 + (b * 7) % 40 for b in range(32)]
    rows = [rng.integers(0, ocfg.vocab_size, n).astype(np.int32) for n in lens]
    nxt = rng.integers(0, ocfg.vocab_size, len(rows)).astype(np.int32)
    monkeypatch.setenv("MIS_PREFILL_SEQ", "0")
    monkeypatch.setenv("MIS_PF_ATTN_LOOP", "0")                           # the chunk's causal attention as two launches over (position, row) pairs
    got = dev.lm_prefill(rows, max_context=96)
    got2 = dev.lm_forward(nxt)                                            # one decode step behind the prompts
    monkeypatch.setenv("MIS_PF_ATTN_LOOP", "1")                           # ... and as one launch per position (what full batches use)
    loop = dev.lm_prefill(rows, max_context=96)
    loop2 = dev.lm_forward(nxt)
    monkeypatch.delenv("MIS_PF_ATTN_LOOP")
    monkeypatch.setenv("MIS_PREFILL_SEQ", "1")
    seq = dev.lm_prefill(rows, max_context=96)
    seq2 = dev.lm_forward(nxt)
    oracle.reset(len(rows))
    ref_all = oracle.forward([np.concatenate([r, nxt[i:i + 1]]) for i, r in enumerate(rows)],
                             logit_positions=[[len(r) - 1, len(r)] for r in rows])
    e_all, d_all, m_all = [], [], []
    for b in range(len(rows)):
        ref = ref_all[b].numpy()
        for dv, sq, rf in ((got[b], seq[b], ref[0]), (got2[b], seq2[b], ref[1])):
            e_max, e_rms, _, agree = logits_errors(dv[None], rf[None])
            assert e_max <= TOL_MAX and agree, (b, e_max)
            e_all.append(e_rms); m_all.append(e_max)
            d_all.append(float(np.sqrt(np.mean((dv - sq) ** 2)) / np.sqrt(np.mean(sq ** 2))))
    # single rows scatter around the bf16 noise floor (0.005-0.011 here, the same for the position-by-position path): bound the
    # mean at the per-row tolerance of the other LM tests and the worst row at twice that
    assert np.mean(e_all) <= 0.008 and np.max(e_all) <= 0.016, (np.mean(e_all), np.max(e_all))
    assert np.mean(d_all) <= 0.008 and np.max(d_all) <= 0.016, (np.mean(d_all), np.max(d_all))
    # the two attention arrangements of the batched path: same keys, same rounding points, (first / second) decode-attention schedule
    l_all = [float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2))) for a, b in zip(list(got) + list(got2), list(loop) + list(loop2))]
    assert np.mean(l_all) <= 0.004 and np.max(l_all) <= 0.016, (np.mean(l_all), np.max(l_all))
    worst = [max(m_all), max(e_all), max(d_all)]
    record(f"batched_prefill_{ocfg.hidden_size}", logits_max_rel=worst[0], logits_rms_rel_worst=worst[1], logits_rms_rel_mean=float(np.mean(e_all)),
           rms_vs_sequential_worst=worst[2], rms_vs_sequential_mean=float(np.mean(d_all)), rms_pairs_vs_per_position_worst=float(np.max(l_all)), tol_max=TOL_MAX, tol_rms_mean=0.008, tol_rms_worst=0.016)


@pytest.mark.parametrize("lens", [[23], [9, 4, 13], [2, 2], [16, 1, 7, 16]], ids=["1x23", "3_ragged", "2x2", "4x16_full"])
def test_short_prompt_prefill_on_the_decode_step_kernels(lens, monkeypatch):
    """Round 6: prompts of at most 64 (position, row) pairs run on the DECODE STEP's kernels with the pairs as rows (`prefill_small`,
    lm_engine.hip: weight-streaming GEMMs, their glue, the attention kernel's pair arrangement) instead of the 128 x 128-tile GEMMs of the
    chunked pass, whose grids are 4 blocks at that size - for the batch-1 token engine's prompt only (`MIS_PREFILL_SMALL=1` forces it here;
    the generic prefill keeps one arithmetic whatever the batch).  Against the oracle (next-token logits, then a decode step behind the prompt:
    the caches), the chunked pass (`MIS_PREFILL_SMALL=0`) and the position-by-position path; q/k-norm + plain-RoPE variant included
    (Soprano's LM is the case this was written for: 23 prompt positions at batch 1)."""
    from gpu_util import logits_errors, record
    for name, cfg in (("llama", ollama.LlamaConfig(**{**ollama.TINY.__dict__, "num_hidden_layers": 2})),
                      ("qwen3_qknorm", ollama.LlamaConfig(**{**ollama.TINY_QWEN3.__dict__, "num_hidden_layers": 2}))):
        W, oracle, dev = lm_pair(cfg, seed=53)
        rng = np.random.default_rng(len(lens))
        rows = [rng.integers(0, cfg.vocab_size, n).astype(np.int32) for n in lens]
        nxt = rng.integers(0, cfg.vocab_size, len(rows)).astype(np.int32)
        got = {}
        for mode, env in (("small", {"MIS_PREFILL_SEQ": "0", "MIS_PREFILL_SMALL": "1"}), ("chunked", {"MIS_PREFILL_SEQ": "0", "MIS_PREFILL_SMALL": "0"}),
                          ("sequential", {"MIS_PREFILL_SEQ": "1"})):
            for k in ("MIS_PREFILL_SEQ", "MIS_PREFILL_SMALL"):
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            a, hid = dev.lm_prefill(rows, max_context=64, want_hidden=True)
            got[mode] = (a, dev.lm_forward(nxt), hid)
        for k in ("MIS_PREFILL_SEQ", "MIS_PREFILL_SMALL"):
            monkeypatch.delenv(k, raising=False)
        oracle.reset(len(rows))
        ref_all = oracle.forward([np.concatenate([r, nxt[i:i + 1]]) for i, r in enumerate(rows)], logit_positions=[[len(r) - 1, len(r)] for r in rows])
        worst = {"small": 0.0, "chunked": 0.0, "sequential": 0.0}
        for b in range(len(rows)):
            ref = ref_all[b].numpy()
            for mode in worst:
                for dv, rf in ((got[mode][0][b], ref[0]), (got[mode][1][b], ref[1])):
                    e_max, e_rms, _, agree = logits_errors(dv[None], rf[None])
                    assert e_max <= TOL_MAX and agree and e_rms <= 0.016, (name, mode, b, e_max, e_rms)
                    worst[mode] = max(worst[mode], e_rms)
        d_small_chunked = max(float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2))) for a, b in zip(list(got["small"][0]) + list(got["small"][1]),
                                                                                                                    list(got["chunked"][0]) + list(got["chunked"][1])))
        assert d_small_chunked <= 0.016, d_small_chunked
        assert np.abs(got["small"][2] - got["sequential"][2]).max() <= 0.02 * np.abs(got["sequential"][2]).max()       # the hidden tap of the last prompt token
        record(f"short_prompt_prefill_{name}_{'x'.join(map(str, lens))}", rms_rel_worst_small=worst["small"], rms_rel_worst_chunked=worst["chunked"],
               rms_rel_worst_sequential=worst["sequential"], small_vs_chunked_rms_worst=d_small_chunked, tol_max=TOL_MAX, tol_rms_row=0.016)


def test_second_attention_schedule_matches_the_oracle():
    """k_attn_decode2 (wave-local prologue, counted waits, one tile in flight per wave while the previous one is multiplied) - the decode
    step's attention at head_dim 128 - against the oracle at contexts that give the waves 0 / 1 / 2 / 3 tiles each (<= 256, 257..512,
    > 512 keys) and with the new key landing in every wave's last tile.  (Its equality with the first schedule, bit for bit on the same
    inputs, is held at the operator level: tests/test_gpu_attn_ops.py::test_second_schedule_and_its_equality_with_the_first, through
    AttnParams::first_schedule.)"""
    from gpu_util import logits_errors, record
    cfg = ollama.LlamaConfig(**{**ollama.TINY.__dict__, "num_hidden_layers": 2})
    W, oracle, dev = lm_pair(cfg)
    rng = np.random.default_rng(31)
    lens = [620, 300, 41]
    rows = [rng.integers(0, cfg.vocab_size, n).astype(np.int32) for n in lens]
    keep = sorted({0, 1, 30, 31, 32, 33, 63, 64, 255, 256, 257, 287, 288, 299, 511, 512, 513, 543, 544, 600, 619})
    dev.lm_reset(len(rows), 640)
    got = {}
    for t in range(max(lens)):
        ids = np.asarray([r[t] if t < len(r) else 0 for r in rows], np.int32)
        act = np.asarray([1 if t < len(r) else 0 for r in rows], np.uint8)
        if t in keep:
            lg = dev.lm_forward(ids, act)
            for b in range(len(rows)):
                if act[b]:
                    got[(b, t)] = lg[b].copy()
        else:
            dev.lm_forward(ids, act, want_logits=False)
    oracle.reset(len(rows))
    checks = [[t for t in keep if t < n] for n in lens]
    ref = oracle.forward(rows, logit_positions=checks)
    worst = [0.0, 0.0]
    for b in range(len(rows)):
        d1 = np.stack([got[(b, t)] for t in checks[b]])
        e_max, e_rms, _, agree = logits_errors(d1, ref[b].numpy())
        assert e_max <= TOL_MAX and e_rms <= TOL_RMS and agree, (b, e_max, e_rms)
        worst = [max(worst[0], e_max), max(worst[1], e_rms)]
    record("attention_second_schedule", logits_max_rel=worst[0], logits_rms_rel=worst[1], tol_max=TOL_MAX, tol_rms=TOL_RMS)
