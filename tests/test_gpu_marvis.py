"""-m gpu: Marvis / CSM (csrc/marvis.hip) against tests/marvis_ref.py: the frame loop (dense, 8-bit, 4-bit) along the engine's own codes
and teacher-forced, the sampler bit for bit, the end rule, batch / seed / row_offset semantics, audio through Mimi in both forms, the
loader, and one case at CSM-1B widths."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import mlx_audio_swift_amd as mas
from mlx_audio_swift_amd import marvis as mv
from oracle import mlxquant
from oracle import sampler as osampler
from oracle import synth

import marvis_ref as mr
import mimi_ref
from gpu_util import record

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}
_MIMI = {}
_REF32 = {}


@pytest.fixture(scope="module", autouse=True)
def _release_handles():
    """Handles shared by this module's tests are destroyed when it ends, so later modules see no extra streams."""
    yield
    for v in _CACHE.values():
        v[1].close()
    for v in _MIMI.values():
        v[1].close()
    _CACHE.clear(); _MIMI.clear(); _REF32.clear()


def _lm_json(c):
    return dict(hidden_size=c.hidden_size, num_hidden_layers=c.num_hidden_layers, intermediate_size=c.intermediate_size,
                num_attention_heads=c.num_attention_heads, num_key_value_heads=c.num_key_value_heads, head_dim=c.resolved_head_dim,
                rms_norm_eps=c.rms_norm_eps, rope_theta=c.rope_theta, rope_scaling=dict(c.rope_scaling), max_position_embeddings=2048)


def _config_json(cfg: mr.CSMConfig, quant=None) -> dict:
    cj = dict(model_type="csm", text_vocab_size=cfg.text_vocab_size, audio_vocab_size=cfg.audio_vocab_size,
              audio_num_codebooks=cfg.audio_num_codebooks, **_lm_json(cfg.backbone),
              depth_decoder_config=dict(vocab_size=cfg.audio_vocab_size, num_codebooks=cfg.audio_num_codebooks, **_lm_json(cfg.decoder)))
    if quant:
        cj["quantization"] = dict(group_size=64, bits=quant)
    return cj


def _quantise(W: dict, bits: int):
    """MLX-quantise what a published quantised checkpoint quantises (every Linear of both LMs, the two Embeddings, projection,
    codebook0_head; never audio_head).  Returns (engine weights with (wq, scales, biases, 64, bits) tuples, reference weights: the
    dequantised values in float32 for streamed Linears, rounded to bf16 for what the engine dequantises at load)."""
    dev, ref = {}, {}
    for k, v in W.items():
        if v.ndim == 2 and k != "model.audio_head":
            wq, sc, bi = mlxquant.quantize(v.float().numpy(), 64, bits)
            sc = torch.from_numpy(np.asarray(sc, np.float32)).to(torch.bfloat16)
            bi = torch.from_numpy(np.asarray(bi, np.float32)).to(torch.bfloat16)
            dq = torch.from_numpy(mlxquant.dequantize(wq, sc.float().numpy(), bi.float().numpy(), 64, bits))
            loaded = k in ("model.text_embeddings.weight", "model.audio_embeddings.weight", "model.projection.weight")
            ref[k] = dq.to(torch.bfloat16).float() if loaded else dq
            dev[k] = (np.asarray(wq, np.uint32), sc, bi, 64, bits)
        else:
            dev[k] = ref[k] = v
    return dev, ref


def _pair(cfg=mr.TINY, quant=None):
    key = (repr(cfg), quant)
    if key not in _CACHE:
        W = mr.make_weights(cfg)
        devW, refW = _quantise(W, quant) if quant else (W, W)
        args = mas.CSMModelArgs.from_json(_config_json(cfg, quant))
        _CACHE[key] = (mr.CSMRef(cfg, refW), mas.MarvisTTSModel.from_weights(args, devW), refW, devW)
    return _CACHE[key][:2]


MIMI_CFG = mimi_ref.MimiRefConfig(dimension=32, n_filters=4, ratios=(3, 2), num_layers=2, num_heads=2, dim_feedforward=64, num_quantizers=12,
                                  bins=96, quantizer_dim=8, sample_rate=240, frame_rate=20.0)


def _host_cfg(c):
    return mas.MimiConfig(num_codebooks=c.num_quantizers, sample_rate=c.sample_rate, frame_rate=c.frame_rate, dimension=c.dimension,
                          n_filters=c.n_filters, n_residual_layers=c.n_residual_layers, ratios=list(c.ratios), kernel_size=c.kernel_size,
                          residual_kernel_size=c.residual_kernel_size, last_kernel_size=c.last_kernel_size, dilation_base=c.dilation_base,
                          compress=c.compress, num_layers=c.num_layers, num_heads=c.num_heads, dim_feedforward=c.dim_feedforward,
                          context=c.context, max_period=c.max_period, bins=c.bins, quantizer_dim=c.quantizer_dim)


def _mimi():
    if "m" not in _MIMI:
        W = mimi_ref.make_synthetic_weights(MIMI_CFG)
        _MIMI["m"] = (mimi_ref.MimiDecoderRef(MIMI_CFG, W), mas.Mimi.from_weights(_host_cfg(MIMI_CFG), W))
    return _MIMI["m"]


def _prompt(cfg, rng, n_text, n_audio):
    K = cfg.audio_num_codebooks
    return mv.tokenize_segment(rng.integers(0, cfg.text_vocab_size, n_text), rng.integers(1, cfg.audio_vocab_size, (K, n_audio)), K, add_eos=False)


def _prompts(cfg, seed=2):
    rng = np.random.default_rng(seed)
    return [_prompt(cfg, rng, 9, 3), _prompt(cfg, rng, 4, 1), _prompt(cfg, rng, 6, 5)]


def _gp(**kw):
    return mas.MarvisGenerateParameters(**kw)


def _dist(a, b):
    scale = float(np.abs(b).max())
    return (float(np.abs(a - b).max()) / scale,
            float(np.sqrt(np.mean((a.astype(np.float64) - b) ** 2)) / np.sqrt(np.mean(b.astype(np.float64) ** 2))))


def _check_case(tag, rows):
    """(b) for one case = the rows of one batch.  rows: (device logits, marvis_ref logits, callable -> marvis_ref in pure float32).
    Bounds of tests/test_gpu_lm.py: every row max|dev - ref| <= 0.016 * max|ref| (two bf16 ulps of the largest logit); rms(dev - ref) /
    rms(ref) <= 0.008 in the mean over the rows and <= 0.016 for the worst row.  Where any of them fails, the bound comes from the
    reference's own rounding error, never from the engine: the float32 reference is evaluated on the same inputs and the engine may
    stand twice as far from the bf16 reference as the bf16 reference stands from float32 (they are two roundings of the same float32
    function) - per row for the max, worst row and mean over the rows for the rms.  Both observed distances are recorded whenever
    that happens (gpu_util.record, and MIS_MARVIS_PARITY_LOG=<file> appends the same rows to a file: profiles/marvis/parity_observed.jsonl
    was written that way).
    Observed on MI355X: CSM-1B widths 0.0075-0.0091 max, rms 0.0071 per row (mean 0.0071-0.0072: within the fixed bounds).  Tiny
    configs: max 0.009-0.023 with 7 of 18 rows above 0.016 (largest 0.0236, 8-bit); rms mean per case 0.0067 / 0.0068 (dense), 0.0109
    / 0.0108 (8-bit), 0.0081 / 0.0098 (4-bit) - the four quantised cases miss the 0.008 mean and need the fall-back for the rms as
    well as for the max (dense Cb = 12 for the max of one row only), against bf16-vs-float32 rms means of 0.014-0.017 per case and
    maxima of 0.018-0.049 per row.  Worst rms of any row: 0.0121."""
    d = [_dist(dv, rf) for dv, rf, _ in rows]
    e_max, e_rms = [x[0] for x in d], [x[1] for x in d]
    rec = dict(dev_vs_bf16_max=e_max, dev_vs_bf16_rms=e_rms, dev_vs_bf16_rms_mean=float(np.mean(e_rms)), fallback=False)
    b_max, b_mean, b_worst = [0.016] * len(rows), 0.008, 0.016
    if max(e_max) > 0.016 or np.mean(e_rms) > b_mean or max(e_rms) > b_worst:
        f = [_dist(rf, f32()) for _, rf, f32 in rows]
        f_max, f_rms = [x[0] for x in f], [x[1] for x in f]
        rec.update(fallback=True, bf16_vs_f32_max=f_max, bf16_vs_f32_rms=f_rms, bf16_vs_f32_rms_mean=float(np.mean(f_rms)))
        b_max = [max(0.016, 2 * x) for x in f_max]
        b_mean, b_worst = max(b_mean, 2 * float(np.mean(f_rms))), max(b_worst, 2 * max(f_rms))
    rec.update(bound_max=b_max, bound_rms_mean=b_mean, bound_rms_worst=b_worst)
    record("marvis " + tag, **rec)
    path = os.environ.get("MIS_MARVIS_PARITY_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps({"test": "marvis " + tag, **rec}) + "\n")
    for b in range(len(rows)):
        assert e_max[b] <= b_max[b], (tag, b, e_max[b], b_max[b])
    assert np.mean(e_rms) <= b_mean and max(e_rms) <= b_worst, (tag, float(np.mean(e_rms)), b_mean, max(e_rms), b_worst)


def _ref32(cfg, quant):
    """marvis_ref in pure float32 on the same weights."""
    key = (repr(cfg), quant)
    if key not in _REF32:
        _REF32[key] = mr.CSMRef(cfg, _CACHE[key][2], round=None)
    return _REF32[key]


@pytest.mark.parametrize("quant", [None, 8, 4], ids=["dense", "8bit", "4bit"])
@pytest.mark.parametrize("Cb", [8, 12])
def test_frame_loop_parity_greedy_and_teacher_forced(quant, Cb):
    cfg = mr.TINY
    ref, dev = _pair(cfg, quant)
    if quant:
        assert dev.native_quant_bits() == [[quant] * 5, [quant] * 4 + [0]]     # every role streams codes (the decoder's heads are audio_head: dense)
    prompts = _prompts(cfg)
    gp = _gp(max_frames=6, quality_level=Cb, temperature=0.0, seed=1)
    codes = dev.generate_codes(prompts, gp)
    assert [c.shape for c in codes] == [(6, Cb)] * 3
    assert dev.generate_codes(prompts[1:2], gp)[0].tolist() == codes[1].tolist()          # batch row == single row
    forced = np.stack(codes)
    logits, sampled, nf = dev.forced_logits(prompts, forced, gp)
    assert nf.tolist() == [6, 6, 6] and np.array_equal(sampled, forced)                   # forcing the loop's own codes changes nothing
    rows = []
    for b, (tok, msk) in enumerate(prompts):
        _, _, rl = ref.run(tok, msk, 6, Cb, 0.0, 1.0, 1, b, forced=codes[b], want_logits=True)
        assert rl.shape == (6, Cb, cfg.audio_vocab_size)
        # (a) along the engine's own codes every chosen code is within 0.04 * max|logits| of the reference maximum - no entry skipped
        for f in range(6):
            for i in range(Cb):
                l = rl[f, i]
                assert l[int(codes[b][f, i])] >= l.max() - 0.04 * float(np.abs(l).max()), (b, f, i)
        # (b) the teacher-forced logits of every (frame, codebook)
        f32 = lambda tok=tok, msk=msk, b=b: _ref32(cfg, quant).run(tok, msk, 6, Cb, 0.0, 1.0, 1, b, forced=codes[b], want_logits=True)[2]
        rows.append((logits[b], rl, f32))
    _check_case(f"tiny q={quant} Cb={Cb}", rows)
    # the node count of the captured frame graph against the chain's expected launches (7 per layer + 1 embed)
    assert dev.launches_per_frame == 3 + Cb * (7 * 2 + 1) + (Cb - 1) * 2 + 2 + (7 * 2 + 1)


def test_sampler_equals_oracle_bit_for_bit():
    V, K = 2051, 32
    rng = np.random.default_rng(7)
    lib = mas._lib.lib()
    for case, scale in enumerate((1.0, 4.0, 12.0)):
        logits = synth.bf16_round((rng.standard_normal((5, V)) * scale).astype(np.float32))
        logits[3, 100:110] = logits[3, 100]                               # ties
        for frame, slot in ((0, 0), (3, 17), (749, 31)):
            out = np.zeros(5, np.int32)
            assert lib.mis_debug_marvis_sample_logits(0, logits.ctypes.data, 5, V, 0.9, 0.8, 11 + case, 2, frame, slot, K, out.ctypes.data) == 0
            want = [osampler.sample(logits[b], 0.9, 0.8, 11 + case, 2 + b, frame * K + slot) for b in range(5)]
            assert out.tolist() == want, (case, frame, slot)
            assert lib.mis_debug_marvis_sample_logits(0, logits.ctypes.data, 5, V, 0.0, 0.8, 0, 0, frame, slot, K, out.ctypes.data) == 0
            assert out.tolist() == [int(np.argmax(logits[b])) for b in range(5)]
    assert max(out) < V                                                   # padded columns (large values in the test harness) are never sampled


def test_end_rule_caps_and_defaults():
    cfg = mr.TINY
    _, dev = _pair(cfg)
    prompts = _prompts(cfg)
    Cb = 8
    gp = _gp(max_frames=7, quality_level=Cb, temperature=0.9, top_p=0.8, seed=3)
    rng = np.random.default_rng(5)
    forced = rng.integers(1, cfg.audio_vocab_size, (3, 7, Cb)).astype(np.int32)
    forced[0, 3] = 0                                                      # row 0: all-zero frame at index 3 ends it with 3 frames
    forced[1, 2] = 0; forced[1, 2, 5] = 9                                 # row 1: c0 = 0 but another code non-zero: goes on
    logits, sampled, nf = dev.forced_logits(prompts, forced, gp)
    assert nf.tolist() == [3, 7, 7]
    assert np.abs(logits[0, :4]).max() > 0 and not logits[0, 4:].any()    # the zero frame was computed, nothing after it
    assert np.abs(logits[1, 6]).max() > 0 and np.abs(logits[2, 6]).max() > 0
    # per-row caps
    g = dev.generate_codes(prompts, _gp(max_frames=9, quality_level=Cb, temperature=0.0), row_max_frames=[2, 9, 5])
    assert [len(x) for x in g] == [2, 9, 5]
    assert mas.MarvisGenerateParameters().max_frames == 750 and mv.MAX_AUDIO_FRAMES == 750
    lib = mas._lib.lib()
    # 0 = the default of 750 frames; anything above is refused, like a prompt of 2048 - 750 positions, a bad Cb and ids outside their tables
    tok, msk, lens, P, B = dev._marshal(prompts[:1])
    out = C.c_void_p(); stride = C.c_int64(); n = (C.c_int32 * 1)()

    def call(params, t=tok, m=msk, ln=lens, p=P):
        return lib.mis_marvis_generate_codes(dev._h, t.ctypes.data, m.ctypes.data, ln.ctypes.data, p, 1, C.byref(params), None, C.byref(out),
                                             C.byref(stride), n)
    assert call(mas._lib.MarvisParamsC(751, 8, 0.0, 1.0, 0, 0)) == 3
    assert call(mas._lib.MarvisParamsC(4, 13, 0.0, 1.0, 0, 0)) == 3 and call(mas._lib.MarvisParamsC(4, -1, 0.0, 1.0, 0, 0)) == 3
    bad = tok.copy(); bad[0, -1, 0] = cfg.audio_vocab_size
    assert call(mas._lib.MarvisParamsC(4, 8, 0.0, 1.0, 0, 0), t=bad) == 3
    bad = tok.copy(); bad[0, 0, -1] = cfg.text_vocab_size
    assert call(mas._lib.MarvisParamsC(4, 8, 0.0, 1.0, 0, 0), t=bad) == 3
    Pl = 2048 - 750
    lt, lm = np.zeros((1, Pl, 13), np.int32), np.zeros((1, Pl, 13), np.uint8)
    lm[:, :, -1] = 1
    assert call(mas._lib.MarvisParamsC(4, 8, 0.0, 1.0, 0, 0), t=lt, m=lm, ln=np.asarray([Pl], np.int32), p=Pl) == 3
    assert "2048" in mas._lib.last_error() or "1298" in mas._lib.last_error()
    with pytest.raises(mas.AudioGenerationError):
        dev.prompt_for(np.zeros(Pl, np.int32), np.zeros((12, 0), np.int32))


def test_batch_rows_seeds_and_row_offset():
    cfg = mr.TINY
    ref, dev = _pair(cfg)
    prompts = _prompts(cfg)[:2]
    gp = _gp(max_frames=8, quality_level=12, temperature=0.9, top_p=0.8, seed=5)
    a = dev.generate_codes(prompts, gp)
    b = dev.generate_codes(prompts, gp)
    c = dev.generate_codes(prompts, _gp(max_frames=8, quality_level=12, temperature=0.9, top_p=0.8, seed=6))
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not all(np.array_equal(x, y) for x, y in zip(a, c))
    shard = dev.generate_codes(prompts[1:], _gp(max_frames=8, quality_level=12, temperature=0.9, top_p=0.8, seed=5, row_offset=1))
    assert np.array_equal(shard[0], a[1])                                 # RNG keyed by the global row
    # the sampled stream is the oracle sampler's on the ENGINE's logits: teacher-forced along the sampled codes, every sampled code equals
    # oracle/sampler.py applied to the returned logits with step = frame * K + codebook
    logits, sampled, nf = dev.forced_logits(prompts, np.stack([x[:4] for x in a]), _gp(max_frames=8, quality_level=12, temperature=0.9, top_p=0.8, seed=5))
    for r in range(2):
        for f in range(4):
            for i in range(12):
                assert int(sampled[r, f, i]) == osampler.sample(logits[r, f, i], 0.9, 0.8, 5, r, f * 12 + i) == int(a[r][f, i])


def test_audio_both_forms_streaming_overlap_and_cancel():
    cfg = mr.TINY
    _, dev = _pair(cfg)
    mref, mimi = _mimi()
    spf = MIMI_CFG.samples_per_frame
    prompts = _prompts(cfg)[:2]
    gp = _gp(max_frames=23, quality_level=12, temperature=0.9, top_p=0.8, seed=5)
    caps = [23, 12]
    pcm, codes = dev.generate_batch(prompts, mimi, gp, row_max_frames=caps, return_codes=True)
    want = dev.generate_codes(prompts, gp, row_max_frames=caps)
    for r in range(2):
        assert np.array_equal(codes[r], want[r]) and len(pcm[r]) == len(codes[r]) * spf == caps[r] * spf
        ref = mref.stream(codes[r].T[None])[0, 0]
        e = float(np.sqrt(np.mean((pcm[r] - ref) ** 2)) / max(np.sqrt(np.mean(ref ** 2)), 1e-12))
        print(f"PARITY marvis audio row {r}: rel rms {e:.2e}")
        assert e < 1e-4                                                   # the bound tests/test_gpu_mimi.py holds the stream to
    # streamed: chunks of 5 frames then the remainder, concatenating to exactly the non-streamed samples
    got = {0: [], 1: []}
    pcm_s = dev.generate_batch(prompts, mimi, gp, row_max_frames=caps, streaming_interval=0.4, on_audio=lambda r, x: got[r].append(x))
    for r in range(2):
        n = caps[r]
        assert [len(x) for x in got[r]] == [5 * spf] * (n // 5) + ([(n % 5) * spf] if n % 5 else [])
        assert np.array_equal(np.concatenate(got[r]), pcm[r]) and np.array_equal(pcm_s[r], pcm[r])
    events = list(dev.generate_stream_batch(prompts, mimi, gp, row_max_frames=caps, streaming_interval=0.4))
    kinds = ["A" if isinstance(e, mas.AudioEvent) else "T" if isinstance(e, mas.TokenEvent) else "I" for e in events]
    for r in range(2):
        toks = [e.token for e in events if isinstance(e, mas.TokenEvent) and e.row == r]
        assert toks == list(codes[r][:, 0])
        assert np.array_equal(np.concatenate([e.audio for e in events if isinstance(e, mas.AudioEvent) and e.row == r]), pcm[r])
        infos = [e for e in events if isinstance(e, mas.InfoEvent) and e.row == r]
        assert len(infos) == 1 and infos[0].info.generation_token_count == caps[r]
    first_audio, last_token = kinds.index("A"), len(kinds) - 1 - kinds[::-1].index("T")
    assert first_audio < last_token, "".join(kinds)                       # audio while the loop was still sampling
    # Cb = 8 decodes 8 codebooks
    pcm8, codes8 = dev.generate_batch(prompts[:1], mimi, _gp(max_frames=6, quality_level=8, temperature=0.0), return_codes=True)
    assert codes8[0].shape == (6, 8)
    ref8 = mref.stream(codes8[0].T[None])[0, 0]
    assert float(np.sqrt(np.mean((pcm8[0] - ref8) ** 2)) / np.sqrt(np.mean(ref8 ** 2))) < 1e-4
    # a Cb Mimi's stream step rejects, and an open host session
    lib = mas._lib.lib()
    tok, msk, lens, P, B = dev._marshal(prompts[:1])
    pcm_p = C.c_void_p(); ps = C.c_int64(); pl = (C.c_int64 * 1)()
    p1 = mas._lib.MarvisParamsC(4, 1, 0.0, 1.0, 0, 0)
    assert lib.mis_marvis_generate(dev._h, mimi._h, tok.ctypes.data, msk.ctypes.data, lens.ctypes.data, P, 1, C.byref(p1), None, C.byref(pcm_p),
                                   C.byref(ps), pl, None, None, None, 0, None, None, None) == 3
    # cancel
    flag = C.c_int(1)
    with pytest.raises(mas.AudioGenerationError) as ei:
        list(dev.generate_stream_batch(prompts, mimi, _gp(max_frames=40, quality_level=12, temperature=0.0), streaming_interval=0.4, cancel_flag=flag))
    assert ei.value.status == 6
    # the session was closed on every path: the host can open its own
    sd = mas.MimiStreamingDecoder(mimi, batch=1)
    sd.decode_frames(codes[0].T[None][:, :, :2])
    lib.mis_mimi_decode_stream_end(mimi._h)


@pytest.mark.parametrize("quant", [None, 8], ids=["raw-keys", "mlx-8bit"])
def test_from_model_directory_round_trips(tmp_path, quant):
    from safetensors.torch import save_file
    cfg = mr.TINY
    _pair(cfg, quant)
    _, dev, refW, devW = _CACHE[(repr(cfg), quant)]
    sd = {}
    for k, v in devW.items():
        if isinstance(v, tuple):
            base = k[: -len(".weight")]
            sd[k] = torch.from_numpy(v[0].view(np.int32)).view(torch.int32).contiguous()
            sd[base + ".scales"], sd[base + ".biases"] = v[1].contiguous(), v[2].contiguous()
        else:
            sd[k if quant else mr.raw_key(k)] = v.contiguous()
    with open(tmp_path / "config.json", "w") as f:
        json.dump(_config_json(cfg, quant), f)
    save_file(sd, str(tmp_path / "model.safetensors"))
    m = mas.MarvisTTSModel.from_pretrained(str(tmp_path))
    try:
        prompts = _prompts(cfg)
        gp = _gp(max_frames=3, quality_level=12, temperature=0.0)
        forced = np.stack(dev.generate_codes(prompts, gp))
        a = m.forced_logits(prompts, forced, gp)[0]
        b = dev.forced_logits(prompts, forced, gp)[0]
        assert np.array_equal(a, b)
        if quant:
            assert m.native_quant_bits() == dev.native_quant_bits()
    finally:
        m.close()


@pytest.mark.parametrize("flavor", ["llama-1B", "llama-100M"])
def test_full_width_teacher_forced(flavor):
    """CSM-1B widths of both flavours (32 / 8 heads of 64 at d = 2048; 8 / 2 heads of 128 with ffn 8192 at d = 1024) as backbone AND
    decoder of one model, reduced layer counts, K = 32, audio vocabulary 2051, text vocabulary 128 256, 4 frames."""
    lc = mr.LLAMA_1B if flavor == "llama-1B" else mr.LLAMA_100M
    other = mr.LLAMA_100M if flavor == "llama-1B" else mr.LLAMA_1B
    cfg = mr.CSMConfig(dataclasses.replace(lc, num_hidden_layers=2), dataclasses.replace(other, num_hidden_layers=1), 128256, 2051, 32)
    ref, dev = _pair(cfg)
    rng = np.random.default_rng(9)
    prompts = [_prompt(cfg, rng, 7, 2), _prompt(cfg, rng, 3, 4)]
    gp = _gp(max_frames=4, quality_level=32, temperature=0.0)
    forced = rng.integers(1, 2051, (2, 4, 32)).astype(np.int32)
    logits, sampled, nf = dev.forced_logits(prompts, forced, gp)
    assert nf.tolist() == [4, 4]
    rows = []
    for b, (tok, msk) in enumerate(prompts):
        _, rs, rl = ref.run(tok, msk, 4, 32, 0.0, 1.0, 0, b, forced=forced[b], want_logits=True)
        f32 = lambda tok=tok, msk=msk, b=b: _ref32(cfg, None).run(tok, msk, 4, 32, 0.0, 1.0, 0, b, forced=forced[b], want_logits=True)[2]
        rows.append((logits[b], rl, f32))
    _check_case(f"fullwidth {flavor}", rows)
    key = (repr(cfg), None)
    _REF32.pop(key, None)
    _CACHE.pop(key)[1].close()                                          # gigabytes of tables: released before the next case
