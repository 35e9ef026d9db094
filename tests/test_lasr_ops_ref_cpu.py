"""What tests/test_gpu_lasr_ops.py leans on, proven without a GPU: the exact grids of tests/lasr_ops_ref.py give the same bits in any float32
summation order; every k-slab, tap and key tile changes the result, so that a wrong kernel (one key too many, the padding on the wrong side of
an even k, a bias shifted by one, R taken from C, ties to the highest index, the token at a chunk boundary dropped) fails the case inputs; the
SiLU margin covers float32 realisations of the expression and exempts at most 1 % of every case's live elements; the threshold pair sits at
256 / 240 blocks; the case tables name every instantiation and cover their edges on live rows; and the operator references chained as ls_encoder chains the kernels reproduce lasr_ref.Ref's block."""
import numpy as np
import pytest

import attn_ref as ar
import enc_ref as er
import gemm_ref as gr
import lasr_ops_ref as lo
import lasr_ref as lr


# ------------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("epi", range(5))
def test_gemm_grid_is_exact_in_any_slab_order_and_sensitive(epi):
    rng = np.random.default_rng(epi)
    masks, kinds = set(), set()
    for c in lo.gemm_cases(epi):
        d = lo.gemm_inputs(c)
        ref, ex = lo.gemm_reference(c, d)
        assert np.array_equal(gr.bf16_value(gr.bf16_bits(d["x"].astype(np.float32))), d["x"]) and np.abs(d["pre"]).max() < 2.0 ** 12
        for order in (None, rng.permutation(c["K"] // 32)):
            got = lo.gemm_f32(c, d, order)
            if epi == lo.LG_SILU:
                assert np.abs(d["pre"]).max() <= lo.SILU_VMAX
                assert lo.rule_holds(got, ref, ex, d["live"][:, None])[0], c
            else:
                assert np.array_equal(got, ref), c
        assert not ref[~d["live"]].any()
        assert d["live"].any(), c                              # no case compares zeros with zeros only
        if c["bias"] and c["N"] > 1:
            assert not np.array_equal(lo.gemm_reference(c, d, "bias_shift")[0], ref), c
        if epi == lo.LG_AXPBY:
            assert not np.array_equal(lo.gemm_reference(c, d, "r_from_c")[0], ref), c
        if c["K"] > 32:                                        # every k-slab changes the LIVE rows
            xs = d["x"][d["live"]]
            parts = [xs[:, 32 * t:32 * t + 32] @ d["w"][:, 32 * t:32 * t + 32].T for t in range(c["K"] // 32)]
            assert all(p.any() for p in parts) and len({p.tobytes() for p in parts}) == len(parts), c
        masks.add(c["mask"]); kinds.add((c["ldx"] > c["K"], c["bias"], c["in_place"], c["K"]))
    assert masks == {0, 1, 2, 3}
    assert {k[3] for k in kinds} == set(lo.GEMM_K) and {k[0] for k in kinds} == {True, False} and {k[1] for k in kinds} == {True, False}
    assert epi != lo.LG_AXPBY or {k[2] for k in kinds} == {True, False}


def test_gemm_case_tables_cover_the_issue():
    """per epilogue, counted over the cases' LIVE rows only (every case has some): every M and N, every N with and without a bias and with
    more than one K, every M with more than one K, both row strides, every count mode where it masks what it is for"""
    tables = []
    for epi in range(5):
        cs = lo.gemm_cases(epi)
        Ns = lo.GEMM_NF32 if epi == lo.LG_F32 else lo.GEMM_N16
        for c in cs:
            cnt, Tp = lo.mask_of(c["M"], c["mask"], c["seed"])
            live = lo.live_rows(c["M"], cnt, Tp)
            assert live.any(), c
            assert c["mask"] != 2 or (c["M"] > 64 and not live[64:128].any()), c            # a 64-tile wholly masked beside live rows
            assert c["mask"] != 3 or (c["M"] > 128 and not live[:128].any() and live[128:].any()), c
        assert {c["M"] for c in cs} == set(lo.GEMM_M) and {c["N"] for c in cs} == set(Ns) and len(cs) <= 45
        for N in Ns:
            mine = [c for c in cs if c["N"] == N]
            assert {c["bias"] for c in mine} == {True, False} and len({c["K"] for c in mine}) >= 2, (epi, N)
            assert {c["ldx"] > c["K"] for c in mine} == {True, False}, (epi, N)
        for M in lo.GEMM_M:
            mine = [c for c in cs if c["M"] == M]
            assert len({c["K"] for c in mine}) >= 2 and len({c["mask"] for c in mine}) >= 2, (epi, M)
            assert epi == lo.LG_F32 or {c["mask"] for c in mine} >= {0, 1}, (epi, M)
        assert {c["K"] for c in cs} == set(lo.GEMM_K)
        assert {c["mask"] for c in cs if c["M"] >= 128} >= {0, 1, 2}
        if epi != lo.LG_F32:
            assert {c["mask"] for c in cs if c["M"] == 129} == {0, 1, 2, 3}, epi               # the first 128-tile masked, row 128 live
        if epi == lo.LG_AXPBY:
            assert {(c["a"], c["b"]) for c in cs} == {(a, b) for a in lo.AXPBY_A for b in lo.AXPBY_B}
            assert {(c["in_place"], c["mask"] != 0) for c in cs} == {(p, m) for p in (True, False) for m in (True, False)}
        tables.append([{k: v for k, v in c.items() if k not in ("epi", "seed")} for c in cs])
    assert all(tables[0] != t for t in tables[1:4])                                            # the bf16 epilogues do not share one table
    assert {n % 16 for n in lo.GEMM_N16} == {0, 4, 8, 12} and all(n % 2 for n in lo.GEMM_NF32)
    named = {(epi, t) for epi in range(5) for t in (2, 4) if lo.gemm_cases(epi)}
    assert named == lo.GEMM_INSTANTIATIONS and len(named) == 10


def test_tile_rule_values_and_the_threshold_pair():
    """block counts worked out by hand.  That the restated rule IS ls_gemm_epi's is checked on the device, by
    test_gpu_lasr_ops.py::test_gemm_launcher_rule_switches_at_256_blocks and by the report of every tile = 0 launch; here only that the
    threshold pair sits where the issue puts it and that the refusals are restated"""
    for (M, N), ti in {(1, 1): 2, (2048, 2048): 4, (2048, 1920): 2, (2049, 1920): 2, (2177, 1920): 4, (128, 32768): 4, (128, 32640): 2, (32641, 128): 4}.items():
        assert lo.gemm_tile_rule(M, N) == ti, (M, N)           # 1, 16 x 16, 16 x 15, 17 x 15 = 255, 18 x 15, 1 x 256, 1 x 255, 256 x 1 blocks
    a, b = lo.THRESHOLD_CASES
    assert lo.gemm_expected(a["epi"], a["M"], a["N"], a["K"], a["ldx"]) == (lo.LG_BIAS, 4)
    assert lo.gemm_expected(b["epi"], b["M"], b["N"], b["K"], b["ldx"]) == (lo.LG_BIAS, 2)
    assert -(-a["N"] // 128) * -(-a["M"] // 128) == 256 and -(-b["N"] // 128) * -(-b["M"] // 128) == 240
    assert lo.gemm_expected(lo.LG_BIAS, 8, 6, 64, 64)[0] == "err" and lo.gemm_expected(lo.LG_F32, 8, 6, 64, 64) == (lo.LG_F32, 2)
    assert lo.gemm_expected(lo.LG_BIAS, 8, 8, 48, 48)[0] == "err" and lo.gemm_expected(lo.LG_BIAS, 8, 8, 64, 68)[0] == "err"


# ------------------------------------------------------------------------------------------------ SiLU
def test_silu_margin_covers_float32_realisations():
    """on every bf16 value of |v| <= 8 and on a dense float32 sample: three float32 realisations of v / (1 + exp(-v)) leave T(silu64) by at most
    one bf16 ulp, on exempt elements only; the margin's largest value is the one the docstring states"""
    allb = gr.bf16_value(np.arange(0x10000, dtype=np.uint32).astype(np.uint16)).astype(np.float64)
    v16 = allb[np.isfinite(allb) & (np.abs(allb) <= lo.SILU_VMAX)]
    v32 = np.random.default_rng(5).uniform(-8, 8, 400000).astype(np.float32).astype(np.float64)
    for v in (v16, v32):
        want, ex = lo.silu_reference(v)
        for variant in range(3):
            ok, share, worst, _ = lo.rule_holds(lo.silu_f32(v, variant), want, ex)
            assert ok and worst <= 1, (variant, share, worst)
    assert float(lo.silu_reference(v32)[1].mean()) < 0.002          # random data: 2 margin / (relative bf16 spacing) and less
    assert abs(lo.margin(8.0) - 39.2 * lo.U) < 1e-12 and lo.SAFETY == 2
    r, ex = lo.near_boundary(np.array([1.00390625, 1.00390625 * (1 + 1e-5), 1.0, 0.0]), 2e-6)      # 1 + 2^-8: the boundary between 1 and 1 + 2^-7
    assert ex.tolist() == [True, False, False, False]


def test_silu_exempt_share_is_within_the_cap_for_every_case():
    worst = 0.0
    for c in lo.gemm_cases(lo.LG_SILU):
        d = lo.gemm_inputs(c)
        ex = lo.gemm_reference(c, d)[1]
        worst = max(worst, lo.exempt_share(ex, d["live"][:, None]))
    for spec in lo.dw_launches():
        if spec["act"] == 0:
            d = lo.dw_case(spec)
            assert np.abs(lo.dw_pre(d)[0]).max() <= lo.SILU_VMAX
            worst = max(worst, lo.exempt_share(lo.dw_reference(d)[1], d["live"].reshape(-1, 1)))
    for spec in lo.DW_GAUSS + [lo.DW_GATE_PROBE]:
        d = lo.dw_case(spec)
        assert np.abs(d["gate"]).max() <= 8.0
        ex = lo.near_boundary(d["a"] * lo.sigmoid64(d["gate"]), lo.margin(d["gate"]))[1] & d["live"][:, :, None]
        worst = max(worst, lo.exempt_share(ex, d["live"][:, :, None]))
    print("largest exempt share", worst)
    assert worst <= lo.SILU_SHARE


# ------------------------------------------------------------------------------------------------ LayerNorm, RoPE
def test_layernorm_tiers_hold_for_the_lasr_widths():
    for d in lo.LN_D:
        for M in lo.LN_M:
            x, w, b = er.ln_constant(M, d, d + M)
            assert np.array_equal(er.ln_f32(x, w, b), np.broadcast_to(b, x.shape))
            x, w, b, a = er.ln_balanced(M, d, 3 * d + M)
            for fused in (False, True):
                assert np.array_equal(er.ln_f32(x, w, b, fused=fused), er.ln_balanced_expected(x, w, a))
            x, w, b = er.ln_gauss(M, d, 50 + d + M)
            ref, bound = er.ln_reference(x, w, b)
            for fused in (False, True):
                assert (np.abs(er.ln_f32(x, w, b, fused=fused) - ref) <= bound).all()
            cnt, Tp = lo.ln_counts(M, d + M)
            live = lo.live_rows(M, cnt, Tp)
            assert M == 1 or (live.any() and not live.all())
    assert 130 in lo.LN_D and 130 % 64 and not 130 % 2


def test_rope_dyadic_is_exact_gaussian_is_within_the_pair_bound():
    rng = np.random.default_rng(9)
    M, nheads, Tp = 23, 3, 7
    rows = ar.grid_bf16(rng.standard_normal((M, nheads * lo.HD + 8)))
    cs, sn = ar.dyadic_tables(rng, Tp, lo.HD)
    y, _ = lo.rope_reference(rows, nheads, Tp, cs, sn)
    for fused in (False, True):
        assert np.array_equal(lo.rope_f32_rows(rows, nheads, Tp, cs, sn, fused), lo.T(y))
    assert not np.array_equal(lo.T(lo.rope_reference(rows, nheads, Tp, cs, sn, "pos")[0]), lo.T(y))
    cs, sn = lo.gauss_tables(rng, Tp)
    y, bound = lo.rope_reference(rows, nheads, Tp, cs, sn)
    for fused in (False, True):
        assert (np.abs(lo.rope_f32_rows(rows, nheads, Tp, cs, sn, fused) - y) <= bound).all()
    assert (np.abs(lo.T(lo.rope_reference(rows, nheads, Tp, cs, sn, "pos")[0]) - y) > bound).mean() > 0.5


# ------------------------------------------------------------------------------------------------ attention
def test_attention_tiers_and_a_key_too_many():
    launches = lo.attn_launches()
    assert {c["cnt"][0] for c in launches} == set(lo.ATTN_CNT)
    assert {(c["cnt"][0], c["tier"]) for c in launches} == {(n, t) for n in lo.ATTN_CNT for t in lo.ATTN_TIERS}
    assert {(c["heads"], c["tier"]) for c in launches} == {(h, t) for h in lo.ATTN_HEADS for t in lo.ATTN_TIERS}
    assert all(c["cnt"][2] == c["Tp"] and max(c["cnt"]) <= c["Tp"] for c in launches) and any(c["Tp"] % 16 for c in launches)
    leaks = 0
    for spec in launches:
        c = lo.attn_case(spec)
        got = lo.attn_f32(c)
        if c["tier"] == "gaussian":
            ref, bound = lo.attn_reference(c)
            assert (np.abs(got - ref) <= bound).all(), spec
        else:
            assert np.array_equal(got, lo.attn_exact_expected(c)), spec
        if c["tier"] == "uniform" and (c["cnt"] < c["Tp"]).any():          # a key too many: the stale key's zero value enters the denominator
            leak = lo.attn_f32(c, mask_leak=1)
            assert not np.array_equal(leak, got), spec
            leaks += 1
    assert leaks >= 5


# ------------------------------------------------------------------------------------------------ GLU + depthwise conv
def test_dwconv_tiers_are_exact_and_every_tap_and_the_padding_side_count():
    seen = set()
    for spec in lo.dw_launches():
        d = lo.dw_case(spec)
        k = d["k"]
        y, mag, g, _ = lo.dw_pre(d)
        assert np.array_equal(y.astype(np.float32).astype(np.float64), y), spec
        # float32, taps in reverse order: the same numbers
        f = np.float32
        padl = (k - 1) // 2
        gp = np.pad(g, ((0, 0), (padl, k - 1 - padl), (0, 0))).astype(f)
        acc = np.zeros(g.shape, f) + d["shift"].astype(f)
        for kk in reversed(range(k)):
            acc = (acc + (d["taps"][kk].astype(f)[None, None] * gp[:, kk:kk + d["Tp"]]).astype(f)).astype(f)
        assert np.array_equal(acc.astype(np.float64), y), spec
        ref = lo.dw_reference(d)[0]
        if k > 1:
            assert not np.array_equal(lo.dw_reference(d, "mirror")[0], ref), spec
        if k % 2 == 0:
            assert not np.array_equal(lo.dw_reference(d, "pad_side")[0], ref), spec
        if d["tier"] == "impulse" and max(d["cnt"]) >= k:
            for kk in range(k):
                assert not np.array_equal(lo.dw_reference(d, ("drop_tap", kk))[0], ref), (spec, kk)
        assert np.array_equal(np.isnan(gr.bf16_value(d["pw"])).all(-1), ~d["live"].reshape(-1))
        seen.add((d["tier"], d["act"], k))
    assert seen == {(t, a, k) for t in ("dense", "impulse") for a in (0, 1) for k in lo.DW_K}
    assert {c for s in lo.dw_launches() for c in s["cnt"]} == set(lo.DW_CNT) and {s["C"] for s in lo.dw_launches()} == set(lo.DW_C)
    assert lo.DW_MAXK in lo.DW_K and {s["act"] for s in lo.dw_launches()} == {0, 1}
    # the float32 sigmoid at the two gate values
    with np.errstate(over="ignore"):
        assert np.float32(1.0) / (np.float32(1.0) + np.exp(np.float32(-lo.GATE_ONE))) == 1.0 and np.float32(3.0) / (np.float32(1.0) + np.exp(np.float32(-lo.GATE_ZERO))) == 0.0


# ------------------------------------------------------------------------------------------------ moves and the CTC tail
def test_moves_and_ctc_tail_references():
    for ks, st in lo.IM2COL_KS_ST:
        c = lo.im2col_case(ks, st, 8, 1)
        ref = lo.im2col_reference(c)
        assert c["Tin"] == (c["Tout"] - 1) * st + ks and not ref[3:12].any() and np.array_equal(ref[17, -8:], c["x"][2, -1])
        assert np.isnan(gr.bf16_value(ref)).any()
    for V in lo.ARGMAX_V:
        x = lo.argmax_rows(V, 37000 + V)
        want = lo.argmax_reference(x)
        assert x.shape[0] % 4 and want[3] == 0 and want[4] == 0
        if V >= 63:
            assert not np.array_equal(lo.argmax_reference(x, highest=True), want)
            assert want[1] == V // 3 and want[2] == V // 2 and want[5] >= V // 2 and want[6] == V - 1
    cnts, kept_all, dropped = set(), False, False
    for c in lo.collapse_launches():
        tokens, ntok = lo.collapse_reference(c["pred"], c["cnt"])
        cnts |= set(c["cnt"].tolist())
        assert c["pred"].shape[1] > c["cnt"].max()
        for b in range(3):
            n = int(c["cnt"][b])
            assert (tokens[b, ntok[b]:] == -1).all() and (tokens[b, :ntok[b]] >= 0).all()
            kept_all |= n > 256 and ntok[b] == n
        dropped |= not np.array_equal(lo.collapse_reference(c["pred"], c["cnt"], drop_at=256)[0], tokens)
    assert cnts == set(lo.COLLAPSE_CNT) and kept_all and dropped
    a = lo.collapse_launches()[0]
    t, n = lo.collapse_reference(a["pred"][2:, :258], np.array([258]))          # a blank a | a 0: both a kept, the repeat astride 255 | 256 once
    assert t[0, n[0] - 3:n[0]].tolist() == [1, 1, 0] and (a["pred"][2, 255], a["pred"][2, 256]) == (1, 1)
    b = lo.collapse_launches()[0]
    assert lo.collapse_reference(b["pred"], b["cnt"])[1][1] == 0                 # the blank-only row


# ------------------------------------------------------------------------------------------------ the block, chained
def test_chained_operator_references_reproduce_the_model_reference_block():
    """lasr_ref.Ref (round=True, float64 sums, T() as one rounding) against the operator specifications chained in ls_encoder's order"""
    cfg = lr.case_config("B")
    e = dict(cfg["encoder_config"], hidden_size=128, num_attention_heads=2, num_key_value_heads=1, intermediate_size=96, conv_kernel_size=4)
    cfg = dict(cfg, encoder_config=e)
    W = lr.make_weights(cfg, 3)

    class Ref1(lr.Ref):
        def T(self, x):
            return lo.T(x)

    ref = Ref1(cfg, W, round=True, acc=np.float64)
    n, d, H, Hk, k = 11, 128, 2, 1, 4
    x0 = lo.T(np.random.default_rng(4).standard_normal((n, d)))
    want = ref.block(x0, 0)

    q = "encoder.layers.0."
    w = lambda name: lr.bf16(W[q + name]).astype(np.float64)
    mat = lambda name: w(name).reshape(W[q + name].shape[0], -1)
    eps = e["layer_norm_eps"]
    act = lo.LG_RELU if e["hidden_act"] == "relu" else lo.LG_SILU
    fa, fb = e["feed_forward_residual_weights"]
    ca, cb = e["conv_residual_weights"]
    ln = lambda h, p: lo.op_ln(h, w(p + ".weight"), w(p + ".bias"), eps)
    h = x0
    x = ln(h, "norm_feed_forward1")
    ff = lo.op_gemm(x, mat("feed_forward1.linear1.weight"), w("feed_forward1.linear1.bias"), act)
    h = lo.op_gemm(ff, mat("feed_forward1.linear2.weight"), w("feed_forward1.linear2.bias"), lo.LG_AXPBY, h, fa, fb)
    x = ln(h, "norm_self_att")
    wqkv = np.concatenate([mat("self_attn.q_proj.weight"), mat("self_attn.k_proj.weight"), mat("self_attn.v_proj.weight")])
    bqkv = np.concatenate([w("self_attn.q_proj.bias"), w("self_attn.k_proj.bias"), w("self_attn.v_proj.bias")])
    qkv = lo.op_gemm(x, wqkv, bqkv, lo.LG_BIAS)
    f32 = np.float32
    inv = (f32(1.0) / np.power(f32(e["rope_theta"]), np.arange(0, 64, 2, dtype=f32) / f32(64))).astype(f32)
    ang = (np.arange(n, dtype=f32)[:, None] * inv[None]).astype(f32).astype(np.float64)
    cs, sn = np.cos(ang).astype(f32).astype(np.float64), np.sin(ang).astype(f32).astype(np.float64)
    qkv = lo.op_rope(qkv, H + Hk, n, cs, sn)
    att = lo.op_attn(qkv, H, Hk, n, 0.125)
    h = lo.op_gemm(att, mat("self_attn.o_proj.weight"), w("self_attn.o_proj.bias"), lo.LG_AXPBY, h, 1.0, 1.0)
    x = ln(h, "norm_conv")
    pw = lo.op_gemm(x, mat("conv.pointwise_conv1.weight"), w("conv.pointwise_conv1.bias"), lo.LG_BIAS)
    scale = (W[q + "conv.norm.weight"] / np.sqrt(W[q + "conv.norm.running_var"] + f32(1e-5))).astype(f32)
    taps = (W[q + "conv.depthwise_conv.weight"][:, :, 0] * scale[:, None]).astype(f32).T.astype(np.float64)
    shift = ((W[q + "conv.depthwise_conv.bias"] - W[q + "conv.norm.running_mean"]) * scale + W[q + "conv.norm.bias"]).astype(f32).astype(np.float64)
    cv = lo.op_glu_dwconv(pw, taps, shift, k, 1 if e["hidden_act"] == "relu" else 0)
    h = lo.op_gemm(cv, mat("conv.pointwise_conv2.weight"), w("conv.pointwise_conv2.bias"), lo.LG_AXPBY, h, ca, cb)
    x = ln(h, "norm_feed_forward2")
    ff = lo.op_gemm(x, mat("feed_forward2.linear1.weight"), w("feed_forward2.linear1.bias"), act)
    x = lo.op_gemm(ff, mat("feed_forward2.linear2.weight"), w("feed_forward2.linear2.bias"), lo.LG_AXPBY, h, fa, fb)
    got = ln(x, "norm_out")
    assert np.array_equal(got, want) and np.abs(want).max() > 1.0
