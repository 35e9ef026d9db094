"""What tests/test_gpu_sortformer_ops.py leans on, proved without a GPU: the float64 operators of tests/sortformer_ops_ref.py composed ARE the
model (sortformer_ref.Ref: the literal rel-shift, ConformerConvolution, ConvSubsampling), the exact tiers give the same float32 bits in
every summation order, a float32 realisation of each kernel's arithmetic stays inside every derived bound, and a wrong kernel leaves it."""
import math

import numpy as np
import pytest
import torch

import sortformer_ops_ref as so
import sortformer_ref as R

f32 = np.float32


# ------------------------------------------------------------------------------------------------ the specification is the model's
def _model():
    cfg = R.case_config("B")
    W = R.synthetic_weights(cfg, 41)
    return cfg, {k: np.asarray(v, np.float64) for k, v in W.items()}, R.Ref(cfg, W, torch.float64)


def _close(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-11 * max(1.0, np.abs(np.asarray(b)).max())


def _taps9(w):
    return w.reshape(w.shape[0], 9).T.copy()


def test_operators_compose_to_pre_encode():
    cfg, W, ref = _model()
    e = cfg.fc_encoder_config
    C, d, mels = e.subsampling_conv_channels, e.hidden_size, e.num_mel_bins
    S = "fc_encoder.subsampling."
    feats = np.random.default_rng(1).standard_normal((37, mels))
    s = so.op_conv0(feats, _taps9(W[S + "layers_0.weight"]), W[S + "layers_0.bias"])
    for dw, pw in (("layers_2", "layers_3"), ("layers_5", "layers_6")):
        rows = so.op_dw_load(s, _taps9(W[S + dw + ".weight"]), W[S + dw + ".bias"])
        s = so.op_gemm(rows, W[S + pw + ".weight"].reshape(C, C), W[S + pw + ".bias"], so.ACT_RELU).reshape(so.half(s.shape[0]), so.half(s.shape[1]), C)
    T, F3 = s.shape[0], s.shape[1]
    w = W[S + "linear.weight"].reshape(d, C, F3).transpose(0, 2, 1).reshape(d, F3 * C)          # the (c, f) flattening re-ordered to channels last
    emb = so.op_gemm(s.reshape(T, F3 * C), w, W[S + "linear.bias"])
    assert _close(emb, ref.pre_encode(torch.as_tensor(feats)).numpy())


def test_operators_compose_to_a_conformer_block():
    cfg, W, ref = _model()
    e = cfg.fc_encoder_config
    d, H, k = e.hidden_size, e.num_attention_heads, e.conv_kernel_size
    hd, T, q = d // H, 41, "fc_encoder.layers.0."
    x = np.random.default_rng(2).standard_normal((T, d))
    g = lambda n: W[q + n]
    lin = lambda n: (g(n + ".weight"), W.get(q + n + ".bias"))
    ln = lambda n, y: so.op_ln(y, g(n + ".weight"), g(n + ".bias"))
    h = x
    for ff, norm in (("feed_forward1", "norm_feed_forward1"), (None, None), ("feed_forward2", "norm_feed_forward2")):
        if ff:
            big = so.op_gemm(ln(norm, h), *lin(ff + ".linear1"), so.ACT_SILU)
            h = so.op_gemm(big, *lin(ff + ".linear2"), R=h, ra=0.5)
            continue
        wq = np.concatenate([g("self_attn." + n + ".weight") for n in ("q_proj", "k_proj", "v_proj")])
        bq = np.concatenate([W.get(q + "self_attn." + n + ".bias", np.zeros(d)) for n in ("q_proj", "k_proj", "v_proj")])
        qkv = so.op_gemm(ln("norm_self_att", h), wq, bq)
        dist = (np.arange(2 * T - 1) - (T - 1))[:, None]                                         # the table by distance: row d + Tcap - 1
        ang = dist * np.exp(-np.arange(0, d, 2) * math.log(10000.0) / d)[None]
        tab = np.stack([np.sin(ang), np.cos(ang)], -1).reshape(2 * T - 1, d)
        P = so.op_gemm(tab, g("self_attn.relative_k_proj.weight"))
        att = so.op_attn(qkv, H, hd, 1.0, math.sqrt(hd), g("self_attn.bias_u"), g("self_attn.bias_v"), P, T)
        h = so.op_gemm(att, *lin("self_attn.o_proj"), R=h)
        pw = so.op_gemm(ln("norm_conv", h), g("conv.pointwise_conv1.weight")[:, 0], g("conv.pointwise_conv1.bias"))
        scale = g("conv.norm.weight") / np.sqrt(g("conv.norm.running_var") + 1e-5)               # the inference BatchNorm folded into taps and shift
        taps = (g("conv.depthwise_conv.weight")[:, :, 0] * scale[:, None]).T
        shift = (g("conv.depthwise_conv.bias") - g("conv.norm.running_mean")) * scale + g("conv.norm.bias")
        h = so.op_gemm(so.op_glu_dwconv(pw, taps, shift, k), g("conv.pointwise_conv2.weight")[:, 0], g("conv.pointwise_conv2.bias"), R=h)
    assert _close(ln("norm_out", h), ref.fc_layer(0, torch.as_tensor(x)).numpy())                # the LITERAL pad / reshape / slice rel-shift


def test_operators_compose_to_a_bart_layer():
    cfg, W, ref = _model()
    t = cfg.tf_encoder_config
    dt, H, eps, q = t.d_model, t.encoder_attention_heads, t.layer_norm_eps, "tf_encoder.layers.0."
    hd, T = dt // H, 39
    x = np.random.default_rng(3).standard_normal((T, dt))
    lin = lambda n: (W[q + n + ".weight"], W.get(q + n + ".bias"))
    wq = np.concatenate([W[q + "self_attn." + n + ".weight"] for n in ("q_proj", "k_proj", "v_proj")])
    bq = np.concatenate([W.get(q + "self_attn." + n + ".bias", np.zeros(dt)) for n in ("q_proj", "k_proj", "v_proj")])
    att = so.op_attn(so.op_gemm(x, wq, bq), H, hd, hd ** -0.5, 1.0)
    g = so.op_ln(so.op_gemm(att, *lin("self_attn.out_proj"), R=x), W[q + "self_attn_layer_norm.weight"], W[q + "self_attn_layer_norm.bias"], eps)
    gx = so.op_gemm(so.op_gemm(g, *lin("fc1"), so.ACT_RELU), *lin("fc2"), R=g)
    assert _close(so.op_ln(gx, W[q + "final_layer_norm.weight"], W[q + "final_layer_norm.bias"], eps), ref.tf_layer(0, torch.as_tensor(x)).numpy())


# ------------------------------------------------------------------------------------------------ the case tables cover what the issue lists
def test_case_tables_cover():
    ex = so.gemm_cases("exact")
    for load in range(4):
        cs = [c for c in ex if c["load"] == load]
        assert {c["Tp"] * c["rowmul"] for c in cs} == {1, 63, 64, 65, 129} and {c["N"] for c in cs} == set(so.GEMM_N)
        assert {c["K"] for c in cs} == set(so.GEMM_K) and {c["pad"] for c in cs} == {True, False} and {c["bias"] for c in cs} == {True, False}
        assert {c["R"] for c in cs} == {None, "in", "sep"} and {c["ra"] for c in cs if c["R"]} == {1.0, 0.5} and {c["act"] for c in cs} == {so.ACT_NONE, so.ACT_RELU}
        assert any(c["cnt"] is None for c in cs) and any(c["pos"] and c["rowmul"] > 1 for c in cs)
        assert any(c["cnt"] and c["cnt"][2] * c["rowmul"] <= 64 < c["Tp"] * c["rowmul"] for c in cs)              # a whole dead tile
        for tier in ("gauss", "act"):
            assert any(c["load"] == load and c["pad"] for c in so.gemm_cases(tier))
    dws = [c for c in ex if c["load"] == so.LOAD_DW]
    assert {c["Fin"] for c in dws} >= {10, 5, 3} and {c["Tin"] % 2 for c in dws} == {0, 1}
    assert {c["act"] for c in so.gemm_cases("act")} == {so.ACT_SILU, so.ACT_SIGMOID}
    L = so.attn_launches()
    assert {(c["rel"], c["hd"]) for c in L} == {(1, h) for h in so.ATTN_HD_REL} | {(0, h) for h in so.ATTN_HD_PLAIN}
    assert {c["cnt"][0] for c in L} == set(so.ATTN_CNT) and {c["Tp"] - c["cnt"][0] for c in L if c["Tp"] != 130} == {0, 1} and {c["heads"] for c in L} == {1, 2}
    assert {so.attn_rule(c["hd"], c["rel"]) for c in L} == so.ATTN_INSTANTIATIONS
    assert {c["tier"] for c in L if c["rel"]} == set(so.ATTN_TIERS_REL) and {c["qscale"] for c in L if c["rel"]} == {1.0, 0.5}
    for hd in (48, 8):                                            # ND 2 with zero-padded columns, and the smallest head, meet exact and bounded tiers
        assert {c["tier"] for c in L if c["hd"] == hd} >= {"distance", "gaussian", "uniform"}
    D = so.dw_launches()
    assert {(c["k"], c["C"]) for c in D if c["tier"] == "exact"} == {(k, C) for k in so.DW_K for C in so.DW_C}
    assert {n for c in D for n in c["cnt"]} == set(so.DW_CNT) and {c["Tp"] == 130 for c in D} == {True, False}
    for tier in ("impulse", "gauss"):
        assert {c["k"] for c in D if c["tier"] == tier} == set(so.DW_K)


# ------------------------------------------------------------------------------------------------ exact tiers in any order; bounds hold for float32
@pytest.mark.parametrize("load", range(4))
def test_gemm_tiers_in_float32(load):
    rng = np.random.default_rng(7)
    for tier in ("exact", "gauss", "act"):
        for c in so.gemm_cases(tier):
            if c["load"] != load:
                continue
            d = so.gemm_case(c)
            ref, bound, pre = so.gemm_reference(d)
            order = rng.permutation(-(-c["K"] // 32))
            for g in (so.gemm_f32(d), so.gemm_f32(d, order, fused=False)):
                if tier == "exact":
                    assert so.same_bits(g, ref), c
                elif tier == "gauss":
                    assert np.all(np.abs(g - ref) <= bound), c
                else:
                    assert np.abs(pre).max() <= so.ACT_VMAX and np.all(np.abs(g - ref) <= so.ACT_MARGIN * np.abs(ref)), c


def test_attn_tiers_in_float32():
    for c in so.attn_launches():
        d = so.attn_case(c)
        if c["tier"] == "gaussian":
            ref, bound = so.attn_reference(d)
            assert np.all(np.abs(so.attn_f32(d) - ref) <= bound), c
        else:
            want = so.attn_exact_expected(d)
            assert so.same_bits(so.attn_f32(d), want) and so.same_bits(so.attn_f32(d, shuffle=c["seed"]), want), c
            if c["tier"] == "tight_nan":
                dist = np.arange(2 * d["Tcap"] - 1) - (d["Tcap"] - 1)
                assert np.isnan(d["P"][np.abs(dist) >= d["nmax"]]).all() and not np.isnan(d["P"][np.abs(dist) < d["nmax"]]).any()


def test_glu_dwconv_tiers_in_float32():
    for c in so.dw_launches():
        d = so.dw_case(c)
        ref, bound = so.dw_reference(d)
        for g in (so.dw_f32(d), so.dw_f32(d, reverse=True, fused=False)):
            if bound is None:
                assert so.same_bits(g, ref), c
            else:
                assert np.all(np.abs(g - ref) <= bound), c


def test_small_kernels_in_float32():
    for d in so.LN_D:
        x, w, b = (so.r32(a) for a in so.ln_rows("gaussian", 7, d, 40000 + d))
        mean, rstd, bm, br = so.stats_reference(x)
        ref, bound = so.ln_reference(x, w, b)
        for rev in (False, True):
            m32, r32_ = so.stats_f32(x, reverse=rev)
            assert np.all(np.abs(m32 - mean) <= bm) and np.all(np.abs(r32_ - rstd) <= br * rstd)
            assert np.all(np.abs(so.ln_f32(x, w, b, reverse=rev, fused=not rev) - ref) <= bound)
        if d % 2 == 0:
            x, w, b = (so.r32(a) for a in so.ln_rows("balanced", 5, d, 40100 + d))
            mean0, rstd0, want = so.balanced_expected(x, w)
            for rev in (False, True):
                m32, r32_ = so.stats_f32(x, reverse=rev)
                assert so.same_bits(m32, mean0) and so.same_bits(r32_, rstd0) and so.same_bits(so.ln_f32(x, w, b, reverse=rev, fused=rev), want)
    for c in so.CONV0_CASES:                                      # integers on a 2^-3 grid: float32 equals float64
        ref = so.conv0_reference(so.conv0_case(c))
        assert np.array_equal(ref.astype(f32).astype(np.float64), ref) and np.abs(ref).max() < 2.0 ** 10


# ------------------------------------------------------------------------------------------------ wrong kernels are caught
def _caught_exact(cases, make, ref_of, mut):
    for c in cases:
        d = make(c)
        a, b = ref_of(d, None), ref_of(d, mut)
        if not np.array_equal(np.nan_to_num(a.astype(f32), nan=-7.0), np.nan_to_num(b.astype(f32), nan=-7.0)):
            return True
    return False


@pytest.mark.parametrize("mut", ["dw_transpose", "dw_mirror", "cnt_in", "pos_row", "ra", "bias_shift"])
def test_gemm_mutants_leave_the_exact_tier(mut):
    cases = [c for c in so.gemm_cases("exact") if (mut not in ("dw_transpose", "dw_mirror", "cnt_in") or c["load"] == so.LOAD_DW)]
    assert _caught_exact(cases, so.gemm_case, lambda d, m: so.gemm_reference(d, m)[0], mut)


def test_silu_for_sigmoid_leaves_the_margin():
    for c in so.gemm_cases("act"):
        d = so.gemm_case(c)
        ref, wrong = so.gemm_reference(d)[0], so.gemm_reference(d, "act_swap")[0]
        assert np.any(np.abs(wrong - ref) > so.ACT_MARGIN * np.abs(ref)), c


@pytest.mark.parametrize("mut", ["band+1", "band-1", "sign", "swap_uv", "tcap", "head_P", "head_u", "head_v", "key_n", "drop_u"])
def test_attn_mutants_leave_an_exact_tier(mut):
    cases = [c for c in so.attn_launches() if c["tier"] != "gaussian" and (c["rel"] or mut == "key_n") and (c["heads"] == 2 or not mut.startswith("head"))]
    assert _caught_exact(cases, so.attn_case, lambda d, m: so.attn_exact_expected(d) if m is None else so.attn_reference(d, m)[0], mut)


@pytest.mark.parametrize("mut", ["u_qscale", "band+1", "swap_uv", "head_P"])
def test_attn_mutants_leave_the_gaussian_bound(mut):
    hit = 0
    for c in so.attn_launches():
        if c["tier"] == "gaussian" and c["rel"] and (mut != "u_qscale" or c["qscale"] != 1.0) and (mut != "head_P" or c["heads"] == 2):
            d = so.attn_case(c)
            ref, bound = so.attn_reference(d)
            assert np.any(np.abs(so.attn_reference(d, mut)[0] - ref) > bound), c
            hit += 1
    assert hit


@pytest.mark.parametrize("mut", ["halves", "padl", "mirror"])
def test_glu_dwconv_mutants_are_caught(mut):
    for tier in ("exact", "impulse"):
        if (tier, mut) == ("impulse", "halves"):
            continue                                             # a = 0 under a closed gate either way: the exact tier's
        for c in so.dw_launches():
            if c["tier"] == tier and max(c["cnt"]) > 2:
                d = so.dw_case(c)
                ref, bound = so.dw_reference(d)
                wrong = so.dw_reference(d, mut)[0]
                assert np.any(np.abs(wrong - ref) > (0.0 if bound is None else bound)), (c, mut)


def test_conv0_transposed_taps_are_caught():
    for c in so.CONV0_CASES:
        d = so.conv0_case(c)
        assert not np.array_equal(so.conv0_reference(d), so.conv0_reference(d, "transpose"))
