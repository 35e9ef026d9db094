"""CPU proofs of what tests/test_gpu_enc_ops.py leans on (tests/enc_ref.py): the grid inputs are exact in every summation order, the case
tables reach every instantiation through the launchers' rules, the exact tiers give the stated outputs for the kernels' arithmetic realised
in float32 numpy (fused or not), the bounds hold for that arithmetic and do NOT hold for the mistakes they are there to catch."""
import functools

import numpy as np

import attn_ref as ar
import enc_ref as er
import gemm_ref as gr
from test_gelu_poly_cpu import gelu_poly_f32


@functools.lru_cache(maxsize=None)
def _cases():
    return er.gemm_cases()


def test_gemm_case_table_reaches_every_instantiation_and_edge():
    cs = _cases()
    assert all(c["expect"][0] == c["kernel"] for c in cs)
    assert {c["expect"] for c in cs} == er.GEMM_INSTANTIATIONS
    for kernel in (er.K_BIG, er.K_BIG2, er.K_BIG3):
        mine = [c for c in cs if c["kernel"] == kernel]
        assert {(c["epi"], c["bias"]) for c in mine} == {(e, b) for e in range(4) for b in (False, True)}
        for key in ("M", "N", "K"):
            vals = {c[key] for c in mine if c["K"] < 4096 and c["N"] < 4096}
            assert {(c["epi"], c[key]) for c in mine} >= {(e, v) for e in range(4) for v in vals}, (kernel, key)
        kinds = {(c["epi"], 0 if c["ldx"] == c["K"] else 1 if c["ldx"] > c["K"] else 2) for c in mine}
        assert kinds == {(e, k) for e in range(4) for k in range(3)}, (kernel, kinds)
        assert any(c["epi"] == er.BG_GELU_POS and c["M"] == 200 and c["pos_rows"] == 77 for c in mine) or kernel == er.K_BIG3
        assert any(c["epi"] == er.BG_GELU_POS and c["M"] % c["pos_rows"] for c in mine)
    # the default rule (switch unset): blocks3 = 200 is the boundary
    assert er.gemm_expected(200 * 256, 4, 128, 128, 2)[0] == er.K_BIG3 and er.gemm_expected(199 * 256, 4, 128, 128, 2)[0] == er.K_BIG2
    assert er.gemm_expected(200 * 256, 4, 96, 96, 0)[0] == er.K_BIG and er.gemm_expected(200 * 256, 4, 64, 64, 0)[0] == er.K_BIG
    for kw in (dict(K=48), dict(ldx=132), dict(N=6)):
        a = dict(dict(M=8, N=8, K=128, ldx=128, epi=0), **kw)
        assert er.gemm_expected(**a) == ("err", er.INVALID_INPUT)


def test_grid_inputs_are_exact_in_any_summation_order():
    """|partial sum| <= 4 K units of 2^e, K <= 4096: 2^14 < 2^24 - and, realised in float32 with the k-tiles permuted, the bits of the float64
    reference; residual and bias included"""
    assert max(c["K"] for c in _cases()) == 4096 and 4 * 4096 < 2 ** 24
    rng = np.random.default_rng(0)
    picks = [c for c in _cases() if c["epi"] in (er.BG_NONE, er.BG_RESID)][::9] + [dict(kernel=2, mode=2, M=5, N=8, K=4096, ldx=2048, epi=er.BG_RESID,
                                                                                       bias=True, pos_rows=0, seed=1)]
    for c in picks:
        d = er.gemm_inputs(c)
        units = np.abs(d["x"]) @ np.abs(d["w"]).T / 2.0 ** d["e"]
        assert units.max() <= 4 * c["K"] and np.array_equal(d["x"], d["img"][np.arange(c["M"])[:, None] * c["ldx"] + np.arange(c["K"])[None]])
        ref, _ = er.gemm_reference(c, d)
        for order in (None, rng.permutation(c["K"] // 32), np.arange(c["K"] // 32)[::-1]):
            assert np.array_equal(er.gemm_f32(d, c, order), ref), c


def test_gelu_cases_stay_inside_the_condition_for_the_polynomial():
    """pre-activations in [-4, 8] (inside the issue's [-6, 8]); gelu_poly_f32 (the epilogue's arithmetic restated) on the cases' own pre-activations: at most one bf16 ulp
    from T(gelu64), at most 1 % of a case's elements differing; the additive half in float32 is the float64 rounding-point value"""
    worst, share = 0, 0.0
    for c in _cases():
        if c["epi"] not in (er.BG_GELU, er.BG_GELU_POS) or c["M"] * c["N"] * c["K"] > 2e8:
            continue
        d = er.gemm_inputs(c)
        assert d["pre"].min() >= er.GELU_LO >= -6.0 and d["pre"].max() <= er.GELU_HI <= 8.0
        ref, g = er.gemm_reference(c, d)
        got = er.b16(gelu_poly_f32(er.T(d["pre"]).astype(np.float32))).astype(np.float64)
        u, s = er.gelu_condition(got, g)
        assert u <= er.GELU_ULP and s <= er.GELU_SHARE, (c, u, s)
        worst, share = max(worst, u), max(share, s)
        if c["epi"] == er.BG_GELU_POS:
            assert np.array_equal(er.add_pos_f32(g, c, d), ref)
    assert worst <= 1
    # why not down to -6: on the grids the cases use (multiples of 2^-3 .. 2^-8) the polynomial rounds differently on 5 % and more of [-6, -4)
    for k in (3, 5, 8):
        v = er.T(np.arange(-6 * 2 ** k, -4 * 2 ** k) / 2.0 ** k)
        got = er.b16(gelu_poly_f32(v.astype(np.float32))).astype(np.float64)
        u, s = er.gelu_condition(got, er.T(er.gelu64(v)))
        assert u <= 1 and s > 0.05


def test_layernorm_exact_tiers_hold_fused_or_not_and_catch_a_wrong_divisor():
    for d in er.LN8_D + er.LN_D:
        for rows in er.LN_ROWS:
            x, w, b = er.ln_constant(rows, d, d + rows)
            for fused in (False, True):
                assert np.array_equal(er.ln_f32(x, w, b, fused=fused), np.broadcast_to(b, x.shape))
            assert not np.array_equal(er.ln_f32(x, w, b, divisor=d + 1), np.broadcast_to(b, x.shape))
            x, w, b, a = er.ln_balanced(rows, d, 3 * d + rows)
            want = er.ln_balanced_expected(x, w, a)
            for fused in (False, True):
                assert np.array_equal(er.ln_f32(x, w, b, fused=fused), want)
            # partial sums in another grouping (256 strided lanes, as the block reduction): still 0 and d a^2
            f = np.float32
            lanes = [x[:, i::256].astype(f).sum(-1, dtype=f) for i in range(min(256, d))]
            assert not np.any(np.sum(lanes, 0, dtype=f))
            assert np.array_equal(np.sum([(x[:, i::256].astype(f) ** 2).sum(-1, dtype=f) for i in range(min(256, d))], 0, dtype=f), (d * a * a).astype(f))
            # (what a bf16 output can show of a divisor off by one: up to d = 100 here; beyond, the constant tier holds the divisor)
            if 4 < d <= 100:
                assert not np.array_equal(er.ln_f32(x, w, b, divisor=d - 1), want)
            assert not np.array_equal(er.ln_f32(np.roll(x, 1, -1), w, b), want) and not np.array_equal(er.ln_f32(x, np.roll(w, 1), b), want)


def test_layernorm_gaussian_bound_holds_and_is_sensitive():
    for d in er.LN8_D + er.LN_D:
        x, w, b = er.ln_gauss(3, d, 50 + d)
        y, bound = er.ln_reference(x, w, b)
        for fused in (False, True):
            assert (np.abs(er.ln_f32(x, w, b, fused=fused) - y) / bound).max() <= 1.0
        if 64 <= d <= 100:   # a divisor off by one (beyond d = 100 it is below what bf16 resolves: the constant tier holds it)
            assert (np.abs(er.ln_f32(x, w, b, divisor=d + 1) - y) / bound).max() > 1.0
        if d >= 64:          # a LayerNorm without its bias, a weight shifted by one column
            assert (np.abs(er.ln_f32(x, np.roll(w, 1), b) - y) / bound).max() > 1.0
            assert (np.abs(er.ln_f32(x, w, 0 * b) - y) / bound).max() > 1.0


def test_im2col_reference_and_rounding_classes():
    x = np.arange(2 * 5 * 2, dtype=np.float64).reshape(2, 5, 2) + 1
    r = er.im2col_reference(x, 3, 2)                       # Tin = 5 odd, stride 2: t = 2 reads rows 3, 4, 5 -> the last is outside
    assert r.shape == (6, 6) and list(r[0]) == [0, 0, 1, 2, 3, 4] and list(r[2]) == [7, 8, 9, 10, 0, 0] and list(r[3]) == [0, 0, 11, 12, 13, 14]
    r = er.im2col_reference(x, 5, 1)
    assert list(r[4]) == [7, 8, 9, 10, 0, 0] and list(r[5]) == [0, 0, 11, 12, 13, 14]
    v = er.im2col_f32_values((2, 9, 80), 3)
    lo = v.view(np.uint32) & 0xFFFF
    bits = gr.bf16_bits(v).astype(np.uint32)
    hi = v.view(np.uint32) >> 16
    assert np.any((lo == 0x8000) & (bits == hi)) and np.any((lo == 0x8000) & (bits == hi + 1)) and np.any((lo > 0x8000) & (bits == hi + 1))
    assert np.any((lo < 0x8000) & (lo > 0) & (bits == hi)) and np.isfinite(v).all()


def test_scatter_reference_matches_the_append_index_formulas():
    B, Tn, H, D, ld, k0, v0 = 2, 33, 2, 64, 3 * 128 + 16, 136, 264
    src = np.random.default_rng(1).integers(1, 0x7F00, (B * Tn, ld)).astype(np.uint16)
    Spad = 64 + 64
    kimg, vimg = er.scatter_reference(src, ld, k0, v0, B, Tn, H, D, Spad)
    for (b, h, t, dd) in ((0, 0, 0, 0), (1, 1, 32, 63), (0, 1, 31, 17), (1, 0, 5, 40)):
        assert kimg[b, h, ar.append_k_index(t, dd, D)] == src[b * Tn + t, k0 + h * D + dd]
        assert vimg[b, h, ar.append_v_index(t, dd, D)] == src[b * Tn + t, v0 + h * D + dd]
    assert kimg[0, 0, ar.append_k_index(40, 3, D)] == 0 and vimg[1, 1, ar.append_v_index(63, 9, D)] == 0     # keys T .. tile end
    assert np.all(kimg[:, :, 64 * D:] == 0xFFFF) and np.all(vimg[:, :, 64 * D:] == 0xFFFF)                   # tiles behind


def test_attention_exact_tiers_give_the_stated_outputs():
    for D, Ts in ((64, er.ATTN_T), (128, [1, 33, 257])):
        for i, Tn in enumerate(Ts):
            for tier in ("locator", "uniform"):
                c = er.attn_case(tier, D, Tn, 10 * Tn + D)
                want = er.attn_exact_expected(c)
                assert np.array_equal(er.attn_f32(c), want), (tier, D, Tn)
                if tier == "uniform" and Tn % 32:
                    assert not np.array_equal(er.attn_f32(c, mask_leak=1), want), Tn       # a leaking mask shows in the denominator
                    assert (np.abs(c["K"][0, 0, Tn]) >= 8192).all() and not c["V"][0, 0, Tn].any()
            assert np.isnan(c["K"][0, 0, 32 * -(-Tn // 32)]).all() and c["Spad"] == 32 * -(-Tn // 32) + 64


def test_attention_gaussian_bound_holds_and_is_sensitive():
    for D, Ts in ((64, [1, 31, 64, 257, 300]), (128, [33, 256])):
        for Tn in Ts:
            c = er.attn_case("gauss", D, Tn, 7 * Tn + D)
            ref, bound = er.attn_reference(c)
            assert not c["K"][0, 0, Tn:32 * -(-Tn // 32)].any()                        # the cache contract: zeros to the tile end
            assert (np.abs(er.attn_f32(c) - ref) / bound).max() <= 1.0, (D, Tn)
            if Tn >= 31:
                assert (np.abs(er.attn_reference(c, scale=1.0 / D)[0] - ref) / bound).max() > 1.0
            if Tn % 32 and Tn >= 31:                                                  # one key too many (a zero key with p = exp(-max))
                assert (np.abs(er.attn_f32(c, mask_leak=1) - ref) / bound).max() > 1.0, (D, Tn)


def test_decoder_helper_references():
    rng = np.random.default_rng(5)
    E, P = er.T(rng.standard_normal((6, 32))), er.T(rng.standard_normal((4, 32)))
    lw, lb = er.ln_gauss_wb(32, 1)
    ids, act, pn = np.array([2, -1, 9, 5]), np.array([1, 0, 1, 1]), np.array([0, 3, 4, 7])
    h, x, bound, pc2, pn2 = er.embed_ln_reference(E, P, ids, act, pn, lw, lb, 4, 16)
    assert np.array_equal(h[1], er.T(E[0] + P[3])) and np.array_equal(h[2], er.T(E[0] + P[3])) and np.array_equal(h[3], er.T(E[5] + P[3]))
    assert np.array_equal(h[4], er.T(E[0] + P[0])) and list(pc2) == [0, 3, 4, 7] and list(pn2) == [1, 3, 5, 8]
    img = np.arange(16 * 32)
    un = er.unpack_x(img, 16, 32)
    assert un.shape == (16, 32) and sorted(un.ravel()) == list(img) and un[3, 9] == ar.xpk_index(3, 9, 1)
    l = er.T(rng.standard_normal((3, 16)) * 4)
    out = er.suppress_reference(l, 12, [1, 5, 40, -2], [5, 7], [0, 2, 0], [1, 1, 0])
    assert np.all(out[0, [1, 5, 7]] == er.b16(np.float32(-1e9))) and np.array_equal(np.delete(out[0], [1, 5, 7]), np.delete(l[0], [1, 5, 7]))
    assert np.all(out[1, [1, 5]] < -9e8) and out[1, 7] == l[1, 7] and np.array_equal(out[2], l[2]) and np.array_equal(out[:, 12:], l[:, 12:])
