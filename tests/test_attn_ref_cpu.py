"""CPU checks of tests/attn_ref.py - the reference, the layouts, the generators and the bounds that tests/test_gpu_attn_ops.py holds the
decode-attention kernels to.  Nothing here needs a GPU; the GPU test's own cases (attn_ref.gpu_cases) are what is checked."""
import numpy as np
import pytest

import attn_ref as ar
import gemm_ref as gr


def _bits(a):
    return gr.bf16_bits(np.asarray(a, np.float32))


def _same_bits(a, b):
    """bf16 payloads equal; NaN (not written) only where both are"""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(_bits(np.where(na, 0, a)), _bits(np.where(nb, 0, b)))


@pytest.mark.parametrize("S,D", [(32, 64), (96, 128), (1536, 64)])
def test_layouts_round_trip_and_match_the_append(S, D):
    """image(logical) is a bijection, and the element the append's index expressions address (transcribed from the kernel: prow, phalf and
    the V^T index - the writer's side) is the one the fragment description (the reader's side) puts there"""
    K = np.arange(S * D, dtype=np.int64).reshape(S, D)
    ki, vi = ar.k_to_image(K), ar.v_to_image(K)
    assert sorted(ki.tolist()) == list(range(S * D)) and sorted(vi.tolist()) == list(range(S * D))
    assert np.array_equal(ar.k_from_image(ki, S, D), K) and np.array_equal(ar.v_from_image(vi, S, D), K)
    pos, d = np.meshgrid(np.arange(S), np.arange(D), indexing="ij")
    assert np.array_equal(ki[ar.append_k_index(pos, d, D)], K) and np.array_equal(vi[ar.append_v_index(pos, d, D)], K)
    b = ar.k_to_image(np.stack([K, K + 7]))                                 # leading dimensions
    assert np.array_equal(b[1], ki + 7)


def test_case_table_reaches_every_instantiation():
    seen = {ar.expected(c) for c in ar.gpu_cases()}
    assert ar.INSTANTIATIONS <= seen and not [e for e in seen if e[0] == "err"]
    c = ar.gpu_cases()[0]
    assert ar.expected(dict(c, H=26, Hkv=2)) == ("err", ar.INVALID_INPUT)             # G = 13 at D = 128: the LDS footprint
    assert ar.expected(dict(c, H=24, Hkv=2))[2] == 5 and ar.expected(dict(c, Smax=48)) == ("err", ar.INVALID_INPUT)
    s2 = next(c for c in ar.gpu_cases() if c["name"].startswith("s2_"))
    assert ar.expected(s2)[0] == 1 and ar.expected(dict(s2, Smax=1056))[0] == 0 and ar.expected(dict(s2, first_schedule=1))[0] == 0
    xs = next(c for c in ar.gpu_cases() if c["name"].startswith("xs_"))
    assert ar.expected(xs)[3] == 1 and ar.expected(xs, xs_on=False)[3] == 0


def test_float32_realisation_stays_inside_the_bound():
    """the kernels' algorithm in float32 (tiles per wave, online softmax, hi + lo, eight-way combine; np.exp for __expf) on every Gaussian
    case of the GPU table: worst |out - ref| / bound observed 0.973 (the bound's ulp / 2 term is attained by the final rounding; the
    summation terms are far from theirs), every X = max |s - M| <= 32 as the generators promise (largest 22.6)"""
    worst, xmax = 0.0, 0.0
    for c in ar.gpu_cases():
        if c["tier"] != "gauss":
            continue
        r = ar.reference(c)
        got = ar.realise_f32(c)
        assert np.array_equal(np.isnan(got), np.isnan(r["out"])), c["name"]
        m = ~np.isnan(got)
        worst = max(worst, float((np.abs(got - r["out"])[m] / r["bound"][m]).max()))
        xmax = max(xmax, r["xmax"])
    print("worst ratio", worst, "largest X", xmax)
    assert worst <= 1.0 and xmax <= 32.0


def test_exact_tiers_are_exact_in_float32():
    """locator: out == V[target] bit for bit, and the margin of the target's score is > 110; uniform: out == bf16(float32(sum) / float32(kv_len))"""
    n = 0
    for c in ar.gpu_cases():
        if c["tier"] == "gauss":
            continue
        r = ar.reference(c)
        got = ar.realise_f32(c)
        if c["tier"] == "uniform":
            assert _same_bits(got, ar.uniform_expected(c, r)), c["name"]
        else:
            B, H, D, G, rows = c["batch"], c["H"], c["D"], c["H"] // c["Hkv"], c["cache_rows"] or c["batch"]
            want = np.full((B, H * D), np.nan)
            for b in np.nonzero(c["active"])[0]:
                kv_len = c["cross_len"] if c["cross"] else c["pos"][b] + 1
                for h in range(H):
                    Kb = r["K"][b % rows, h // G, :kv_len]
                    s = c["scale"] * (Kb @ r["q"][b, h])
                    t = c["targets"][b, h]
                    assert s[t] - np.delete(s, t).max(initial=-np.inf) > 110.0, (c["name"], b, h)
                    want[b, h * D:(h + 1) * D] = r["V"][b % rows, h // G, t]
            assert _same_bits(got, want) and _same_bits(ar.T(r["out"]), want), c["name"]
        n += 1
    assert n >= 20


def test_dyadic_tables_make_the_rope_step_exact():
    """fused and unfused float32 forms of x1 c - x2 s agree bit for bit with each other and with float64 on every exact-prologue case"""
    n = 0
    for c in ar.gpu_cases():
        if c["rope"] is None or not c["exact"]:
            continue
        B, H, D = c["batch"], c["H"], c["D"]
        x = ar.T(c["slabs"].sum(0))[:B, :(H + c["Hkv"]) * D].reshape(B, -1, D)
        cs, sn = c["rope"][0][c["pos"]][:, None], c["rope"][1][c["pos"]][:, None]
        a, b = ar.rope_f32(x, cs, sn, False), ar.rope_f32(x, cs, sn, True)
        h = D // 2
        want = np.concatenate([x[..., :h] * cs - x[..., h:] * sn, x[..., :h] * sn + x[..., h:] * cs], -1)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(a.astype(np.float64), want), c["name"]
        n += 1
    assert n >= 20


def test_real_tables_move_the_appended_key_by_at_most_one_ulp_rarely():
    """the cap the GPU test applies to the kernel's appended key (attn_ref.KEY_SHARE_CAP = 1 %): a float32 prologue, fused or not, differs
    from T(float64) by at most one bf16 ulp in at most a third of the cap (measured here: no element of the ~20 000 differs - a float32
    result rounds to another bf16 than the float64 one only within 2^-16 of a tie)"""
    worst = 0.0
    for c in ar.gpu_cases():
        if c["exact"] or c["cross"]:
            continue
        want = ar.prologue(c)[1]
        for fused in (False, True):
            d = gr.bf16_ulp_distance(ar.new_key_f32(c, fused), want)
            assert d.max() <= 1, c["name"]
            worst = max(worst, float((d != 0).mean()))
    print("worst share", worst)
    assert worst <= ar.KEY_SHARE_CAP / 3


MUTATIONS = ["sin_sign", "row_plus_one", "adjacent_pairs", "norm_after_rope", "kv_len_plus_one"]


@pytest.mark.parametrize("mut", MUTATIONS)
def test_widened_bound_still_catches_a_wrong_prologue(mut):
    """every real-valued case of the GPU table: a reference with one step done wrong leaves the widened bound somewhere in every case it applies to"""
    n = 0
    for c in ar.gpu_cases():
        if c["exact"] or c["qp"] or (mut == "norm_after_rope" and c["qnorm_w"] is None) or (mut != "kv_len_plus_one" and c["rope"] is None):
            continue
        r, m = ar.reference(c), ar.reference(c, mut)
        ok = ~np.isnan(r["out"])
        assert (np.abs(m["out"] - r["out"])[ok] > r["wide"][ok]).any(), c["name"]
        n += 1
    assert n >= (2 if mut == "norm_after_rope" else 5)


QP_MUTATIONS = ["qp_drop_ktile", "qp_drop_bias", "qp_no_ln_affine", "qp_swap_ntiles"]


@pytest.mark.parametrize("mut", QP_MUTATIONS)
def test_widened_bound_still_catches_a_wrong_query_projection(mut):
    """every QP case of the GPU table: the last k-tile of W_q dropped, the bias dropped, the LayerNorm weight and bias dropped, two n-tiles of
    every head exchanged - each leaves the widened bound (smallest max |mutant - ref| / bound over the cases: 1.6, 2.5, 3.2, 8.1)"""
    n, least = 0, np.inf
    for c in ar.gpu_cases():
        if not c["qp"] or (mut == "qp_drop_bias" and c["qp"]["bias"] is None):
            continue
        r, m = ar.reference(c), ar.reference(c, mut)
        ok = ~np.isnan(r["out"])
        ratio = float((np.abs(m["out"] - r["out"])[ok] / r["wide"][ok]).max())
        least = min(least, ratio)
        assert ratio > 1.0, (c["name"], ratio)
        n += 1
    print(mut, "least ratio", least)
    assert n == (3 if mut == "qp_drop_bias" else 6)
