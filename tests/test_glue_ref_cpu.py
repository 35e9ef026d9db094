"""tests/glue_ref.py holds what it says (no GPU): the exact tiers give the same bits under three float32 summation orders, the Gaussian tier
stays inside its bound under those orders fused and unfused, and float32 emulations of subtly wrong kernels are rejected on the very
inputs tests/test_gpu_glue_ops.py uses."""
import numpy as np
import pytest

import attn_ref as ar
import glue_ref as g

SHAPES = [(3, 16, 4), (2, 16, 100), (5, 16, 252), (4, 16, 1280), (8, 16, 3076), (3, 16, 4100), (1, 16, 6), (9, 16, 6148)]


def _x(c, hp, order="pair", fused=False, **mut):
    if c["ln"]:
        return g.ln_f32(hp, c["w"], c["b"], c["eps"], order, fused, **mut)
    return g.rms_f32(hp, c["w"], c["eps"], order, **mut)          # (RMSNorm has no fused variant: every step is exact or one operation)


@pytest.mark.parametrize("ln", [False, True])
def test_exact_tiers_are_order_independent(ln):
    for S, Mpad, N in SHAPES:
        c = g.exact_case(S, Mpad, N, ln, 100 + N)
        hp = g.hprime(c["slabs"], c["h"])
        assert np.array_equal(hp.astype(np.float64), c["hp"])
        assert np.all(hp[0] == 0) and (not ln or (np.all(hp[1] == hp[1, 0]) and set(hp[2]) == {199.0, 200.0}))
        for order in g.ORDERS:
            for fused in (False, True):
                x = _x(c, hp, order, fused).astype(np.float64)
                assert np.array_equal(x, c["expect"]), (N, order, fused)
        if ln:
            assert np.array_equal(c["expect"][0], c["b"]) and np.array_equal(c["expect"][1], c["b"])
        else:
            assert np.all(c["expect"][0] == 0)


@pytest.mark.parametrize("ln", [False, True])
def test_gaussian_tier_within_the_bound_in_every_order(ln):
    worst = 0.0
    for S, Mpad, N in SHAPES:
        c = g.gauss_case(S, Mpad, N, ln, 200 + N)
        hp = g.hprime(c["slabs"], c["h"])
        for order in g.ORDERS:
            for fused in (False, True):
                frac, bad = g.check_x(c, _x(c, hp, order, fused), hp)
                worst = max(worst, frac)
                assert bad == 0 and frac <= 1.0, (N, order, fused, frac, bad)
    print(f"{'LayerNorm' if ln else 'RMSNorm'}: worst fraction of the bound {worst:.4f}")


def test_slab_order_is_pinned():
    """on Gaussian slabs the sum in another order, a dropped slab and an unrounded o all give other h' bits"""
    for S, Mpad, N in SHAPES:
        if S < 3:
            continue
        c = g.gauss_case(S, Mpad, N, False, 200 + N)
        hp = g.bits(g.hprime(c["slabs"], c["h"]))
        for mut in (dict(reverse=True), dict(drop_last=True), dict(round_o=False)):
            assert not np.array_equal(hp, g.bits(g.hprime(c["slabs"], c["h"], **mut))), (N, mut)
    c = g.exact_case(4, 16, 256, False, 7)                                   # the exact tier notices a dropped slab too
    assert not np.array_equal(g.hprime(c["slabs"], c["h"], drop_last=True).astype(np.float64), c["hp"])


def _rejected(c, hp, exact, order="pair", **mut):
    with np.errstate(all="ignore"):
        x = _x(c, hp, order, **mut)
    if exact:
        return not np.array_equal(x.astype(np.float64), c["expect"], equal_nan=False)
    return g.check_x(c, x, hp)[1] > 0


# Which tier rejects which mutation at which width ("e": the exact tier, "g": the Gaussian tier; statistics in the 'pair' order).  Written
# down so that a later weakening of the inputs shows: the test requires exactly this, and every entry names at least one tier.
#   no_eps       eps dropped: the zero row gives 0 * inf
#   padded       statistics divided by the width rounded up to 32 (widths that are no multiple of 32)
#   twice_last / twice_group   a dead thread's clamped column N - 1 / N - 4 counted twice in the statistics
#   w_first      RMSNorm: w applied before the inner rounding (w = +-2^i on the exact tier commutes with T(): only Gaussian w can show it)
CAUGHT = {
    (False, 4): dict(no_eps="e", twice_last="eg", twice_group="eg", padded="eg", w_first="g"),
    (False, 100): dict(no_eps="e", twice_last="eg", twice_group="eg", padded="eg", w_first="g"),
    (False, 252): dict(no_eps="e", twice_last="eg", twice_group="eg", padded="eg", w_first="g"),
    (False, 1280): dict(no_eps="e", twice_last="g", twice_group="g", w_first="g"),
    (False, 3076): dict(no_eps="e", twice_last="g", twice_group="g", padded="eg", w_first="g"),
    (False, 4100): dict(no_eps="e", twice_last="g", twice_group="g", padded="g", w_first="g"),
    (False, 6): dict(no_eps="e", twice_last="eg", twice_group="eg", padded="eg", w_first="g"),
    (False, 6148): dict(no_eps="e", twice_last="g", twice_group="g", padded="g", w_first="g"),
    (True, 4): dict(no_eps="eg", twice_last="eg", twice_group="eg", padded="eg"),
    (True, 100): dict(no_eps="e", twice_last="eg", twice_group="eg", padded="eg"),
    (True, 252): dict(no_eps="e", twice_last="eg", twice_group="eg", padded="eg"),
    (True, 1280): dict(no_eps="e", twice_last="eg", twice_group="eg"),
    (True, 3076): dict(no_eps="e", twice_last="eg", twice_group="eg", padded="eg"),
    (True, 4100): dict(no_eps="e", twice_last="eg", twice_group="eg", padded="eg"),
    (True, 6): dict(no_eps="e", twice_last="eg", twice_group="eg", padded="eg"),
    (True, 6148): dict(no_eps="e", twice_last="eg", twice_group="eg", padded="eg"),
}


@pytest.mark.parametrize("ln", [False, True])
def test_wrong_statistics_are_rejected(ln):
    for S, Mpad, N in SHAPES:
        ce, cg = g.exact_case(S, Mpad, N, ln, 100 + N), g.gauss_case(S, Mpad, N, ln, 200 + N)
        he, hg = g.hprime(ce["slabs"], ce["h"]), g.hprime(cg["slabs"], cg["h"])
        muts = dict(no_eps=dict(no_eps=True), twice_last=dict(twice=N - 1), twice_group=dict(twice=max(N - 4, 0)))
        if N % 32:
            muts["padded"] = dict(divisor=-(-N // 32) * 32)
        if not ln:
            muts["w_first"] = dict(w_first=True)
        got = {k: ("e" if _rejected(ce, he, True, **m) else "") + ("g" if _rejected(cg, hg, False, **m) else "") for k, m in muts.items()}
        assert got == CAUGHT[(ln, N)] and all(got.values()), (ln, N, got)


def test_one_pass_variance_is_rejected_in_every_order():
    """LayerNorm variance taken as E[x^2] - mean^2: the rows of 256 with 1, 5 and 7 columns at 255 (gauss_case rows 1 .. 3, mean^2 / variance
    about 65536 N / k) reject it in the sequential, the pairwise and the lane-tree order at a small, a medium and every multi-pass width,
    while the two-pass variance stays inside the bound there in every order, fused or not (test_gaussian_tier_within_the_bound_in_every_order
    runs the same cases).  N = 4 is left out: sums of four such squares are exact, E[x^2] - mean^2 is the true variance there."""
    for S, Mpad, N in SHAPES:
        if N == 4:
            continue
        c = g.gauss_case(S, Mpad, N, True, 200 + N)
        hp = g.hprime(c["slabs"], c["h"])
        for r, cols in enumerate(g.offset_row_columns(N), 1):                # the rows are what they claim, through the sum
            want = np.full(N, 256.0)
            want[cols] = 255.0
            assert np.array_equal(hp[r], want)
        for order in g.ORDERS:
            assert _rejected(c, hp, False, order, one_pass=True), (N, order)


def test_rms_check_at_a_power_of_two():
    """p = c / sqrt(c^2 + eps) lies just below 1 and rounds up to it: the other neighbour is 1 - 2^-8 (half a step), far beyond E"""
    hp, w = np.full((1, 64), 2.0), g.T(1.0 + 0.5 * np.random.default_rng(0).standard_normal(64))
    assert g.rms_check(g.T(w * 1.0)[None], hp, w, g.EPS_RMS) == (0.0, 0)
    assert g.rms_check(g.T(w * (1.0 - 2.0 ** -8))[None], hp, w, g.EPS_RMS)[1] > 0
    p, E = g.rms_reference(hp, w, g.EPS_RMS)
    assert np.all(p < 1.0) and np.all(g.T(p) == 1.0)


def test_placement_is_pinned():
    for Mpad, N in ((16, 100), (48, 256)):
        rows = np.arange(Mpad * N, dtype=np.uint32).reshape(Mpad, N).astype(np.uint16)
        img = g.pack_x(rows)
        x, tail = g.unpack_x(img, Mpad, N)
        assert np.array_equal(x, rows) and np.all(tail == 0xFFFF)
        m, k = np.meshgrid(np.arange(Mpad), np.arange(N), indexing="ij")
        wrong = np.full_like(img, 0xFFFF)
        wrong[g.xpk_swapped(m, k, Mpad // 16)] = rows
        assert not np.array_equal(g.unpack_x(wrong, Mpad, N)[0], rows)
        assert sorted(ar.xpk_index(m, k, Mpad // 16).reshape(-1)) == sorted(set(ar.xpk_index(m, k, Mpad // 16).reshape(-1)))


def test_dispatch_restated():
    assert g.glue_expected(2, 3072, False) == (g.K_CPT, 2, 3, 256) and g.glue_expected(2, 3072, True) == (g.K_GLUE4, 2, 1, 768)
    assert g.glue_expected(5, 4096, False) == (g.K_GLUE4, 8, 1, 1024) and g.glue_expected(5, 4100, False)[0] == g.K_GENERAL
    assert g.glue_expected(9, 256, True) == (g.K_GENERAL, 8, 0, 1024) and g.glue_expected(1, 6, False)[0] == g.K_GENERAL
    seen = {g.instantiation_key(g.glue_expected(S, N, ln), N, ln) for N in g.GLUE_N for S in g.GLUE_S + g.GLUE_S_GENERAL for ln in (False, True) if not (ln and N % 2)}
    assert seen == g.GLUE_INSTANTIATIONS and len(seen) == 15


def test_load_time_references():
    for dt in (g.MIS_F32, g.MIS_F16, g.MIS_BF16):
        for n in (1, 255, 257):
            src = g.convert_values(n, dt, n)
            want, nan = g.convert_reference(src, dt)
            assert len(src) == n and len(want) == n
    src = g.convert_values(257, g.MIS_F32, 1)
    want, nan = g.convert_reference(src, g.MIS_F32)
    by = dict(zip(src.view(np.uint32).tolist(), want.tolist()))
    assert by[0x3F808000] == 0x3F80 and by[0x3F818000] == 0x3F82 and by[0x7F7FFFFF] == 0x7F80 and by[0x80000000] == 0x8000 and by[0x00008000] == 0x0000
    assert by[0x00018000] == 0x0002 and by[0x7F800000] == 0x7F80 and nan.sum() >= 3
    q, sc, bi = g.dequant_inputs(16, 192, 4, g.MIS_F32, 3)
    unf, fus = g.dequant_reference(q, sc, bi)
    assert q.min() == 0 and q.max() == 15 and 0 < np.mean(unf != fus) < 0.05                  # equal almost everywhere, not everywhere (planted pairs)
    q, sc, bi = g.dequant_inputs(16, 192, 8, g.MIS_F16, 3)
    unf, fus = g.dequant_reference(q, sc, bi)
    assert np.array_equal(unf, fus)                                                            # 16-bit scales: the product is exact


def test_norm_gemm_exact_case_is_exact():
    import enc_ref as er
    for K, N_out in ((32, 32), (384, 48), (1280, 32)):
        c = g.norm_gemm_exact_case(K, N_out, 9, 5, K)
        hp = g.hprime(c["slabs"], c["h"])
        for order in g.ORDERS:
            x = g.ln_f32(hp, c["w"], c["b"], c["eps"], order).astype(np.float64)
            assert np.array_equal(x, c["x"]), (K, order)
        f = np.float32
        for perm in (np.arange(K), np.arange(K)[::-1], np.random.default_rng(K).permutation(K)):
            acc = np.zeros((16, N_out), f)
            for k in perm:                                                   # one term at a time, any order: the same float32 sum
                acc = (acc + np.outer(c["x"][:, k].astype(f), c["W"][:, k].astype(f))).astype(f)
            assert np.array_equal((acc + c["bias"].astype(f)).astype(np.float64), c["pre"])
        assert er.GELU_LO <= c["pre"][:9].min() and c["pre"][:9].max() <= er.GELU_HI
