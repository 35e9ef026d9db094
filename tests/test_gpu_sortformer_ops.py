"""The private kernels of csrc/sortformer.hip, one launch at a time through the mis_debug_sortformer_* entry points (the launchers the chain
itself calls), against tests/sortformer_ops_ref.py: bit for bit wherever the arithmetic is exact, a derived bound elsewhere.  Every launch
asserts its status, the reported instantiation against the restated rule, that no poison is left where the kernel must write, and that
rows behind a count are zero.  What the expectations lean on is proved in tests/test_sortformer_ops_ref_cpu.py."""
import numpy as np
import pytest

import gpu_util
import sortformer_ops_ref as so

pytestmark = pytest.mark.gpu


def whole(out):
    """no poison (0xFFFFFFFF) and no NaN left in an output the kernel must write completely"""
    return not np.any(so.bits(out) == so.POISON) and not np.isnan(out).any()


def zero_behind(out, live):
    return np.all(so.bits(out)[~np.asarray(live, bool)] == 0)


def ratio(got, ref, bound):
    return float((np.abs(got.astype(np.float64) - ref) / np.maximum(bound, 1e-300))[bound > 0].max(initial=0.0))


# ------------------------------------------------------------------------------------------------ GEMM
def _gemm(d):
    st, Y, Ra, rep = so.run_gemm(d)
    assert st == so.OK and rep == so.gemm_load_rule(d["load"]), (st, rep, d["load"])
    assert whole(Y) and zero_behind(Y, d["live"])
    if Ra is not None:                                               # a residual of its own comes back untouched (NaN rows included)
        want = so.nan_where(d["Rv"], ~d["live"][:, None]).astype(np.float32)
        assert np.array_equal(so.bits(Ra), so.bits(want))
    return Y


@pytest.mark.parametrize("load", range(4))
def test_gemm_exact(load):
    for c in so.gemm_cases("exact"):
        if c["load"] == load:
            d = so.gemm_case(c)
            assert so.same_bits(_gemm(d), so.gemm_reference(d)[0]), c


@pytest.mark.parametrize("load", range(4))
def test_gemm_gauss(load):
    worst = 0.0
    for c in so.gemm_cases("gauss"):
        if c["load"] == load:
            d = so.gemm_case(c)
            ref, bound, _ = so.gemm_reference(d)
            worst = max(worst, ratio(_gemm(d), ref, bound))
    assert gpu_util.observe("error / bound", worst, 1.0)


@pytest.mark.parametrize("load", range(4))
def test_gemm_silu_sigmoid(load):
    worst = 0.0
    for c in so.gemm_cases("act"):
        if c["load"] == load:
            d = so.gemm_case(c)
            ref = so.gemm_reference(d)[0]
            worst = max(worst, ratio(_gemm(d), ref, so.ACT_MARGIN * np.abs(ref)))
    assert gpu_util.observe("error / bound", worst, 1.0)


def test_gemm_alone_equals_ragged():
    for c in so.gemm_cases("gauss"):
        if c["cnt"] is None:
            continue
        d = so.gemm_case(c)
        Y, nr = _gemm(d), c["Tp"] * c["rowmul"]
        for b in range(d["B"]):
            st, Yb, _, _ = so.run_gemm(d, only=b)
            assert st == so.OK and np.array_equal(so.bits(Yb), so.bits(Y[b * nr:(b + 1) * nr])), (c, b)


# ------------------------------------------------------------------------------------------------ attention
def _attn(d):
    st, out, rep = so.run_attn(d)
    assert st == so.OK and rep == so.attn_rule(d["hd"], d["rel"]), (st, rep)
    live = (np.arange(d["Tp"])[None, :] < d["cnt"][:, None]).reshape(-1)
    assert whole(out) and zero_behind(out, live)
    return out


@pytest.mark.parametrize("rel", (1, 0))
def test_attn_exact(rel):
    seen = set()
    for c in so.attn_launches():
        if c["rel"] == rel and c["tier"] != "gaussian":
            d = so.attn_case(c)
            assert so.same_bits(_attn(d), so.attn_exact_expected(d)), c
            seen.add(c["tier"])
    assert seen == set(so.ATTN_TIERS_REL if rel else so.ATTN_TIERS_PLAIN) - {"gaussian"} | ({"distance"} if rel else set())


@pytest.mark.parametrize("rel", (1, 0))
def test_attn_gauss(rel):
    worst = 0.0
    for c in so.attn_launches():
        if c["rel"] == rel and c["tier"] == "gaussian":
            d = so.attn_case(c)
            ref, bound = so.attn_reference(d)
            worst = max(worst, ratio(_attn(d), ref, bound))
    assert gpu_util.observe("error / bound", worst, 1.0)


def test_attn_alone_equals_ragged():
    for c in so.attn_launches()[::4]:
        d = so.attn_case(c)
        out, Tp = _attn(d), d["Tp"]
        for b in range(d["B"]):
            st, ob, _ = so.run_attn(d, only=b)
            assert st == so.OK and np.array_equal(so.bits(ob), so.bits(out[b * Tp:(b + 1) * Tp])), (c, b)


# ------------------------------------------------------------------------------------------------ GLU + depthwise conv
def _dw(d):
    st, out = so.run_glu_dwconv(d)
    assert st == so.OK and whole(out) and zero_behind(out, d["live"].reshape(-1))
    return out


def test_glu_dwconv_exact():
    for c in so.dw_launches():
        if c["tier"] == "exact":
            d = so.dw_case(c)
            assert so.same_bits(_dw(d), so.dw_reference(d)[0]), c


@pytest.mark.parametrize("tier", ("impulse", "gauss"))
def test_glu_dwconv_bounded(tier):
    worst = 0.0
    for c in so.dw_launches():
        if c["tier"] == tier:
            d = so.dw_case(c)
            ref, bound = so.dw_reference(d)
            worst = max(worst, ratio(_dw(d), ref, bound))
    assert gpu_util.observe("error / bound", worst, 1.0)


def test_glu_dwconv_alone_equals_ragged():
    for c in so.dw_launches()[::3]:
        d = so.dw_case(c)
        out, Tp = _dw(d), d["Tp"]
        for b in range(d["B"]):
            st, ob = so.run_glu_dwconv(d, only=b)
            assert st == so.OK and np.array_equal(so.bits(ob), so.bits(out[b * Tp:(b + 1) * Tp])), (c, b)


# ------------------------------------------------------------------------------------------------ the small kernels
def test_conv0_exact():
    for c in so.CONV0_CASES:
        d = so.conv0_case(c)
        st, out = so.run_conv0(d)
        assert st == so.OK and whole(out)
        assert zero_behind(out, np.broadcast_to((np.arange(d["T1p"])[None, :] < d["T1"][:, None])[:, :, None, None], out.shape))
        assert so.same_bits(out, so.conv0_reference(d)), c


@pytest.mark.parametrize("d", so.LN_D)
def test_stats_and_ln(d):
    worst = 0.0
    for M in so.LN_M:
        for ti, tier in enumerate(("constant", "balanced", "gaussian")):
            if tier == "balanced" and d % 2:
                continue
            seed = 39500 + 10 * d + M + ti
            x, w, b = so.ln_rows(tier, M, d, seed)
            x, w, b = so.r32(x), so.r32(w), so.r32(b)
            cnt, Tp = so.ln_counts(M, seed)
            live = so.ln_live(M, cnt, Tp)
            st, stats = so.run_stats(x)
            assert st == so.OK and whole(stats)
            ys = []
            for in_place in (0, 1):
                st, y = so.run_ln(so.nan_where(x, ~live[:, None]), w, b, cnt, Tp, in_place)
                assert st == so.OK and whole(y) and zero_behind(y, np.broadcast_to(live[:, None], y.shape))
                ys.append(y)
            assert np.array_equal(so.bits(ys[0]), so.bits(ys[1]))
            y = ys[0][live]
            if tier == "constant":
                rstd0 = np.float32(1) / np.sqrt(np.float32(so.EPS))
                assert so.same_bits(stats[:, 0], x[:, 0]) and np.all(so.bits(stats[:, 1]) == so.bits(np.full(M, rstd0, np.float32)))
                assert so.same_bits(y, np.broadcast_to(b, x.shape)[live])
            elif tier == "balanced":
                mean, rstd, want = so.balanced_expected(x, w)
                assert so.same_bits(stats[:, 0], mean) and so.same_bits(stats[:, 1], rstd) and so.same_bits(y, want[live])
            else:
                mean, rstd, bm, br = so.stats_reference(x)
                ref, bound = so.ln_reference(x, w, b)
                worst = max(worst, ratio(stats[:, 0], mean, bm), ratio(stats[:, 1], rstd, br * rstd), ratio(y, ref[live], bound[live]))
    assert gpu_util.observe("error / bound", worst, 1.0)


def test_intake_exact():
    rng = np.random.default_rng(39700)
    for d, Tp, cnt in ((48, 5, [3, 5, 0]), (65, 7, [9, 1, 7])):
        cnt = np.asarray(cnt, np.int32)
        x = so.r32(rng.standard_normal((3 * Tp, d)))
        live = (np.arange(Tp)[None, :] < cnt[:, None]).reshape(-1)
        g = float(np.sqrt(np.float32(d)))
        st, y = so.run_intake(so.nan_where(x, ~live[:, None]), cnt, Tp, g)
        assert st == so.OK and whole(y) and zero_behind(y, np.broadcast_to(live[:, None], y.shape))
        assert so.same_bits(y[live], x[live] * float(np.float32(g)))


@pytest.mark.parametrize("on", (1, 0))
def test_peak_exact(on):
    x, N = so.peak_case(39800)
    st, scale = so.run_peak(x, N, on)
    assert st == so.OK and whole(scale)
    assert np.array_equal(so.bits(scale), so.bits(so.peak_reference(x, N, on)))


# ------------------------------------------------------------------------------------------------ instantiations, refusals
def test_every_instantiation_runs():
    loads, attns = set(), set()
    for load in range(4):
        d = so.gemm_case(next(c for c in so.gemm_cases("exact") if c["load"] == load))
        st, _, _, rep = so.run_gemm(d)
        assert st == so.OK
        loads.add(rep)
    for nd, rel in sorted(so.ATTN_INSTANTIATIONS):
        d = so.attn_case(next(c for c in so.attn_launches() if so.attn_rule(c["hd"], c["rel"]) == (nd, rel)))
        st, _, rep = so.run_attn(d)
        assert st == so.OK
        attns.add(rep)
    assert loads == so.GEMM_INSTANTIATIONS and attns == so.ATTN_INSTANTIATIONS


def test_refused_shapes_launch_nothing():
    g = so.gemm_case(next(c for c in so.gemm_cases("exact") if c["load"] == so.LOAD_LN and not c["pad"]))
    for over in (dict(ldy=g["N"] - 1), dict(ldx=g["K"] - 1), dict(load=4), dict(act=4), dict(stats=None), dict(rowmul=0), dict(load=so.LOAD_DW)):
        st, Y, _, rep = so.run_gemm(g, **over)
        assert st == so.INVALID_INPUT and rep == -1 and np.all(so.bits(Y) == so.POISON), over
    a = so.attn_case(next(c for c in so.attn_launches() if c["rel"] and c["tier"] == "gaussian"))
    for over in (dict(hd=65), dict(hd=0), dict(ld=a["voff"] + a["heads"] * a["hd"] - 1), dict(ldo=a["heads"] * a["hd"] - 1), dict(ldp=a["heads"] * a["hd"] - 1),
                 dict(Tcap=0), dict(koff=-1)):
        st, out, rep = so.run_attn(a, **over)
        assert st == so.INVALID_INPUT and rep == (-1, -1) and np.all(so.bits(out) == so.POISON), over
    d = so.dw_case(so.dw_launches()[0])
    for k in (0, so.DW_MAXK + 1):
        st, out = so.run_glu_dwconv(d, k=k)
        assert st == so.INVALID_INPUT and np.all(so.bits(out) == so.POISON), k
    x, N = so.peak_case(39801)
    st, scale = so.run_peak(x, np.array([301, 1, 2, 3, 4], np.int32), 1)
    assert st == so.INVALID_INPUT and np.all(so.bits(scale) == so.POISON)
