"""The private kernels of csrc/moonshine.hip as OPERATORS: k_ms_conv1_tanh, the GroupNorm chain, k_ms_rope_rows, k_ms_attn_enc / _self / _cross,
k_ms_gemv in the decoder's four instantiations, k_ms_embed and k_ms_argmax_embed, one launch at a time through the mis_debug_moonshine_* entry
points at the end of csrc/moonshine.hip (the engine's own launchers), against the float64 specification of tests/moonshine_ops_ref.py (its
claims are proven in tests/test_moonshine_ops_ref_cpu.py).  Inputs whose result is exact are compared BIT FOR BIT - a key too many behind
T3[b], a RoPE pair rotated at column rot, a bias shifted by a column, a cache row appended by the wrong head, a row taken from
min(row, B - 1) cannot hide behind a tolerance; SiLU and the GroupNorm output are held to the boundary rule, Gaussian data to the derived
bounds.  Every launch asserts its status and that no poison (0xFFFF / NaN) is left where the kernel must write; the entry points fail on a
touched guard or padding column."""
import numpy as np
import pytest

import gemm_ref as gr
import lasr_ops_ref as lo
import moonshine_ops_ref as mo
from gpu_util import record

pytestmark = pytest.mark.gpu
OK, INVALID = mo.OK, mo.INVALID_INPUT


def _fail(errors):
    assert not errors, f"{len(errors)} failures, first: " + "\n".join(str(e) for e in errors[:8])


def _tag(c):
    return str({k: v for k, v in c.items() if k in ("kind", "tier", "heads", "T3", "Tpad", "pos", "rot", "d", "ln", "epi", "B", "K", "N", "bias", "seed")})


def _bound_check(got, ref, bound, tag, errors):
    """-> the worst fraction of the bound"""
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = np.where(bound > 0, np.abs(got - ref) / bound, np.where(got == ref, 0.0, np.inf))
    worst = float(np.nanmax(frac)) if not np.isnan(got).any() else float("inf")
    print(f"fraction of the bound {worst:.4f} {tag}")
    if not worst <= 1.0:
        errors.append(f"outside the bound ({worst:.3f} of it, or NaN) " + tag)
    return worst


# ------------------------------------------------------------------------------------------------ conv1 + tanh
def test_conv1_exact_taps_ragged_rows_and_the_gaussian_bound():
    """d of two channels a thread and no multiple of 256; T1 of 0, 1 and around the 16-frame block in one batch, T1pad no multiple of 16, a
    stride longer than the longest row, 3e4 behind every row's own extent; frames behind T1[b] are exact zeros"""
    errors, worst = [], 0.0
    for c in mo.conv1_cases():
        d = mo.conv1_case(c)
        st, out = mo.run_conv1(d)
        ref, bound = mo.conv1_reference(d)
        if st != OK or np.isnan(out).any():
            errors.append(f"status {st} or poison left {_tag(c)}")
            continue
        dead = np.arange(d["T1pad"])[None] >= d["T1"][:, None]
        if np.any(out[dead].view(np.uint32) != 0):
            errors.append("frames behind T1[b] are not exact zeros " + _tag(c))
        if c["tier"] == "exact":
            if not np.array_equal(out.view(np.uint32), ref.astype(np.float32).view(np.uint32)):
                errors.append("exact tier differs " + _tag(c))
        else:
            worst = max(worst, _bound_check(out.astype(np.float64), ref, bound, _tag(c), errors))
    record("moonshine_ops_conv1_gauss", fraction_of_bound=worst, tanh_ulp_allowed=mo.TANH_ULP, tanh_route="measured: 4 x torch float32 CPU tanh vs float64",
           tanh_cpu_ulp=mo.TANH_CPU_ULP)
    _fail(errors)


# ------------------------------------------------------------------------------------------------ GroupNorm
def test_groupnorm_partials_bit_for_bit_output_by_the_boundary_rule():
    """one chunk, the chunk edge, two and three chunks and a one-frame row in one batch: nch comes from the longest row, a short row's later
    chunks hold 0; both passes' partials and the zero mean bit for bit; zeros behind T1[b], in the tail and nowhere else"""
    errors = []
    c = mo.gn_case()
    ref = mo.gn_reference(c)
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
    st, p0, _, _, _, nch = mo.run_groupnorm(c, stage=0)
    if st != OK or nch != c["nch"] or not np.array_equal(p0.view(np.uint32), f32(ref["part0"]).view(np.uint32)):
        errors.append(f"stage 0: status {st}, nch {nch}, or the pass-0 partials differ")
    st, p0, p1, _, _, nch = mo.run_groupnorm(c, stage=1)
    if st != OK or not np.array_equal(p0.view(np.uint32), f32(ref["part0"]).view(np.uint32)) or not np.array_equal(p1.view(np.uint32), f32(ref["part1"]).view(np.uint32)):
        errors.append(f"stage 1: status {st}, or the partials differ")
    st, p0, p1, stats, y, nch = mo.run_groupnorm(c, stage=2)
    if st != OK:
        errors.append(f"stage 2: status {st}")
    else:
        if not np.array_equal(p1.view(np.uint32), f32(ref["part1"]).view(np.uint32)) or np.any(stats[:, 0].view(np.uint32) != 0):
            errors.append("the chain's partials differ or the mean is not exactly 0")
        rel = np.abs(stats[:, 1].astype(np.float64) - ref["stats"][:, 1]) / ref["stats"][:, 1]
        if not rel.max() <= 8 * mo.SAFETY * mo.U:
            errors.append(f"rstd off by {rel.max():.3g} relative")
        if np.any(y[~ref["live"]] != 0):
            errors.append("frames behind T1[b] or the tail are not exact zeros")
        ok, share, worst, n = lo.rule_holds(mo.val(y), ref["y"], ref["exempt"], ref["live"])
        es = lo.exempt_share(ref["exempt"], ref["live"])
        print(f"GroupNorm: {n} live elements, exempt {es:.5f}, differing {share:.5f}, worst {worst} ulp")
        record("moonshine_ops_groupnorm", share_differing=share, worst_ulp=worst, exempt_share=es, rstd_rel_err=float(rel.max()))
        if not ok or es > mo.SILU_SHARE:
            errors.append(f"output differs off a rounding boundary or by more than one bf16 ulp ({worst}), exempt share {es:.4f}")
    _fail(errors)


# ------------------------------------------------------------------------------------------------ RoPE
def test_rope_rows_partial_interleaved_bit_for_bit():
    """rot of head sizes 36, 52, 64 and full rotation, v heads and padding behind the rotated heads, M no multiple of 4 and above Tpad; the whole
    image is compared: columns >= rot, v heads and padding untouched"""
    errors = []
    for c in mo.rope_cases():
        d = mo.rope_case(c)
        st, img = mo.run_rope(d)
        if st != OK or not np.array_equal(img, mo.rope_reference(d)):
            errors.append(f"status {st} or the rows differ {_tag(c)}")
    _fail(errors)


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("kind", [0, 2])
def test_attention_encoder_and_cross_three_tiers(kind):
    """T3 of 0 (encoder), 1 and around the 64-key trip in one batch, Tpad 130 / 131 (the last block's waves clamp), padded rows, three GQA
    arrangements, both scales; rows behind T3[b] exact zeros; MS_MAX_KEYS keys on one head"""
    errors, worst = [], 0.0
    for c in mo.attn_launches(kind):
        d = mo.attn_case(c)
        st, out = mo.run_attn(d)
        if st != OK or np.any(out == 0xFFFF):
            errors.append(f"status {st} or poison left {_tag(c)}")
            continue
        if c["tier"] == "gaussian":
            ref, bound = mo.attn_reference(d)
            worst = max(worst, _bound_check(mo.val(out), ref, bound, _tag(c), errors))
        elif not np.array_equal(out, mo.bits(mo.attn_exact_expected(d))):
            errors.append("exact tier differs " + _tag(c))
    record(f"moonshine_ops_attn_kind{kind}_gauss", fraction_of_bound=worst)
    _fail(errors)


def test_attention_self_every_position_whole_cache():
    """positions 0, 1, around both 64-key trips, 200 and MS_MAX_POS - 1; RoPE at pos; the caches hold NaN behind pos and come back whole: row pos
    is the rotated k and v, written once per kv head, every other byte unchanged"""
    errors, worst = [], 0.0
    for c in mo.attn_launches(1):
        d = mo.self_case(c)
        st, out, kc, vc = mo.run_self(d)
        ref, bound, kc_ref, vc_ref = mo.self_reference(d)
        if st != OK or np.any(out == 0xFFFF):
            errors.append(f"status {st} or poison left {_tag(c)}")
            continue
        if not np.array_equal(kc, kc_ref) or not np.array_equal(vc, vc_ref):
            errors.append("the caches differ (row pos, or a byte elsewhere) " + _tag(c))
        if c["tier"] == "gaussian":
            worst = max(worst, _bound_check(mo.val(out), ref, bound, _tag(c), errors))
        elif not np.array_equal(out, mo.bits(ref)):
            errors.append("exact tier differs " + _tag(c))
    record("moonshine_ops_attn_self_gauss", fraction_of_bound=worst)
    _fail(errors)


# ------------------------------------------------------------------------------------------------ decode-step GEMM
def _gemv_sweep(ln, epi, errors, seen):
    shares = []
    for c in mo.gemv_cases(ln, epi):
        d = mo.gemv_case(c)
        st, out, rep = mo.run_gemv(d)
        if st != OK or rep != (ln, epi):
            errors.append(f"status {st}, ran {rep} {_tag(c)}")
            continue
        seen.add(rep)
        ref, silu, _ = mo.gemv_reference(d)
        if epi == mo.MS_F32:
            if not np.array_equal(out.view(np.uint32), ref.astype(np.float32).view(np.uint32)):
                errors.append("float32 sums differ (or poison left) " + _tag(c))
            continue
        if np.any(out == 0xFFFF):
            errors.append("poison left " + _tag(c))
        elif silu is None:
            if not np.array_equal(out, mo.bits(ref)):
                errors.append("output differs " + _tag(c))
        else:
            ex, lo_alt, hi_alt = silu
            got = mo.val(out)
            bad = (got != ref) & ~(ex & ((got == lo_alt) | (got == hi_alt)))
            shares.append((int(ex.sum()), int((got != ref).sum()), ex.size))
            if bad.any():
                errors.append(f"gate output differs off a SiLU rounding boundary ({int(bad.sum())} elements) " + _tag(c))
    return shares


@pytest.mark.parametrize("ln,epi", mo.GEMV_INST)
def test_gemv_every_instantiation_every_edge(ln, epi):
    """B around the eight-row register group and at 64 (LN, K = 512: the full LDS footprint), K / 4 below, at and off the 64 lanes, N of one
    wave, one block and more, bias and none; MS_RESID in place; exact LayerNorm rows whose statistics differ row by row"""
    errors, seen = [], set()
    shares = _gemv_sweep(ln, epi, errors, seen)
    if seen != {(ln, epi)}:
        errors.append(f"the report word names {sorted(seen)}")
    if shares:                                                       # the SiLU cap over the sweep's elements (a case of F = 1 has too few of its own)
        n = sum(s[2] for s in shares)
        record("moonshine_ops_gemv_gate", exempt_share=sum(s[0] for s in shares) / n, share_differing=sum(s[1] for s in shares) / n, elements=n)
        if sum(s[0] for s in shares) / n > mo.SILU_SHARE:
            errors.append("the exempt share of the gate sweep passes the cap")
    _fail(errors)


def test_gemv_every_instantiation_ran():
    errors, seen = [], set()
    for ln, epi in mo.GEMV_INST:
        c = mo.gemv_cases(ln, epi)[0]
        st, _, rep = mo.run_gemv(mo.gemv_case(c))
        assert st == OK, (st, c)
        seen.add(rep)
    assert seen == set(mo.GEMV_INST), sorted(set(mo.GEMV_INST) - seen)


@pytest.mark.parametrize("ln,epi", mo.GEMV_INST)
def test_gemv_gaussian_data_within_the_float32_summation_bound(ln, epi):
    """what integer data and zero-mean rows cannot catch: accumulation in less than float32, a LayerNorm that forgets its mean.  Gaussian x of
    mean 0.5, w and bias with full bf16 mantissas; the LN instantiations against the float64 LayerNorm"""
    errors, worst = [], 0.0
    for c in mo.gemv_cases(ln, epi)[::5]:
        d = mo.gemv_case(c, gauss=True)
        st, out, rep = mo.run_gemv(d)
        ref, bound = mo.gemv_gauss_reference(d)
        if st != OK or rep != (ln, epi):
            errors.append(f"status {st} {_tag(c)}")
            continue
        got = out.astype(np.float64) if epi == mo.MS_F32 else mo.val(out)
        worst = max(worst, _bound_check(got, ref, bound, _tag(c), errors))
    record(f"moonshine_ops_gemv_gauss_ln{ln}_epi{epi}", fraction_of_bound=worst)
    _fail(errors)


# ------------------------------------------------------------------------------------------------ embed, arg-max + embed
def test_embed_rows_and_out_of_range_ids():
    emb, ids = mo.embed_case()
    st, h = mo.run_embed(emb, ids)
    assert st == OK and np.array_equal(h, mo.embed_reference(emb, ids))


@pytest.mark.parametrize("V", mo.ARGMAX_V)
def test_argmax_embed_corner_rules(V):
    """the maximum at id 0, at V - 1 and in every wave's stride, a tie across waves, NaN and -inf rows, EOS on active and inactive rows,
    an inactive row, n_gen == stride: every output of the launch bit for bit"""
    c = mo.argmax_case(V)
    st, active, n_gen, tokens, done, h = mo.run_argmax_embed(c)
    ra, rn, rt, rd, rh, ids = mo.argmax_reference(c)
    assert st == OK
    errors = [name for name, got, want in (("active", active, ra), ("n_gen", n_gen, rn), ("tokens", tokens, rt), ("done_count", done, rd), ("h", h, rh))
              if not np.array_equal(got, want)]
    assert np.array_equal(ids, c["want"])
    assert not errors, (errors, n_gen, rn, tokens, rt, done, rd)


# ------------------------------------------------------------------------------------------------ the contract
def test_entry_points_refuse_what_the_kernels_exclude():
    errors = []

    def refuse(name, st):
        if st != INVALID:
            errors.append(f"{name}: status {st}")
    g = mo.gemv_case(dict(ln=1, epi=mo.MS_BF16, B=8, K=256, N=4, bias=True, seed=1))
    refuse("K % 4", mo.run_gemv(g, K=254)[0])
    refuse("B > 64", mo.run_gemv(g, B=65)[0])
    refuse("an instantiation the decoder does not use", mo.run_gemv(g, ln=0, epi=mo.MS_BF16)[0])
    big = mo.gemv_case(dict(ln=0, epi=mo.MS_RESID, B=2, K=516, N=4, bias=False, seed=2))
    big["lnw"] = np.ones(516)
    refuse("LN with K > 512", mo.run_gemv(big, ln=1, epi=mo.MS_BF16)[0])
    a = mo.attn_case(mo.attn_launches(0)[0])
    refuse("T3 > MS_MAX_KEYS", mo.run_attn(a, T3=np.r_[a["T3"][:-1], mo.MAX_KEYS + 1])[0])
    refuse("T3 > Tpad", mo.run_attn(a, T3=np.r_[a["T3"][:-1], a["Tpad"] + 1])[0])
    refuse("H % Hkv", mo.run_attn(a, Hkv=3)[0])
    x = mo.attn_case(mo.attn_launches(2)[0])
    refuse("cross-attention without a key", mo.run_attn(x, T3=np.r_[0, x["T3"][1:]])[0])
    s = mo.self_case(mo.attn_launches(1)[0])
    refuse("pos >= Smax", mo.run_self(s, pos=s["Smax"])[0])
    refuse("Smax > MS_MAX_POS", mo.run_self(s, Smax=mo.MAX_POS + 1)[0])
    r = mo.rope_case(mo.rope_cases()[0])
    refuse("odd rot", mo.run_rope(r, rot=31)[0])
    c1 = mo.conv1_case(mo.conv1_cases()[0])
    refuse("conv1 frames behind the stride", mo.run_conv1(c1, stride=c1["stride"] - 200)[0])
    gn = mo.gn_case()
    refuse("GroupNorm row without a frame", mo.run_groupnorm(gn, T1=np.r_[0, gn["T1"][1:]])[0])
    _fail(errors)
