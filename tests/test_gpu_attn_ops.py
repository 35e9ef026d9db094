"""The decode-attention kernels as OPERATORS: k_attn_decode<D, NIT, XS, QP> and k_attn_decode2<NS> (csrc/lm_kernels.hip), one
launch_attn_decode call at a time through mis_debug_attn_decode on inputs whose result is known (tests/attn_ref.py, proven on the CPU in
tests/test_attn_ref_cpu.py).  Every launch asserts the instantiation that ran, the output (bit for bit in the locator and uniform tiers,
within the derived bound in the Gaussian tier; rows the launch must not write still poisoned), and the WHOLE cache images afterwards (the
image before plus exactly the new key and value; untouched by cross-attention).  The two schedules, and the cross-attention loop with and
without XS, must agree bit for bit."""
import functools

import numpy as np
import pytest

import attn_ref as ar
import gemm_ref as gr
from gpu_util import record

pytestmark = pytest.mark.gpu
OK = ar.OK


def _u16(a):
    return gr.bf16_bits(np.asarray(a, np.float32))


def _same_bits(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(_u16(np.where(na, 0, a)), _u16(np.where(nb, 0, b)))


def _check(c, res, errors, ratios, xs_on=True):
    """the four asserts every launch gets; appends to errors, records error / bound per tier in ratios"""
    st, out, kout, vout, hout, rep = res
    name, B, H, D, Hkv, Smax = c["name"], c["batch"], c["H"], c["D"], c["Hkv"], c["Smax"]
    want_rep = ar.expected(c, xs_on)
    if st != OK or rep != want_rep:                                                   # 1. the instantiation
        errors.append(f"{name}: status {st}, ran {rep}, the launcher's rule says {want_rep}")
        return
    r = ar.reference(c)
    if not np.isnan(out[B:]).all() or not np.isnan(out[:B][~c["active"].astype(bool)]).all():       # 2. the output
        errors.append(f"{name}: a row the launch must not write lost its poison")
    got, ref = out[:B].astype(np.float64), r["out"]
    m = ~np.isnan(ref)
    if np.isnan(got[m]).any():
        errors.append(f"{name}: NaN in an active row (element never written, an input over-read, or a non-finite product)")
    elif c["tier"] == "locator":
        if not _same_bits(got, ar.T(ref)):
            errors.append(f"{name}: locator output differs in {int((_u16(got[m]) != _u16(ar.T(ref)[m])).sum())} elements")
    elif c["tier"] == "uniform":
        if not _same_bits(got, ar.uniform_expected(c, r)):
            errors.append(f"{name}: uniform output differs in {int((_u16(got[m]) != _u16(ar.uniform_expected(c, r)[m])).sum())} elements")
    else:
        bound = r["bound"] if c["exact"] else r["wide"]
        ratio = float((np.abs(got - ref)[m] / bound[m]).max()) if m.any() else 0.0
        key = "gauss_exact" if c["exact"] else "gauss_widened"
        ratios[key] = max(ratios.get(key, 0.0), ratio)
        if ratio > 1.0:
            errors.append(f"{name}: |out - ref| is {ratio:.3f} of the bound")
    rows = c["cache_rows"] or B                                                       # 3. / 4. the caches
    vwant = ar.bits_of(ar.v_to_image(r["V"])).reshape(-1)
    if not np.array_equal(vout.reshape(-1), vwant):
        errors.append(f"{name}: V^T image differs from before + the new values in {int((vout.reshape(-1) != vwant).sum())} elements")
    kwant = ar.bits_of(ar.k_to_image(r["K"])).reshape(-1)
    if c["exact"] or c["cross"]:
        if not np.array_equal(kout.reshape(-1), kwant):
            errors.append(f"{name}: K image differs from before + the new keys in {int((kout.reshape(-1) != kwant).sum())} elements")
    else:
        Kg = gr.bf16_value(ar.k_from_image(kout.reshape(rows, Hkv, Smax * D), Smax, D)).astype(np.float64)
        new = np.zeros((rows, Smax), bool)
        act = np.nonzero(c["active"])[0]
        new[act % rows, c["pos"][act]] = True
        keep = ~np.broadcast_to(new[:, None, :, None], Kg.shape)
        if not np.array_equal(_u16(Kg[keep]), _u16(r["K"][keep])):
            errors.append(f"{name}: K image changed outside the appended keys")
        d = gr.bf16_ulp_distance(Kg[act % rows, :, c["pos"][act]], r["knew"][act])
        share = float((d != 0).mean())
        ratios["key_share"] = max(ratios.get("key_share", 0.0), share)
        if d.max() > 1 or share > ar.KEY_SHARE_CAP:
            errors.append(f"{name}: appended key up to {int(d.max())} bf16 ulp off, {share:.4f} of its elements differ (cap {ar.KEY_SHARE_CAP})")
    if c["qp"]:
        want = np.where(c["active"].astype(bool)[:, None], r["h_new"], np.nan)
        if not _same_bits(hout, want):
            errors.append(f"{name}: qp_h_out differs (or is incomplete, or an inactive row was written)")


@functools.lru_cache(maxsize=None)
def _sweep():
    errors, ratios, seen, results = [], {}, set(), {}
    for c in ar.gpu_cases():
        res = ar.run(c)
        results[c["name"]] = res
        seen.add(res[5])
        _check(c, res, errors, ratios)
    for k, v in sorted(ratios.items()):
        record(f"attn_ops_{k}", fraction_of_bound=v)
    return errors, ratios, seen, results


def _of(prefixes):
    errors = _sweep()[0]
    return [e for e in errors if e.startswith(tuple(prefixes))]


def test_first_schedule_every_group_size_slab_count_and_edge_position():
    """D = 128 with G in {1, 3, 4, 6, 7, 12}, D = 64 with G in {1, 2, 14, 15, 16}; S in {1, 2, 5, 8}; positions 0, 1, 30 .. 33, 255 .. 257, 511,
    512, 543, 544 and Smax - 1 as rows of one launch; every slot pos & 31 in the locator tier; packed outputs at Mpad 16, 32, 48 and row-major"""
    e = _of(["d128_", "d64_"])
    assert not e, f"{len(e)} failures:\n" + "\n".join(e[:8])


def test_second_schedule_and_its_equality_with_the_first():
    """NS = 1 .. 4, G in {1, 3, 4}, waves with 0 .. 4 tiles, the new key's tile owned by wave 0, 7 and waves between, pos = Smax - 1 at Smax = 1024;
    each launch repeated with first_schedule = 1: outputs and both cache images bit-equal ("same arithmetic", the kernel's header).
    Observed on an MI355X: bit-equal.  (The one input for which the cache BITS differ, a -0.0 slab element at S = 1, is kept out of these
    cases and held by test_negative_zero_slab.)"""
    e = _of(["s2_"])
    results = _sweep()[3]
    for c in ar.gpu_cases():
        if c["name"].startswith("s2_"):
            c1 = dict(c, first_schedule=1)
            r1, r2 = ar.run(c1), results[c["name"]]
            if r1[0] != OK or r1[5] != ar.expected(c1) or r1[5][0] != 0 or r2[5][0] != 1:
                e.append(f"{c['name']}: first-schedule repeat: status {r1[0]}, ran {r1[5]}")
            elif not (_same_bits(r1[1], r2[1]) and np.array_equal(r1[2], r2[2]) and np.array_equal(r1[3], r2[3])):
                e.append(f"{c['name']}: the two schedules differ: {int((_u16(np.nan_to_num(r1[1])) != _u16(np.nan_to_num(r2[1]))).sum())} output elements, "
                         f"{int((r1[2] != r2[2]).sum())} K, {int((r1[3] != r2[3]).sum())} V")
    c = ar.build("s2_fallback_1056", "uniform", 128, 3, [0, 31, 500, 1055], S=2, Smax=1056, seed=77)
    errs, rat = [], {}
    res = ar.run(c)
    _check(c, res, errs, rat)
    assert res[5][0] == 0, res[5]                                       # 33 tiles: the first schedule
    assert not e and not errs, "\n".join((e + errs)[:8])


def test_negative_zero_slab():
    """a slab element that is -0.0 at S = 1: k_attn_decode sums the slabs from 0.0f (0.0f + -0.0f = +0.0f), k_attn_decode2<1> takes the single
    slab as it is (-0.0f) - the one step the two schedules order differently.  Each schedule is held to the reference: outputs bit for bit
    (uniform tier), both caches equal to the reference as NUMBERS everywhere and in bits wherever the reference is not a zero; the first
    schedule's zeros are +0 as the specification's sum from zero gives them."""
    for first in (1, 0):
        c = ar.build(f"negzero_{first}", "uniform", 128, 2, [0, 31, 32, 100], S=1, Smax=128, first_schedule=first, neg_zero=True, seed=88)
        st, out, kout, vout, _, rep = ar.run(c)
        assert st == OK and rep == ar.expected(c) and rep[0] == 1 - first
        r = ar.reference(c)
        assert _same_bits(out[:c["batch"]].astype(np.float64), ar.uniform_expected(c, r))
        for img, want in ((kout, ar.k_to_image(r["K"])), (vout, ar.v_to_image(r["V"]))):
            got, want = gr.bf16_value(img).astype(np.float64).reshape(-1), want.reshape(-1)
            assert np.array_equal(got, want)                                                   # -0.0 == +0.0
            nz = want != 0
            assert np.array_equal(img.reshape(-1)[nz], ar.bits_of(want)[nz])
            if first and img is vout:                                                          # (no arithmetic between the sum and the value's append)
                assert np.array_equal(img.reshape(-1), ar.bits_of(want))


def test_arithmetic_flavours_within_the_widened_bound():
    """Qwen3 q/k-norm at D = 128 and 64, rope_in_dtype, real cos / sin tables at theta 1e4 and 1e6, no RoPE at D = 64: output within the
    widened bound, the appended key within one bf16 ulp and under the CPU-derived share, nothing else of the caches changed"""
    e = _of(["qknorm_", "rope_in_dtype", "real_theta", "whisper_self"])
    assert not e, "\n".join(e[:8])


def test_prefill_pair_arrangement():
    """cache_rows = 3, 3 x 5 (position, sequence) rows: the append-only launch writes keys and values and leaves the output poisoned; the attending
    launch on the caches it left gives row (t, s) the reference over keys 0 .. t of sequence s"""
    a = ar.prefill_pair()
    errors, ratios = [], {}
    res = ar.run(a)
    _check(a, res, errors, ratios)
    assert res[0] == OK and np.isnan(res[1]).all(), "the append-only launch wrote an output"
    b = dict(a, append_only=0, name="prefill_attend", kimg=res[2], vimg=res[3])
    _check(b, ar.run(b), errors, ratios)
    record("attn_ops_prefill_pair", fraction_of_bound=ratios["gauss_exact"])
    assert not errors, "\n".join(errors)
    assert ratios["gauss_exact"] <= 1.0


def test_cross_attention_pair_loop_and_xs(monkeypatch):
    """cross_len 1, 31, 33, 200 on the pair loop; 1280, 1500, 1536 on XS (waves with 5, 5 or 6, 6 tiles), and the same with MIS_ATTN_XS=0 (read per
    launch): the pair loop must give the same bits ("results are bit-identical", the kernel's comment); caches untouched"""
    e = _of(["cross_", "xs_"])
    results = _sweep()[3]
    monkeypatch.setenv("MIS_ATTN_XS", "0")
    for c in ar.gpu_cases():
        if c["name"].startswith("xs_"):
            r0, r1 = ar.run(c), results[c["name"]]
            if r0[0] != OK or r0[5] != ar.expected(c, xs_on=False) or r0[5][3] != 0 or r1[5][3] != 1:
                e.append(f"{c['name']}: MIS_ATTN_XS=0: status {r0[0]}, ran {r0[5]}")
            elif not (_same_bits(r0[1], r1[1]) and np.array_equal(r0[2], r1[2]) and np.array_equal(r0[3], r1[3])):
                e.append(f"{c['name']}: XS and the pair loop differ in {int((_u16(np.nan_to_num(r0[1])) != _u16(np.nan_to_num(r1[1]))).sum())} output elements")
    assert not e, "\n".join(e[:8])


def test_query_projection_prologue():
    """H = Hkv in {2, 6, 20} (KT = 4: waves without a k-tile; 12; 40: five per wave), qp_S in {1, 4, 5, 8} (QP = 4 and 8), with and without bias:
    qp_h_out bit for bit and complete, the output within the widened bound, the caches untouched; KT = 41 is refused"""
    e = _of(["qp_"])
    assert not e, "\n".join(e[:8])
    c = next(c for c in ar.gpu_cases() if c["name"].startswith("qp_h20"))
    bad = dict(c, qp=dict(c["qp"], KT=41))
    st, _, _, _, _, rep = ar.run(bad)
    assert (st, rep[0]) == (ar.GENERATION_FAILED, -1) and ar.expected(bad) == ("err", ar.GENERATION_FAILED)


def test_inactive_rows_and_repeatability():
    """inactive rows between active ones at rows 0 .. 7 keep their output poison and their caches; a second launch on the same buffers gives the same bits"""
    e = _of(["inactive_"])
    assert not e, "\n".join(e[:8])
    results = _sweep()[3]
    for name in ("inactive_s2", "d128_g7_gauss", "xs_1500_gauss"):
        c = next(c for c in ar.gpu_cases() if c["name"] == name)
        a, b = results[name], ar.run(c)
        assert _same_bits(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), name


def test_rejected_shapes_launch_nothing():
    """a GQA group of 13 at D = 128 (the LDS footprint), a cache that is no whole number of 32-key tiles (either schedule), nine slabs: the
    launcher's status, nothing launched"""
    g13 = ar.build("g13", "uniform", 128, 13, [0, 5, 40], Smax=64, first_schedule=1, seed=9)
    s9 = ar.build("s9", "uniform", 128, 2, [0, 5, 40], S=9, Smax=64, first_schedule=1, seed=9)
    for first in (0, 1):
        t48 = ar.build("smax48", "uniform", 128, 2, [0, 5, 40], Smax=64, first_schedule=first, seed=9)
        t48["Smax"] = 48                                                # (images and tables of 64 positions: nothing is launched anyway)
        for bad in (g13, s9, t48):
            st, _, _, _, _, rep = ar.run(bad)
            want = ar.expected(bad)
            assert want[0] == "err" and (st, rep[0]) == (want[1], -1), (bad["name"], st, rep, want)


def test_every_instantiation_ran():
    """the reports seen across the file cover all eleven instantiations of launch_attn_decode, and NO case of the sweep failed - the tests above
    pick their cases' failures by name, this one takes them all"""
    errors, _, seen, _ = _sweep()
    assert not errors, f"{len(errors)} failures in the sweep (whatever their names), first:\n" + "\n".join(errors[:8])
    assert ar.INSTANTIATIONS <= seen, ar.INSTANTIATIONS - seen
    r = _sweep()[1]
    assert max(r.get("gauss_exact", 0.0), r.get("gauss_widened", 0.0)) <= 1.0, r
