"""The private kernels of csrc/lasr.hip as OPERATORS: k_lasr_gemm with its five epilogues on both tile sizes, k_lasr_ln, k_lasr_rope, k_lasr_attn,
k_lasr_glu_dwconv, k_lasr_im2col, k_lasr_pack, k_lasr_argmax and k_lasr_collapse, one launch at a time through the mis_debug_lasr_* entry
points at the end of csrc/lasr.hip, against the float64 specification of tests/lasr_ops_ref.py (its claims are proven in
tests/test_lasr_ops_ref_cpu.py).  Inputs whose result is exact are compared BIT FOR BIT - a key too many in the masked tile, a depthwise tap
from the wrong side of an even k, a bias shifted by a column, a residual read from the wrong buffer or a token lost at a chunk boundary
cannot hide behind a tolerance; SiLU is held to the boundary rule, Gaussian data to the derived bounds.  Rows behind a row count hold NaN
and must come back as exact zeros.  Every launch asserts its status, the instantiation the restated rule names, that no poison (0xFFFF) is
left where the kernel must write and that it is intact where it must not (the entry points fail on a touched guard or padding column)."""
import functools

import numpy as np
import pytest

import attn_ref as ar
import enc_ref as er
import gemm_ref as gr
import lasr_ops_ref as lo
from gpu_util import record

pytestmark = pytest.mark.gpu
OK = lo.OK


def _val(bits):
    return gr.bf16_value(bits).astype(np.float64)


def _same(bits, want64):
    return np.array_equal(bits, gr.bf16_bits(np.asarray(want64, np.float64).astype(np.float32)).reshape(bits.shape))


def _poison(bits):
    return bool(np.any(bits == 0xFFFF))


def _fail(errors):
    assert not errors, f"{len(errors)} failures, first: " + "\n".join(str(e) for e in errors[:8])


class Silu:
    """the observed side of the SiLU rule, recorded per test"""

    def __init__(self):
        self.share, self.worst, self.bad, self.n = 0.0, 0, 0, 0

    def hold(self, got_bits, want, exempt, live, tag, errors):
        """live: the elements of live rows (broadcastable); shares are over those"""
        ok, share, worst, n = lo.rule_holds(_val(got_bits), want, exempt, live)
        es = lo.exempt_share(exempt, live)
        print(f"SiLU {tag}: {n} live elements, exempt {es:.5f}, differing {share:.5f}, worst {worst} ulp")
        self.share, self.worst = max(self.share, share), max(self.worst, worst)
        self.bad += int(round(share * n)); self.n += n
        if not ok or es > lo.SILU_SHARE:
            errors.append(f"SiLU: differs off a rounding boundary or by more than one bf16 ulp ({worst}), exempt share {es:.4f} " + tag)

    def record(self, name):
        record(name, worst_ulp=self.worst, worst_case_share_differing=self.share, share_differing=self.bad / max(self.n, 1), elements=self.n)


# ------------------------------------------------------------------------------------------------ GEMM
def _gemm_one(c, tile, errors, silu, seen, d=None):
    tag = str({k: v for k, v in c.items() if k != "seed"}) + f" tile {tile}"
    d = lo.gemm_inputs(c) if d is None else d
    want = lo.gemm_expected(c["epi"], c["M"], c["N"], c["K"], c["ldx"], tile)
    st, out, Ra, rep = lo.run_gemm(c, d, tile)
    if st != OK or rep != want:
        errors.append(f"status {st}, ran {rep}, the launcher's rule says {want}: {tag}")
        return None
    seen.add(rep)
    ref, ex = lo.gemm_reference(c, d)
    if c["epi"] == lo.LG_F32:
        if np.isnan(out).any() or not np.array_equal(out.astype(np.float64), ref):
            errors.append("float32 output differs (or poison left) " + tag)
        return out
    if _poison(out):
        errors.append("poison left (element never written) " + tag)
        return out
    if Ra is not None and not np.array_equal(Ra, d["Rb"]):
        errors.append("the separate R buffer was written " + tag)
    if c["epi"] == lo.LG_SILU:
        silu.hold(out, ref, ex, d["live"][:, None], tag, errors)
    elif not _same(out, ref):
        errors.append("output differs " + tag)
    return out


@functools.lru_cache(maxsize=None)
def _gemm_sweep(epi):
    errors, seen, silu = [], set(), Silu()
    for c in lo.gemm_cases(epi):
        d = lo.gemm_inputs(c)
        o2, o4 = _gemm_one(c, 2, errors, silu, seen, d), _gemm_one(c, 4, errors, silu, seen, d)
        if o2 is not None and o4 is not None and not np.array_equal(o2.view(np.uint8), o4.view(np.uint8)):
            errors.append(f"the 64- and the 128-tile give different bits: {c}")
    if epi == lo.LG_SILU:
        silu.record("lasr_ops_gemm_silu")
    return errors, seen


@pytest.mark.parametrize("epi", range(5))
def test_gemm_every_epilogue_both_tiles_every_edge(epi):
    """M and N around both tile sizes, N % 16 in {4, 8, 12} (LG_F32: odd N), K of one, two, three and nine slabs, dense and padded rows, bias and
    none, row counts that mask rows inside a tile and a whole tile (X and R hold NaN there), AXPBY in place and with a separate R; the same
    operands through both tiles give the same bits, LG_SILU included"""
    errors, _ = _gemm_sweep(epi)
    _fail(errors)


def test_gemm_every_instantiation_ran():
    seen = set()
    for epi in range(5):
        seen |= _gemm_sweep(epi)[1]
    assert seen == lo.GEMM_INSTANTIATIONS, sorted(lo.GEMM_INSTANTIATIONS - seen)


def test_gemm_launcher_rule_switches_at_256_blocks():
    errors, seen = [], set()
    for c in lo.THRESHOLD_CASES:
        _gemm_one(c, 0, errors, None, seen)
    _fail(errors)
    assert seen == {(lo.LG_BIAS, 4), (lo.LG_BIAS, 2)}


def test_gemm_refused_shapes_launch_nothing():
    base = dict(epi=lo.LG_BIAS, M=8, N=8, K=64, ldx=64, bias=True, mask=0, in_place=False, a=0.0, b=0.0, seed=1)
    d = lo.gemm_inputs(dict(base, K=96, ldx=104))
    assert lo.run_gemm(base, d, 0)[0] == OK
    for kw in (dict(K=48, ldx=48), dict(ldx=68), dict(N=6), dict(epi=lo.LG_SILU, N=2)):
        c = dict(base, **kw)
        st, _, _, rep = lo.run_gemm(c, d, 2)
        assert (st, rep[0]) == (lo.GENERATION_FAILED, -1) and lo.gemm_expected(c["epi"], c["M"], c["N"], c["K"], c["ldx"])[0] == "err", (kw, st, rep)
    st, _, _, rep = lo.run_gemm(dict(base, epi=lo.LG_F32, N=6), d, 0)          # any N for the float32 epilogue
    assert (st, rep) == (OK, (lo.LG_F32, 2))
    st, _, _, rep = lo.run_gemm(dict(base, epi=lo.LG_AXPBY), d, 0)             # an epilogue without its R: the entry point's refusal
    assert (st, rep[0]) == (lo.INVALID_INPUT, -1)


@pytest.mark.parametrize("tile", [2, 4])
def test_gemm_gaussian_within_the_float32_summation_bound(tile):
    """|dev - ref64| <= delta (1 + 2^-8) + 2^-8 |ref|, delta = 2 gamma_K sum_k |x_k| |w_k| (gemm_ref's float32 summation bound; the second
    term: half a bf16 ulp of the perturbed value)"""
    K, M, N = 288, 129, 132
    rng = np.random.default_rng(K + tile)
    gam = 2.0 * (K * lo.U) / (1.0 - K * lo.U)
    x, w = lo.T(rng.standard_normal((M, K))), lo.T(0.05 * rng.standard_normal((N, K)))
    c = dict(epi=lo.LG_BIAS, M=M, N=N, K=K, ldx=K, in_place=False, a=0.0, b=0.0)
    st, out, _, rep = lo.run_gemm(c, dict(img=gr.exact_bits(x).reshape(-1), w=w, bias=None, cnt=None, Tp=1), tile)
    assert st == OK and rep == (lo.LG_BIAS, tile) and not _poison(out)
    ref, delta = x @ w.T, gam * (np.abs(x) @ np.abs(w).T)
    ratio = float((np.abs(_val(out) - ref) / (delta * (1 + 2.0 ** -8) + 2.0 ** -8 * np.abs(ref))).max())
    record(f"lasr_ops_gemm_gaussian_tile{tile}", fraction_of_bound=ratio)
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ LayerNorm
def test_layernorm_exact_tiers_bound_and_masked_rows():
    errors, worst = [], 0.0
    for d in lo.LN_D:
        for M in lo.LN_M:
            for masked in (False, True):
                tag = f"d = {d}, M = {M}, counts {masked}"
                cnt, Tp = lo.ln_counts(M, d + M) if masked else (None, 1)
                live = lo.live_rows(M, cnt, Tp)[:, None]
                x, w, b = er.ln_constant(M, d, d + M)
                st, y = lo.run_ln(lo.bits_nan(x, ~live), w, b, cnt=cnt, Tp=Tp)
                if st != OK or not _same(y, np.where(live, np.broadcast_to(b, x.shape), 0.0)):
                    errors.append(f"constant rows: status {st} or y != b " + tag)
                x, w, b, a = er.ln_balanced(M, d, 3 * d + M)
                st, y = lo.run_ln(lo.bits_nan(x, ~live), w, b, cnt=cnt, Tp=Tp)
                if st != OK or not _same(y, np.where(live, er.ln_balanced_expected(x, w, a), 0.0)):
                    errors.append(f"balanced rows differ (status {st}) " + tag)
                x, w, b = er.ln_gauss(M, d, 50 + d + M)
                st, y = lo.run_ln(lo.bits_nan(x, ~live), w, b, cnt=cnt, Tp=Tp)
                ref, bound = er.ln_reference(x, w, b)
                if st != OK or _poison(y) or np.any(y[~live[:, 0]] != 0):
                    errors.append(f"gaussian rows: status {st}, poison left or a masked row not zero " + tag)
                    continue
                r = float((np.abs(_val(y) - ref) / bound)[live[:, 0]].max(initial=0.0))
                worst = max(worst, r)
                if r > 1.0:
                    errors.append(f"gaussian rows: {r:.3f} of the bound " + tag)
    record("lasr_ops_layernorm", fraction_of_bound=worst)
    _fail(errors)


# ------------------------------------------------------------------------------------------------ RoPE
def _rope_rows(rng, M, ld, nheads):
    rows = gr.exact_bits(ar.grid_bf16(rng.standard_normal((M, ld)))).copy()
    behind = rows[:, nheads * lo.HD:]
    behind[:, ::3] = lo.NAN_PAYLOADS[rng.integers(0, 4, behind[:, ::3].shape)]          # V and padding: NaN payloads too
    return rows


def test_rope_exact_with_dyadic_tables_bounded_with_gaussian_ones():
    """Gaussian cos / sin (exact in float32) rather than a real table: position 0 and the high dimensions of a real table are (1, ~0), nearly the
    identity, while a Gaussian table puts every element under the fused / unfused pair bound"""
    errors, worst = [], 0.0
    for i, nheads in enumerate([1, 3, 5]):
        Tp, M = 7, 23 + 2 * i                                   # M crosses Tp three times; M nheads is odd
        ld = nheads * lo.HD + [8, 64, 136][i]
        rng = np.random.default_rng(32000 + i)
        rows = _rope_rows(rng, M, ld, nheads)
        for kind in ("dyadic", "gaussian"):
            cs, sn = ar.dyadic_tables(rng, Tp, lo.HD) if kind == "dyadic" else lo.gauss_tables(rng, Tp)
            st, got = lo.run_rope(rows, nheads, Tp, cs, sn)
            tag = f"nheads {nheads}, ld {ld}, M {M}, {kind} tables"
            if st != OK or not np.array_equal(got[:, nheads * lo.HD:], rows[:, nheads * lo.HD:]):
                errors.append(f"status {st} or a column behind the rotated heads changed " + tag)
                continue
            y, bound = lo.rope_reference(_val(rows), nheads, Tp, cs, sn)
            head = got[:, :nheads * lo.HD]
            if kind == "dyadic":
                if not _same(head, lo.T(y)):
                    errors.append("rotated heads differ " + tag)
            else:
                r = float((np.abs(_val(head) - y) / bound).max())
                worst = max(worst, r)
                if _poison(head) or r > 1.0:
                    errors.append(f"{r:.3f} of the bound " + tag)
    record("lasr_ops_rope_gaussian_tables", fraction_of_bound=worst)
    _fail(errors)


# ------------------------------------------------------------------------------------------------ attention
def test_attention_every_count_every_tier():
    """cnt around the 16-query and 32-key tiles, Tp = cnt, cnt + 1 and 130 (query blocks wholly behind cnt), three rows of different counts,
    GQA, padded rows; qkv rows behind cnt hold NaN (uniform tier: stale keys with zero values)"""
    errors, worst = [], 0.0
    for spec in lo.attn_launches():
        c = lo.attn_case(spec)
        tag = str(spec)
        st, out = lo.run_attn(c)
        if st != OK or _poison(out):
            errors.append(f"status {st} or poison left " + tag)
            continue
        dead = (np.arange(c["Tp"])[None, :] >= c["cnt"][:, None]).reshape(-1)
        if np.any(out[dead] != 0):
            errors.append("a query behind cnt is not zero " + tag)
        if c["tier"] == "gaussian":
            ref, bound = lo.attn_reference(c)
            r = float((np.abs(_val(out) - ref)[~dead] / bound[~dead]).max())
            worst = max(worst, r)
            if not r <= 1.0:
                errors.append(f"{r:.3f} of the bound " + tag)
        elif not _same(out, lo.attn_exact_expected(c)):
            errors.append("output differs " + tag)
    record("lasr_ops_attention_gaussian", fraction_of_bound=worst)
    _fail(errors)


# ------------------------------------------------------------------------------------------------ GLU + depthwise conv
def test_glu_dwconv_exact_tiers_every_k():
    """k odd and even up to LS_DW_MAXK, channel blocks with dead lanes, counts around the 64-frame tile, pw rows behind cnt NaN; dense integers and
    impulses that give every tap its own power of two; ReLU bit for bit, SiLU by the boundary rule"""
    errors, silu, acts = [], Silu(), set()
    for spec in lo.dw_launches():
        d = lo.dw_case(spec)
        tag = str(spec)
        st, out, rep = lo.run_glu_dwconv(d)
        if st != OK or rep != d["act"] or _poison(out):
            errors.append(f"status {st}, ran act {rep}, or poison left " + tag)
            continue
        acts.add(rep)
        ref, ex, _ = lo.dw_reference(d)
        if np.any(out[~d["live"].reshape(-1)] != 0):
            errors.append("a frame behind cnt is not zero " + tag)
        if d["act"] == 1:
            if not _same(out, ref):
                errors.append("output differs " + tag)
        else:
            silu.hold(out, ref, ex, d["live"].reshape(-1, 1), tag, errors)
    silu.record("lasr_ops_dwconv_silu")
    _fail(errors)
    assert acts == {0, 1}


def test_glu_dwconv_gaussian_gate_and_summation():
    """g = T(a sigmoid(gate)) is read back through k = 1 launches with taps +1 and -1 (max(g, 0) and max(-g, 0)) and held to the boundary rule;
    Gaussian taps over k frames are held to the float32 summation bound"""
    errors, gate = [], Silu()
    d = lo.dw_case(lo.DW_GATE_PROBE)
    _, _, g, _ = lo.dw_pre(d)
    _, ex = lo.near_boundary(d["a"] * lo.sigmoid64(d["gate"]), lo.margin(d["gate"]))
    live = d["live"][:, :, None]
    g, ex = g.reshape(-1, d["C"]), (ex & live).reshape(-1, d["C"])
    one = np.ones((1, d["C"]), np.float32)
    stp, pos, _ = lo.run_glu_dwconv(d, taps=one)
    stn, neg, _ = lo.run_glu_dwconv(d, taps=-one)
    assert stp == OK and stn == OK and not _poison(pos) and not _poison(neg)
    gate.hold(gr.exact_bits(_val(pos) - _val(neg)), g, ex, d["live"].reshape(-1, 1), "the gate", errors)
    gate.record("lasr_ops_dwconv_gate")
    worst = 0.0
    for spec in lo.DW_GAUSS:
        d = lo.dw_case(spec)
        st, out, rep = lo.run_glu_dwconv(d)
        ref, _, delta = lo.dw_reference(d)
        if st != OK or rep != 1 or _poison(out) or np.any(out[~d["live"].reshape(-1)] != 0):
            errors.append(f"status {st}, poison left or a frame behind cnt not zero {spec}")
            continue
        r = float((np.abs(_val(out) - ref) / (delta * (1 + 2.0 ** -8) + 2.0 ** -8 * np.abs(ref) + 1e-300)).max())
        worst = max(worst, r)
        if not r <= 1.0:
            errors.append(f"{r:.3f} of the bound {spec}")
    record("lasr_ops_dwconv_gaussian", fraction_of_bound=worst)
    _fail(errors)


# ------------------------------------------------------------------------------------------------ im2col, pack
def test_im2col_and_pack_are_pure_moves():
    errors = []
    for i, (ks, st_) in enumerate(lo.IM2COL_KS_ST):
        for Cc in lo.IM2COL_C:
            c = lo.im2col_case(ks, st_, Cc, 36000 + 10 * i + Cc)
            st, out = lo.run_im2col(c)
            if st != OK or not np.array_equal(out, lo.im2col_reference(c)):
                errors.append(f"im2col: status {st} or output differs: ks {ks}, st {st_}, C {Cc}")
    for mels, Kp in ((40, 64), (80, 96), (32, 32)):
        feats = er.im2col_f32_values((3, 9, mels), 36100 + mels)
        F = [9, 0, 4]
        st, out = lo.run_pack(feats, F, Kp)
        if st != OK or not np.array_equal(out, lo.pack_reference(feats, F, Kp)):
            errors.append(f"pack: status {st} or output differs: mels {mels}, Kp {Kp}")
    _fail(errors)


# ------------------------------------------------------------------------------------------------ the CTC tail
def test_argmax_lowest_index_on_ties():
    errors = []
    for V in lo.ARGMAX_V:
        x = lo.argmax_rows(V, 37000 + V)
        st, pred = lo.run_argmax(x)
        if st != OK or not np.array_equal(pred, lo.argmax_reference(x)):
            errors.append(f"V {V}: status {st}, got {pred.tolist()}, want {lo.argmax_reference(x).tolist()}")
    _fail(errors)


def test_collapse_against_greedy_ctc():
    errors = []
    for c in lo.collapse_launches():
        st, tokens, ntok = lo.run_collapse(c["pred"], c["cnt"])
        wt, wn = lo.collapse_reference(c["pred"], c["cnt"])
        if st != OK or not np.array_equal(ntok, wn) or not np.array_equal(tokens, wt):
            errors.append(f"cnt {c['cnt'].tolist()}: status {st}, ntok {ntok.tolist()} (want {wn.tolist()}) or tokens differ / a slot behind ntok written")
    _fail(errors)
