"""What tests/test_gpu_moonshine_ops.py leans on, proven without a GPU: the exact generators of tests/moonshine_ops_ref.py give the same bits
under any float32 summation order, every planted fault changes the expected output of every case it applies to, no case compares zeros with
zeros only, the case tables name every instantiation and edge, and the measured / derived margins hold for float32 realisations on the CPU."""
import numpy as np
import pytest
import torch

import attn_ref as ar
import gemm_ref as gr
import lasr_ops_ref as lo
import moonshine_ops_ref as mo

f32 = np.float32


def _perm(seed):
    return lambda n: np.random.default_rng(seed).permutation(n)


# ------------------------------------------------------------------------------------------------ conv1
def test_conv1_exact_tier_any_order_saturates_and_sees_a_shifted_window():
    for c in mo.conv1_cases():
        d = mo.conv1_case(c)
        ref, bound = mo.conv1_reference(d)
        assert np.abs(ref).max() > 0.5 and not np.array_equal(ref, mo.conv1_reference(d, shift=1)[0])
        live = np.arange(d["T1pad"])[None] < d["T1"][:, None]
        assert not ref[~live].any() and ref[live].any(-1).all()                          # every live frame has a non-zero channel
        if c["tier"] != "exact":
            assert bound[live].min() > 0 and bound.max() < 1e-3
            continue
        assert set(mo.CONV1_TAPS) <= set(d["tap"].tolist())
        want = ref.astype(f32)
        assert set(np.unique(want).tolist()) == {-1.0, 0.0, 1.0}                         # float32 tanh(16) == 1: far inside the saturated range
        assert 1.0 - np.tanh(16.0) < 2.0 ** -25 * 1e-5 and float(torch.tanh(torch.tensor(16.0))) == 1.0 and float(np.tanh(f32(16.0))) == 1.0
        for order in (None, np.random.default_rng(1).permutation(127), np.arange(127)[::-1]):
            assert np.array_equal(mo.conv1_reference(d, order=order, dtype=f32)[0].astype(f32), want)
        # a stale sample read: the 3e4 behind the extent would reach a sum (the last frame's window ends where it begins)
        e = dict(d, pcm=np.where(d["pcm"] == mo.STALE_PCM, 0.0, d["pcm"]))
        assert np.array_equal(mo.conv1_reference(e)[0], ref)


def test_tanh_ulp_figure_is_the_measured_one():
    """the route taken: no accuracy table on the machine, so 4 x the distance of torch's float32 CPU tanh to float64 over tanh_probe()"""
    x = torch.from_numpy(mo.tanh_probe())
    t64 = torch.tanh(x.double()).numpy()
    dist = np.abs(torch.tanh(x).double().numpy() - t64) / mo.ulp_f32(t64)
    assert 0.5 <= dist.max() <= mo.TANH_CPU_ULP and mo.TANH_ULP == 4 * mo.TANH_CPU_ULP


# ------------------------------------------------------------------------------------------------ GroupNorm
def test_groupnorm_partials_exact_in_any_order_and_the_rule_covers_float32():
    c = mo.gn_case()
    ref = mo.gn_reference(c)
    assert c["nch"] == 3 and [-(-int(t) * c["d"] // mo.GN_CHUNK) for t in c["T1"]] == [1, 1, 2, 2, 3]
    assert 113 * c["d"] < mo.GN_CHUNK < 114 * c["d"]
    assert np.all(ref["stats"][:, 0] == 0) and np.abs(ref["part0"]).max() > 0 and np.all(ref["part1"][:, 0] > 0)
    assert np.all(ref["part0"][0, 1:] == 0) and np.all(ref["part1"][0, 1:] == 0)            # the short row's later chunks
    for seed in (1, 2):
        alt = mo.gn_reference(c, order=_perm(seed), dtype=f32)
        assert np.array_equal(alt["part0"], ref["part0"]) and np.array_equal(alt["part1"], ref["part1"])
    assert lo.exempt_share(ref["exempt"], ref["live"]) <= mo.SILU_SHARE                   # the reference alone stays within the cap
    assert np.abs(ref["y"][ref["live"]]).min() > 0 and not ref["y"][~ref["live"]].any()
    # float32 realisations of the affine (fused or not, rstd by a reciprocal or a division) leave the reference on exempt elements only
    B, d, Tp = c["B"], c["d"], c["T1pad"]
    for fused in (False, True):
        y = np.zeros_like(ref["y"])
        for b in range(B):
            n = int(c["T1"][b]) * d
            q = f32(ref["part1"][b].astype(f32).sum(dtype=f32) / f32(n))
            rstd = f32(1.0) / np.sqrt(f32(q + f32(1e-5)))
            x = c["x"].reshape(B, -1)[b, :n].astype(f32)
            p = (x * rstd).astype(f32)
            gw, gb = np.tile(c["gw"], n // d).astype(f32), np.tile(c["gb"], n // d).astype(f32)
            v = (p.astype(np.float64) * gw + gb).astype(f32) if fused else ((p * gw).astype(f32) + gb).astype(f32)
            y[b * Tp * d:b * Tp * d + n] = lo.b16(v)
        ok, share, worst, _ = lo.rule_holds(y, ref["y"], ref["exempt"], ref["live"])
        assert ok, (fused, share, worst)
    # statistics of the neighbouring row change the output
    wrong = mo.gn_reference(c, mean_of=lambda b: (b + 1) % B)
    assert not lo.rule_holds(wrong["y"], ref["y"], ref["exempt"], ref["live"])[0]


# ------------------------------------------------------------------------------------------------ RoPE
def test_rope_dyadic_is_exact_and_the_three_faults_show():
    assert sorted({c["rot"] for c in mo.rope_cases()}) == [32, 46, 56, 64] and {c["Tpad"] for c in mo.rope_cases()} == {1, 5}
    assert [mo.__dict__["ROPE_ROT"][i] for i in range(3)] == [max(2, int(h * 0.9) - int(h * 0.9) % 2) for h in (36, 52, 64)]
    for c in mo.rope_cases():
        d = mo.rope_case(c)
        assert d["M"] % 4 and d["M"] > d["Tpad"] and d["nheads"] * 64 < d["ld"] - 8
        want = mo.rope_reference(d)
        nh, rot = d["nheads"], d["rot"]
        x = d["x"][:, :nh * 64].reshape(d["M"], nh, 64)
        pos = np.arange(d["M"]) % d["Tpad"]
        y = mo.rope_pairs(x, d["cs"][pos][:, None], d["sn"][pos][:, None], rot)
        assert np.array_equal(mo.T(y), y) and np.abs(y).max() <= 16                    # representable: exact in float32, fused or not
        assert np.array_equal(want[:, nh * 64:], d["img"][:, nh * 64:])                   # v heads and padding
        assert np.array_equal(want[:, :nh * 64].reshape(-1, 64)[:, rot:], d["img"][:, :nh * 64].reshape(-1, 64)[:, rot:])
        assert np.any(want != d["img"])
        for mut in ("half_split", "pos") + (("at_rot",) if rot < 64 else ()):
            assert not np.array_equal(mo.rope_reference(d, mut), want), (c, mut)


# ------------------------------------------------------------------------------------------------ attention
def test_attention_tiers_are_exact_and_a_key_too_many_shows():
    for kind in (0, 2):
        cases = mo.attn_launches(kind)
        assert {c["heads"] for c in cases} >= set(mo.ATTN_HEADS) and {c["Tpad"] for c in cases} >= {130, 131}
        assert {(c["tier"], c["heads"]) for c in cases} >= {(t, h) for t in mo.ATTN_TIERS for h in mo.ATTN_HEADS}
        assert {round(c["scale"] ** -2) for c in cases} == {36, 64}
        assert all(sorted(c["T3"]) == ([0] if kind == 0 else []) + [1, 63, 64, 65, 129] for c in cases if c["Tpad"] < 1000)
        assert (kind == 0) == any(c["T3"] == [mo.MAX_KEYS] and c["heads"] == (1, 1) for c in cases)
        for c in cases:
            d = mo.attn_case(c)
            if c["tier"] == "gaussian":
                ref, bound = mo.attn_reference(d)
                assert np.abs(ref).max() > 1 and bound.max() < 0.02
                with np.errstate(invalid="ignore"):
                    off = mo.attn_reference(d, 1)[0]
                assert np.isnan(off).any() or np.abs(off - ref).max() > bound.max()
                continue
            want = mo.attn_exact_expected(d)
            assert np.abs(want).max() > 0 and np.array_equal(mo.T(want), want)
            if c["tier"] == "locator":
                # every other key scores at most half the target's: the float32 probability is exactly 0
                for b in range(d["B"]):
                    n = int(d["T3"][b])
                    if n < 2 or n > 200:
                        continue
                    s = d["scale"] * np.einsum("hqc,hkc->hqk", d["q"][b, :, :(n if kind == 0 else 1)], np.repeat(d["K"][b, :, :n], d["H"] // d["Hkv"], 0))
                    top = np.sort(s, -1)
                    assert np.all(top[..., -1] - top[..., -2] > 110) and np.exp(f32(-110.0)) * f32(2 ** 24) < 1e-40
                    assert np.array_equal(np.argmax(s, -1), d["targets"][b, :, :s.shape[1]])
            else:
                # the integer sum is exact in float32 in any order
                for b in range(d["B"]):
                    n = int(d["T3"][b])
                    if n:
                        v = d["V"][b, :, :n]
                        assert np.array_equal(np.cumsum(v[:, np.random.default_rng(b).permutation(n)].astype(f32), 1, dtype=f32)[:, -1], v.sum(1))
            if c["Tpad"] < 1000:
                with np.errstate(invalid="ignore"):
                    off = mo.T(mo.attn_reference(d, 1)[0])
                live = (np.arange(d["Tpad"])[None] < d["T3"][:, None]).reshape(-1) if kind == 0 else np.ones(d["B"], bool)
                assert not np.array_equal(off[live], want[live]), c


def test_self_attention_cases_cache_append_and_the_wrong_head():
    cases = mo.attn_launches(1)
    assert {c["pos"] for c in cases} == set(mo.SELF_POS) | {mo.MAX_POS - 1} and all(c["B"] == 3 and c["Smax"] == 201 for c in cases if c["pos"] <= 200)
    assert {(c["pos"], c["tier"]) for c in cases} >= {(p, t) for p in mo.SELF_POS for t in mo.ATTN_TIERS}
    for c in cases:
        d = mo.self_case(c)
        out, bound, kc, vc = mo.self_reference(d)
        pos = c["pos"]
        assert np.abs(out).max() > 0
        changed = (kc != d["kc"]) | (vc != d["vc"])
        assert changed[:, :, pos].any() and not changed[:, :, :pos].any() and not changed[:, :, pos + 1:].any()
        assert np.all(d["kc"][:, :, pos + 1:] == mo.NAN16)                                # NaN behind pos before the launch
        if d["Hkv"] > 1:
            assert not np.array_equal(mo.self_reference(d, wrong_head=True)[3], vc)
        if c["tier"] == "locator":
            assert np.array_equal(d["qr"], ar.locator_key(d["targets"], 64))              # the quarter turns are undone exactly
            assert (d["targets"] == pos).any() or d["H"] == 1
        elif c["tier"] == "gaussian":
            assert 0 < bound.max() < 0.02
        # RoPE of the new q and k is exact in float32: the unrounded values sit on a 2^-10 grid below 2^6
        for raw in (mo.val(d["qkv"][:, :(d["H"] + d["Hkv"]) * 64]).reshape(c["B"], -1, 64),):
            y = mo.rope_pairs(raw, d["cs"][pos], d["sn"][pos], c["rot"])
            assert np.array_equal(y.astype(f32).astype(np.float64), y) and np.array_equal(y * 1024, np.round(y * 1024))


# ------------------------------------------------------------------------------------------------ decode-step GEMM
def test_layernorm_rows_give_plus_minus_the_weight_in_float32():
    """T(x rstd lnw) == +-lnw under float32 statistics, for any bf16 lnw; another row's statistics change the bits"""
    rng = np.random.default_rng(5)
    for K in (4, 260, 512):
        X, sign = mo.ln_exact_rows(rng, 64, K)
        assert len({tuple(np.abs(r[:1])) for r in X}) == 64 and np.array_equal(mo.T(X), X)
        lnw = ar.grid_bf16(1.0 + 0.1 * rng.standard_normal(K))
        x = X.astype(f32)
        mean = (x.sum(1, dtype=f32) / f32(K))[:, None]
        assert not mean.any()
        q = ((x - mean) ** 2).astype(f32).sum(1, dtype=f32)
        assert np.array_equal(q.astype(np.float64), (X ** 2).sum(1))                     # the variance is exact
        for recip in (False, True):
            sd = np.sqrt((q / f32(K) + f32(1e-5)).astype(f32))
            xn = ((x - mean) * (f32(1.0) / sd)[:, None]).astype(f32) if recip else ((x - mean) / sd[:, None]).astype(f32)
            assert np.abs(np.abs(xn.astype(np.float64)) - 1).max() < 5.2e-6
            assert np.array_equal(lo.b16((xn * lnw.astype(f32)).astype(f32)).astype(np.float64), sign * lnw)
            wrong = lo.b16((((x - mean) / np.roll(sd, 1)[:, None]).astype(f32) * lnw.astype(f32)).astype(f32)).astype(np.float64)
            assert np.all((wrong != sign * lnw).any(1))


def test_gemv_tables_exactness_and_planted_faults():
    assert mo.GEMV_INST == [(1, mo.MS_BF16), (0, mo.MS_RESID), (1, mo.MS_GATE), (1, mo.MS_F32)]
    exempt = total = 0
    for ln, epi in mo.GEMV_INST:
        cases = mo.gemv_cases(ln, epi)
        assert {(c["B"], c["K"]) for c in cases} == {(b, k) for b in [1, 7, 8, 9, 33, 64] for k in [4, 252, 256, 260, 288, 416, 512]}
        assert {(c["B"], c["N"]) for c in cases} >= {(b, n) for b in mo.GEMV_B for n in [1, 4, 5, 131]}
        assert {(c["K"], c["N"]) for c in cases} >= {(k, n) for k in mo.GEMV_K for n in mo.GEMV_N}
        assert epi == mo.MS_F32 or {c["bias"] for c in cases} == {True, False}
        for c in cases:
            d = mo.gemv_case(c)
            ref, silu, _ = mo.gemv_reference(d)
            assert np.abs(ref).max() > 0 and np.abs(d["xs"] @ d["W"].T).max() < 2 ** 12, c
            for order in (np.random.default_rng(c["seed"]).permutation(c["K"]), np.arange(c["K"])[::-1]):
                assert np.array_equal(mo.gemv_reference(d, order=order, dtype=f32)[0], ref), c
            if silu is not None:
                exempt, total = exempt + int(silu[0].sum()), total + silu[0].size
                assert np.abs(mo.T(d["xs"] @ d["W"][c["N"]:].T + (0 if d["b"] is None else d["b"][c["N"]:]))).max() <= lo.SILU_VMAX
                a, sg = mo.T(d["xs"] @ d["W"][:c["N"]].T + (0 if d["b"] is None else d["b"][:c["N"]])), silu[1]
                assert np.array_equal((sg.astype(f32) * 1).astype(np.float64), sg)          # the product of two bf16 values is exact in float32
            muts = (["bias_shift"] if c["bias"] and d["rows"] > 1 else []) + (["gate_row"] if epi == mo.MS_GATE and c["N"] > 1 else []) + \
                   (["resid_row"] if epi == mo.MS_RESID and c["B"] > 1 else []) + (["repeat_last"] if c["B"] > 1 else [])
            for mut in muts:
                assert not np.array_equal(mo.gemv_reference(d, mut=mut)[0], ref), (c, mut)
    assert exempt / total <= mo.SILU_SHARE
    full = [c for c in mo.gemv_cases(1, mo.MS_BF16) if c["B"] == 64 and c["K"] == 512]
    assert full and full[0]["B"] * full[0]["K"] * 2 == 65536                              # the full LDS footprint


def _gemv_f32(d, no_mean=False):
    """the kernel's arithmetic in float32 numpy (numpy's own summation orders)"""
    xs = d["X"].astype(f32)
    if d["ln"]:
        K = d["K"]
        mean = np.zeros((d["B"], 1), f32) if no_mean else (xs.sum(1, dtype=f32) / f32(K))[:, None]
        t = (xs - mean).astype(f32)
        rstd = f32(1.0) / np.sqrt(((t * t).astype(f32).sum(1, dtype=f32) / f32(K) + f32(1e-5)).astype(f32))
        xs = lo.b16(((t * rstd[:, None]).astype(f32) * d["lnw"].astype(f32)).astype(f32))
    acc = (xs @ d["W"].astype(f32).T).astype(f32)
    if d["epi"] == mo.MS_F32:
        return acc.astype(np.float64)
    pre = acc if d["b"] is None else (acc + d["b"].astype(f32)[None]).astype(f32)
    v = lo.b16(pre)
    if d["epi"] == mo.MS_BF16:
        return v.astype(np.float64)
    if d["epi"] == mo.MS_RESID:
        return lo.b16((v + d["h"].astype(f32)).astype(f32)).astype(np.float64)
    N = d["N"]
    return lo.b16((lo.silu_f32(v[:, N:], 1).astype(f32) * v[:, :N]).astype(f32)).astype(np.float64)


def test_gemv_gaussian_bound_covers_float32_and_sees_a_forgotten_mean():
    """every instantiation has Gaussian cases with real Gaussian rows of non-zero mean; a float32 realisation stays inside the bound, one
    that forgets the mean (which every zero-mean exact row would let pass) leaves it; few elements may round either way"""
    for ln, epi in mo.GEMV_INST:
        for c in mo.gemv_cases(ln, epi)[::5]:
            d = mo.gemv_case(c, gauss=True)
            ref, bound = mo.gemv_gauss_reference(d)
            assert np.abs(d["X"].mean(1)).min() > 0.05 or c["K"] == 4
            assert np.all(np.abs(_gemv_f32(d) - ref) <= bound), c
            assert (d["slack"] > 0).mean() <= 0.01
            assert not np.array_equal(d["W"], ar.grid_bf16(d["W"], 2.0 ** -10)) or c["K"] * d["rows"] < 16   # full mantissas: the sums are not exact
            if ln and c["K"] >= 252:
                assert np.any(np.abs(_gemv_f32(d, no_mean=True) - ref) > bound), c
    assert any(c["B"] == 64 for c in mo.gemv_cases(1, 0)[::5]) and {c["K"] for c in mo.gemv_cases(1, 0)[::5]} >= {4, 252, 256, 512}


# ------------------------------------------------------------------------------------------------ embed, arg-max + embed
def test_embed_and_argmax_rules():
    emb, ids = mo.embed_case()
    assert {-1, mo.EMBED_VOCAB, 0, mo.EMBED_VOCAB - 1} <= set(ids.tolist()) and emb.shape[1] == 288
    want = mo.embed_reference(emb, ids)
    assert np.array_equal(want[0], emb[0]) and np.array_equal(want[1], emb[0]) and np.array_equal(want[3], emb[-1]) and not np.array_equal(emb[0], emb[-1])
    assert mo.ARGMAX_V == [255, 256, 257, 2049]
    for V in mo.ARGMAX_V:
        c = mo.argmax_case(V)
        active, n_gen, tokens, done, h, ids = mo.argmax_reference(c)
        row = {n: i for i, n in enumerate(mo.ARGMAX_ROWS)}
        assert np.array_equal(ids, c["want"]) and ids[row["max0"]] == 0 and ids[row["maxlast"]] == V - 1
        assert [(ids[row[f"wave{w}"]] % 256) // 64 for w in range(4)] == [0, 1, 2, 3]
        assert ids[row["tie"]] == 70 and mo.argmax_reference(c, highest=True)[5][row["tie"]] != 70
        assert ids[row["nan"]] == 0 and ids[row["neginf"]] == 0 and ids[row["nan_front"]] > V // 2
        assert done[0] - c["done"][0] == 2 and not active[row["eos"]] and not active[row["eos2"]] and c["active"][row["eos"]]
        assert np.array_equal(tokens[row["eos"]], c["tokens"][row["eos"]]) and n_gen[row["eos"]] == c["n_gen"][row["eos"]]
        for r in ("inactive", "eos_inactive"):
            assert np.array_equal(tokens[row[r]], c["tokens"][row[r]]) and n_gen[row[r]] == c["n_gen"][row[r]] and not active[row[r]]
        f = row["full"]
        assert c["n_gen"][f] == mo.ARGMAX_STRIDE and np.array_equal(tokens[f], c["tokens"][f]) and n_gen[f] == mo.ARGMAX_STRIDE + 1
        assert tokens[row["wave1"], c["n_gen"][row["wave1"]]] == 70 and np.array_equal(h, c["emb"][ids])


# ------------------------------------------------------------------------------------------------ the model, chained
def test_chained_operator_references_reproduce_the_model_reference():
    """moonshine_ref.MoonshineRef(round="bf16") with float64 sums and T() as its one rounding, heads padded to 64 as the engine loads them,
    against the operator specifications chained as ms_encode_device and the decoder step chain the kernels: one tiny config with GQA in both
    stacks, attention biases, an untied projection; the encoder output and three cached decoder steps.  A shared mistake of the specification
    and the kernel headers - the LayerNorm's eps or weight, the kv head of a group, the gate's half of fc1, the RoPE pairing - shows here."""
    import enc_ref as er
    import mlx_audio_swift_amd as mas
    import moonshine_ref as mr

    cfg = mas.MoonshineConfig(vocab_size=40, hidden_size=64, intermediate_size=96, encoder_num_hidden_layers=1, decoder_num_hidden_layers=1,
                              encoder_num_attention_heads=4, decoder_num_attention_heads=4, encoder_num_key_value_heads=2, decoder_num_key_value_heads=2,
                              attention_bias=True, tie_word_embeddings=False)
    W = mr.pad_heads(cfg, mr.make_weights(cfg, seed=11), 64)

    class Ref1(mr.MoonshineRef):
        def r(self, x):
            return torch.from_numpy(mo.T(x.double().numpy())) if self.round == "bf16" else x

    ref = Ref1(cfg, W, round="bf16", acc=torch.float64)
    audio = torch.randn(1700, generator=torch.Generator().manual_seed(12)) * 0.2
    want_enc = ref.encode(audio).numpy()

    d, H, Hk, hd = 64, 4, 2, 16
    rot, scale = mr.rotary_dim(hd, cfg.partial_rotary_factor), float(hd) ** -0.5
    w = lambda k: ref.w[k].double().numpy()
    E, D = "model.encoder", "model.decoder"
    gelu = lambda v: mo.T(er.gelu64(v))
    lin = lambda x, p, bias=True: mo.T(x @ w(p + ".weight").T + (w(p + ".bias") if bias else 0.0))     # the big GEMM's T(acc + bias)
    cat = lambda p, names, suf: np.concatenate([w(f"{p}.{n}.{suf}") for n in names])
    inv = 1.0 / torch.pow(torch.tensor(float(cfg.rope_theta)), torch.arange(0, rot, 2, dtype=torch.float32) / rot)
    ang = (torch.arange(8).float()[:, None] * inv[None]).double()
    cs, sn = torch.cos(ang).float().double().numpy(), torch.sin(ang).float().double().numpy()

    # ---- ms_encode_device
    c1 = mo.op_conv1(audio.double().numpy(), w(E + ".conv1.weight")[:, 0])
    gn = mo.op_groupnorm(c1, w(E + ".groupnorm.weight"), w(E + ".groupnorm.bias"))
    spans = lambda x, k, st: np.stack([x[st * t:st * t + k].reshape(-1) for t in range((len(x) - k) // st + 1)])   # frame t = a contiguous span of k frames
    convw = lambda p: w(p + ".weight").transpose(0, 2, 1).reshape(w(p + ".weight").shape[0], -1)                  # [out][k in]
    c2 = gelu(mo.T(spans(gn, 7, 3) @ convw(E + ".conv2").T + w(E + ".conv2.bias")))
    h = gelu(mo.T(spans(c2, 3, 2) @ convw(E + ".conv3").T + w(E + ".conv3.bias")))
    n = len(h)
    assert n == mr.frames(1700) == 3
    q = E + ".layers.0"
    x = mo.op_ln(h, w(q + ".input_layernorm.weight"))
    qkv = mo.T(x @ cat(q + ".self_attn", ("q_proj", "k_proj", "v_proj"), "weight").T + cat(q + ".self_attn", ("q_proj", "k_proj", "v_proj"), "bias"))
    qkv = np.stack([mo.op_rope_row(qkv[t], H + Hk, cs[t], sn[t], rot) for t in range(n)])
    K, V = qkv[:, H * 64:(H + Hk) * 64], qkv[:, (H + Hk) * 64:]
    att = np.stack([mo.op_attend(qkv[t, :H * 64], K, V, H, Hk, scale) for t in range(n)])
    h = mo.T(lin(att, q + ".self_attn.o_proj", False) + h)
    x = mo.op_ln(h, w(q + ".post_attention_layernorm.weight"))
    h = mo.T(lin(gelu(lin(x, q + ".mlp.fc1")), q + ".mlp.fc2") + h)
    enc = mo.op_ln(h, w(E + ".layer_norm.weight"))
    assert np.array_equal(enc, want_enc) and np.abs(enc).max() > 1.0

    # ---- the decoder step, three positions through the caches
    q = D + ".layers.0"
    ckv = mo.T(enc @ cat(q + ".encoder_attn", ("k_proj", "v_proj"), "weight").T + cat(q + ".encoder_attn", ("k_proj", "v_proj"), "bias"))
    emb = gr.bf16_bits(ref.w[D + ".embed_tokens.weight"].numpy())
    ref.reset(torch.from_numpy(want_enc))
    kc, vc = [], []
    for pos, tok in enumerate([cfg.decoder_start_token_id, 5, 39]):
        want = ref.step(tok).numpy()
        h = mo.val(mo.embed_reference(emb, np.array([tok])))
        qkv = mo.op_gemv(h, w(q + ".input_layernorm.weight"), cat(q + ".self_attn", ("q_proj", "k_proj", "v_proj"), "weight"),
                         cat(q + ".self_attn", ("q_proj", "k_proj", "v_proj"), "bias"), mo.MS_BF16)
        row = mo.op_rope_row(qkv[0], H + Hk, cs[pos], sn[pos], rot)
        kc.append(row[H * 64:(H + Hk) * 64]); vc.append(row[(H + Hk) * 64:])
        att = mo.op_attend(row[:H * 64], np.stack(kc), np.stack(vc), H, Hk, scale)[None]
        h = mo.op_gemv(att, None, w(q + ".self_attn.o_proj.weight"), None, mo.MS_RESID, h)
        cq = mo.op_gemv(h, w(q + ".post_attention_layernorm.weight"), w(q + ".encoder_attn.q_proj.weight"), w(q + ".encoder_attn.q_proj.bias"), mo.MS_BF16)
        att = mo.op_attend(cq[0], ckv[:, :Hk * 64], ckv[:, Hk * 64:], H, Hk, scale)[None]
        h = mo.op_gemv(att, None, w(q + ".encoder_attn.o_proj.weight"), None, mo.MS_RESID, h)
        act = mo.op_gemv(h, w(q + ".final_layernorm.weight"), w(q + ".mlp.fc1.weight"), w(q + ".mlp.fc1.bias"), mo.MS_GATE)
        h = mo.op_gemv(act, None, w(q + ".mlp.fc2.weight"), w(q + ".mlp.fc2.bias"), mo.MS_RESID, h)
        logits = mo.op_gemv(h, w(D + ".norm.weight"), w("proj_out.weight"), None, mo.MS_F32)[0]
        assert np.array_equal(logits.astype(f32), want) and np.abs(want).max() > 0.5, (pos, np.abs(logits - want).max())
