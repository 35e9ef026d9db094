"""DeepFilterNet on the GPU against tests/deepfilternet_ref.py: every tap of a ragged batch of eight rows stage by stage (the float64
reference run on the device's own previous stage; a recurrence layer over the whole row from the zero state), the chain end to end, bit
identity across batches, the short rows, one row of several thousand frames, the published shape once, launch counts, errors and the
directory loader.

Gates are derived, never read from the device: for each stage d_ref is the relative rms between the reference's float32 mode and its
float64 mode on the same input, and the gate is 4 d_ref (the tile accumulates K in MFMA pairs, an order neither mode has; the rule of
tests/test_gpu_bigvgan.py) + FLOOR = 2^-23, one float32 unit in the last place, for stages whose float32 distance is 0 (an all-zero
stage, a stage of exact operations).  With MIS_DEEPFILTERNET_PARITY_LOG=<file> the observed distances and gates are appended as JSON
lines."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlx_audio_swift_amd as mas  # noqa: E402
import deepfilternet_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -23
SHORT = 5                                                                 # rows 0..4: 0, 1, hop - 1, hop, hop + 1 samples


def relrms(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30)) if a.size else 0.0


def log_parity(**line):
    path = os.environ.get("MIS_DEEPFILTERNET_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")


def stage_plan(ref):
    """tap -> (function of (reference, taps of one row, waveform), in the order the engine computes them)."""
    Le, Lr, Ld = ref.L
    fb = "erb_fb" in ref.W
    plan = [(0, lambda r, t, x: r.stft(x))]
    if fb:
        plan.append((26, lambda r, t, x: r.erb_db(t[0])))
    plan += [(1, lambda r, t, x: r.features(t[0], t.get(26))[0]), (2, lambda r, t, x: r.features(t[0], t.get(26))[1]),
             (3, lambda r, t, x: r.e0(t[1])), (4, lambda r, t, x: r.e1(t[3])), (5, lambda r, t, x: r.e2(t[4])), (6, lambda r, t, x: r.e3(t[5])),
             (7, lambda r, t, x: r.c0(t[2])), (8, lambda r, t, x: r.c1(t[7])), (9, lambda r, t, x: r.emb0(t[6], t[8]))]

    def chain(base, prefix, n, src):
        out = [(base, lambda r, t, x: r.linear_in(t[src].reshape(len(t[src]), -1), prefix))]
        for l in range(n):
            out.append((base + 1 + l, lambda r, t, x, l=l: r.gru(t[base + l], prefix, l)))
        return out

    plan += chain(32, "enc.emb_gru", Le, 9)
    plan += [(10, lambda r, t, x: r.linear_out(t[32 + Le], "enc.emb_gru")), (11, lambda r, t, x: r.lsnr(t[10]))]
    plan += chain(48, "erb_dec.emb_gru", Lr, 10) + chain(64, "df_dec.df_gru", Ld, 10)
    plan += [(12, lambda r, t, x: r.linear_out(t[48 + Lr], "erb_dec.emb_gru")),
             (13, lambda r, t, x: r.pathway(t[6], 3, t[12].reshape(t[6].shape))), (14, lambda r, t, x: r.d3(t[13])),
             (15, lambda r, t, x: r.pathway(t[5], 2, t[14])), (16, lambda r, t, x: r.d2(t[15])),
             (17, lambda r, t, x: r.pathway(t[4], 1, t[16])), (18, lambda r, t, x: r.d1(t[17])),
             (19, lambda r, t, x: r.pathway(t[3], 0, t[18])), (20, lambda r, t, x: r.mask(t[19])),
             (21, lambda r, t, x: r.df_skip(t[64 + Ld], t[10])), (22, lambda r, t, x: r.c0p(t[7])), (23, lambda r, t, x: r.coefs(t[21], t[22])),
             (24, lambda r, t, x: r.enhanced(t[0], t[20], t[23])), (25, lambda r, t, x: r.istft(t[24], len(x)))]
    return plan


class Bundle:
    def __init__(self, name, **kw):
        self.name = name
        self.cfg, self.W = R.case(name, **kw)
        self.model = mas.DeepFilterNet.from_weights(self.cfg, self.W)
        self.ref64, self.ref32 = R.DeepFilterNetRef(self.cfg, self.W), R.DeepFilterNetRef(self.cfg, self.W, np.float32)
        self.plan = stage_plan(self.ref64)
        self.rows = R.rows(self.cfg)
        self._run = None
        self._chain = {}

    def shapes(self, T):
        c, E, D, C_ = self.cfg, self.cfg.nb_erb, self.cfg.nb_df, self.cfg.conv_ch
        s = {1: (T, E, 1), 2: (T, D, 2), 3: (T, E, C_), 4: (T, E // 2, C_), 5: (T, E // 4, C_), 6: (T, E // 4, C_), 7: (T, D, C_), 8: (T, D // 2, C_),
             13: (T, E // 4, C_), 14: (T, E // 4, C_), 15: (T, E // 4, C_), 16: (T, E // 2, C_), 17: (T, E // 2, C_), 18: (T, E, C_), 19: (T, E, C_),
             20: (T, E, 1), 22: (T, D, 2 * c.df_order), 23: (T, D, 2 * c.df_order)}
        return s

    def run(self):
        """The ragged batch of eight once: waveforms, lsnr, every tap."""
        if self._run is None:
            wav, lsnr = self.model.enhance_raw(self.rows, junk=np.nan)
            taps = {k: self.model.tap(k) for k, _ in self.plan}
            self._run = (wav, lsnr, taps, self.model.launches)
        return self._run

    def row_taps(self, taps, b, dtype):
        T = self.ref64.frames(len(self.rows[b]))
        sh = self.shapes(T)
        out = {}
        for k, v in taps.items():
            if k == 25:
                out[k] = v[b, : len(self.rows[b])].astype(dtype)
            elif k == 11:
                out[k] = v[b, :T].astype(dtype)
            else:
                out[k] = v[b, :T].reshape(sh.get(k, (T, -1))).astype(dtype)
        return out

    def chain(self, b):
        if b not in self._chain:
            self._chain[b] = (self.ref64.forward(self.rows[b]), self.ref32.forward(self.rows[b]))
        return self._chain[b]


@pytest.fixture(scope="module")
def bundles():
    return {"S": Bundle("S"), "W": Bundle("W")}


def gate_of(name, kind, stage, dev, w64, w32):
    dev, w64, w32 = np.concatenate([a.ravel() for a in dev]), np.concatenate([a.ravel() for a in w64]), np.concatenate([a.ravel() for a in w32])
    assert dev.shape == w64.shape and np.isfinite(dev).all(), (name, stage)
    d_ref, d_dev = relrms(w32, w64), relrms(dev, w64)
    gate = 4.0 * d_ref + FLOOR
    print(f"deepfilternet {name} {kind} stage {stage}: device {d_dev:.3e} f32-reference {d_ref:.3e} gate {gate:.3e}")
    log_parity(config=name, stage=stage, kind=kind, device=d_dev, f32_reference=d_ref, gate=gate)
    return d_dev, gate


# ---------------------------------------------------------------------------------------------- 1. taps, stage by stage
@pytest.mark.parametrize("name", ["S", "W"])
def test_taps_stage_by_stage(bundles, name):
    bd = bundles[name]
    wav, lsnr, taps, _ = bd.run()
    bad = []
    for k, fn in bd.plan:
        dev, w64, w32 = [], [], []
        for b in range(len(bd.rows)):
            t64, t32 = bd.row_taps(taps, b, np.float64), bd.row_taps(taps, b, np.float32)
            dev.append(t64[k]), w64.append(fn(bd.ref64, t64, bd.rows[b])), w32.append(fn(bd.ref32, t32, bd.rows[b]))
            assert w64[-1].size == dev[-1].size, (k, b, w64[-1].shape, dev[-1].shape)
            T = bd.ref64.frames(len(bd.rows[b]))
            tail = taps[k][b, len(bd.rows[b]):] if k == 25 else taps[k][b, T:]
            assert not tail.any(), (k, b)                                 # zeros behind the row
        d_dev, gate = gate_of(name, "step", k, dev, w64, w32)
        if d_dev > gate:
            bad.append((k, d_dev, gate))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- 2. the chain end to end
@pytest.mark.parametrize("name", ["S", "W"])
def test_chained_enhance(bundles, name):
    bd = bundles[name]
    wav, lsnr, taps, _ = bd.run()
    bad = []
    for k in (20, 23, 11, 25):
        dev, w64, w32 = [], [], []
        for b in range(len(bd.rows)):
            c64, c32 = bd.chain(b)
            dev.append(bd.row_taps(taps, b, np.float64)[k]), w64.append(c64[k]), w32.append(c32[k])
        d_dev, gate = gate_of(name, "chained", k, dev, w64, w32)
        if d_dev > gate:
            bad.append((k, d_dev, gate))
    for b, x in enumerate(bd.rows):
        assert wav[b].shape == x.shape and np.array_equal(wav[b], taps[25][b, : len(x)])
        assert np.array_equal(lsnr[b], taps[11][b, : len(lsnr[b]), 0])
    assert np.abs(np.concatenate(wav)).max() > 1e-3
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- 3. bit identity
@pytest.mark.parametrize("name", ["S", "W"])
def test_rows_do_not_depend_on_their_batch(bundles, name):
    bd = bundles[name]
    wav, lsnr, taps, _ = bd.run()
    m = bd.model

    def same(b, w, ls, at):
        T = len(lsnr[b])
        assert np.array_equal(w, wav[b]) and np.array_equal(ls, lsnr[b]), b
        assert np.array_equal(m.tap(20)[at, :T], taps[20][b, :T]) and np.array_equal(m.tap(23)[at, :T], taps[23][b, :T]), b

    for b, x in enumerate(bd.rows):                                       # batch 1 against batch 8
        w, ls = m.enhance_raw([x])
        same(b, w[0], ls[0], 0)
    perm = [5, 0, 7, 3, 6, 1, 4, 2]                                        # row order permuted, zeros in the padding instead of NaN
    w, ls = m.enhance_raw([bd.rows[i] for i in perm], junk=None)
    t20, t23 = m.tap(20), m.tap(23)
    for at, b in enumerate(perm):
        T = len(lsnr[b])
        assert np.array_equal(w[at], wav[b]) and np.array_equal(ls[at], lsnr[b]), b
        assert np.array_equal(t20[at, :T], taps[20][b, :T]) and np.array_equal(t23[at, :T], taps[23][b, :T]), b
    w, ls = m.enhance_raw([bd.rows[7], bd.rows[5]], junk=1e30)             # a row beside a longer one
    same(7, w[0], ls[0], 0)


# ---------------------------------------------------------------------------------------------- 4. the short rows
@pytest.mark.parametrize("name", ["S", "W"])
def test_short_rows(bundles, name):
    bd = bundles[name]
    wav, lsnr, taps, _ = bd.run()
    hop = bd.cfg.hop_size
    T, n = bd.model.frames([len(x) for x in bd.rows[:SHORT]])
    assert list(T) == [2, 2, 2, 3, 3] and list(n) == [0, 1, hop - 1, hop, hop + 1]
    for b in range(SHORT):
        assert wav[b].shape == (len(bd.rows[b]),) and len(lsnr[b]) == T[b] and np.isfinite(wav[b]).all() and np.isfinite(lsnr[b]).all()
    assert wav[0].size == 0
    # The gates are ratios of rms distances, and the 1-sample row's waveform is ONE number: its distance is a single draw, not an
    # rms (a first version gated row by row; S row 1 gave device 8.1e-7 against f32-reference 9.4e-8, every other row <= 0.47 of its
    # gate).  So the five rows are pooled, as the stage tests pool their rows: 289 samples, 12 frames.
    bad = []
    for k in (20, 23, 25):
        chains = [bd.chain(b) for b in range(SHORT)]
        d_dev, gate = gate_of(name, "short rows", k, [bd.row_taps(taps, b, np.float64)[k] for b in range(SHORT)], [c[0][k] for c in chains],
                              [c[1][k] for c in chains])
        if d_dev > gate:
            bad.append((k, d_dev, gate))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- 5. a long row
def test_one_long_row_on_w():
    """3000 frames: the recurrences and the normalisations accumulate over time."""
    bd = Bundle("W", max_batch=1, max_seconds=6.1)
    x = R.rows(bd.cfg, long_frames=3000)[5]
    wav, lsnr = bd.model.enhance_raw([x])
    taps = {k: bd.model.tap(k) for k in (20, 23, 25)}
    bd.rows = [x]
    c64, c32 = bd.ref64.forward(x), bd.ref32.forward(x)
    bad = []
    for k in (20, 23, 25):
        d_dev, gate = gate_of("W", "long row", k, [bd.row_taps(taps, 0, np.float64)[k]], [c64[k]], [c32[k]])
        if d_dev > gate:
            bad.append((k, d_dev, gate))
    assert np.isfinite(wav[0]).all() and len(lsnr[0]) == 1 + (bd.cfg.hop_size + len(x)) // bd.cfg.hop_size
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- 6. the published shape
def test_published_shape_one_short_row():
    bd = Bundle("P")
    x = R.rows(bd.cfg, long_frames=6)[5]
    bd.rows = [x]
    wav, lsnr = bd.model.enhance_raw([x])
    taps = {k: bd.model.tap(k) for k in (20, 23, 25)}
    c64, c32 = bd.ref64.forward(x), bd.ref32.forward(x)
    bad = []
    for k in (20, 23, 25):
        d_dev, gate = gate_of("P", "chained", k, [bd.row_taps(taps, 0, np.float64)[k]], [c64[k]], [c32[k]])
        if d_dev > gate:
            bad.append((k, d_dev, gate))
    assert bd.model.launches == bd.model.expected_launches(True, True) == 26 + 4 + 2 + 2 + 2 + 2
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- 7. launches
def test_launch_count(bundles):
    """26 + [erb_fb] + [df_skip] + the two linear_outs + 2 L_enc + L_erb + L_df + max(L_erb, L_df) (equal hidden sizes)."""
    s, w = bundles["S"], bundles["W"]
    assert s.run()[3] == s.model.expected_launches(False, False) == 26 + 2 + 2 * 1 + 2 + 1 + 2
    assert w.run()[3] == w.model.expected_launches(True, True) == 26 + 4 + 2 * 1 + 2 + 2 + 2


# ---------------------------------------------------------------------------------------------- 8. errors
def test_errors_leave_the_handle_usable(bundles):
    bd = bundles["S"]
    wav = bd.run()[0]
    m = bd.model
    for rows, word in (([bd.rows[3]] * 9, "max_batch"), ([np.zeros(bd.cfg.max_samples + 1, np.float32)], "max_seconds")):
        with pytest.raises(mas.AudioGenerationError) as e:
            m.enhance_batch(rows)
        assert word in str(e.value), str(e.value)
    with pytest.raises(mas.DeepFilterNetError) as e:
        m.enhance(np.zeros((2, 10), np.float32))
    assert e.value.sts_case == "invalidAudioShape"
    with pytest.raises(mas.AudioGenerationError) as e:
        m.enhance(bd.rows[3], sample_rate=16000)
    assert "resampler" in str(e.value)
    with pytest.raises(mas.AudioGenerationError):
        m.tap(99)
    assert np.array_equal(m.enhance(bd.rows[7]), wav[7])
    raw = mas.DeepFilterNet(bd.cfg)
    with pytest.raises(mas.AudioGenerationError) as e:
        raw.enhance(bd.rows[3])
    assert "not finalized" in str(e.value)
    with pytest.raises(mas.AudioGenerationError) as e:
        raw.finalize()
    assert "mask.erb_inv_fb" in str(e.value)
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.DeepFilterNet(mas.DeepFilterNetConfig(emb_hidden_dim=48))
    assert "hidden" in str(e.value)


# ---------------------------------------------------------------------------------------------- 9. the loader
def test_from_local_equals_from_weights(bundles, tmp_path):
    import torch
    from safetensors.torch import save_file
    bd = bundles["S"]
    sd = {k: torch.from_numpy(v).to(torch.float32).contiguous() for k, v in bd.W.items()}
    sd["enc.erb_conv0.2.num_batches_tracked"] = torch.zeros(1)
    (tmp_path / "v3").mkdir()
    save_file(sd, str(tmp_path / "v3" / "model.safetensors"))
    keys = ("sample_rate", "fft_size", "hop_size", "nb_erb", "nb_df", "df_order", "df_lookahead", "conv_lookahead", "conv_ch", "emb_hidden_dim",
            "df_hidden_dim", "linear_groups", "enc_linear_groups", "model_version")
    (tmp_path / "v3" / "config.json").write_text(json.dumps({k: getattr(bd.cfg, k) for k in keys}))
    m = mas.load_sts_model(str(tmp_path), model_type="dfn", max_batch=8, max_seconds=0.7)
    assert isinstance(m, mas.DeepFilterNet) and m.layers == bd.model.layers
    wav = bd.run()[0]
    got = m.enhance_batch(bd.rows)
    assert all(np.array_equal(a, b) for a, b in zip(got, wav))
