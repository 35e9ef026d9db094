"""BigVGAN on the GPU against tests/bigvgan_ref.py: the anti-aliased activation one launch at a time, every tap of two small configs
stage by stage (the reference run on the device's own previous stage) and the waveform chained end to end, batch independence,
launch count, errors, the directory loader and one run at the published widths.

Gates are derived, never read from the device: for each stage d_ref is the relative rms between the reference's float32 mode and its
float64 mode on the same input, and the gate is 4 d_ref (the tile accumulates K in MFMA pairs, an order neither mode has) plus, where the
stage holds a Snake, mis_sin_sq's absolute bound 3.3e-7 x max 1 / beta over the stage's rms.  The float32 reference is asserted to lie
inside every gate.  With MIS_BIGVGAN_PARITY_LOG=<file> the observed distances and gates are appended as JSON lines."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlx_audio_swift_amd as mas  # noqa: E402
import bigvgan_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
SIN_SQ_BOUND = 3.3e-7
RAGGED = [70, 13, 1]


def config(name, **kw):
    if name == "A":
        d = dict(num_mels=8, upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], upsample_initial_channel=32, resblock="1",
                 resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3, activation="snakebeta", snake_logscale=True,
                 use_bias_at_final=False, use_tanh_at_final=False)
    elif name == "B":
        d = dict(num_mels=8, upsample_rates=[2, 2], upsample_kernel_sizes=[4, 4], upsample_initial_channel=48, resblock="2",
                 resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3, activation="snake", snake_logscale=False,
                 use_bias_at_final=True, use_tanh_at_final=True)
    else:                                                                # the published widths, one stage and the tail
        d = dict(num_mels=100, upsample_rates=[4], upsample_kernel_sizes=[8], upsample_initial_channel=1536, resblock="1",
                 resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1], [3], [5]], activation="snakebeta", snake_logscale=True)
    d.update(dict(max_batch=4, max_frames=80), **kw)
    return mas.BigVGANConfig(**d)


def make_weights(cfg, seed):
    """Random float32 weights in the reference's layouts.  weight_g keeps every stage's variance near its input's; alpha (and beta) are drawn so
    that alpha u spans several periods: e^[0.5, 2] under snake_logscale, [2, 8] without."""
    rng = np.random.default_rng(seed)
    W = {}
    rates = {f"ups.{i}.0.weight_g": s for i, s in enumerate(cfg.upsample_rates)}
    rates["conv_post.weight_g"] = 2.0 / 16                              # a quarter of the others: most samples stay inside the clip
    for name, shape in mas.bigvgan_expected_shapes(cfg).items():
        if name.endswith("weight_v"):
            v = rng.standard_normal(shape, dtype=np.float32)
        elif name.endswith("weight_g"):
            v = (rng.uniform(0.8, 1.2, shape) * np.sqrt(rates.get(name, 2) / 2.0)).astype(np.float32)
        elif name.endswith("bias"):
            v = (0.1 * rng.standard_normal(shape)).astype(np.float32)
        else:
            lo, hi = (0.5, 2.0) if cfg.snake_logscale else (2.0, 8.0)
            v = rng.uniform(lo, hi, shape).astype(np.float32)
        W[name] = v
    return W


def relrms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30))


def log_parity(**line):
    path = os.environ.get("MIS_BIGVGAN_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")


class Bundle:
    """One config: the engine, its weights and both reference modes; runs are cached by their frame counts."""

    def __init__(self, name, seed, **kw):
        self.name, self.cfg = name, config(name, **kw)
        self.W = make_weights(self.cfg, seed)
        self.model = mas.BigVGAN.from_weights(self.cfg, self.W)
        self.ref64, self.ref32 = R.BigVGANRef(self.cfg, self.W, np.float64), R.BigVGANRef(self.cfg, self.W, np.float32)
        self.n_taps = 2 + len(self.cfg.upsample_rates) * (len(self.cfg.resblock_kernel_sizes) + 2)
        self.runs = {}

    def mel(self, frames, junk=0.0):
        m = np.full((len(frames), self.cfg.num_mels, max(frames)), junk, np.float32)
        for b, n in enumerate(frames):
            m[b, :, :n] = np.random.default_rng(77 + n).standard_normal((self.cfg.num_mels, n), dtype=np.float32)
        return m

    def run(self, frames):
        key = tuple(frames)
        if key not in self.runs:
            mel = self.mel(frames)
            wav = self.model.decode(mel, frames)
            self.runs[key] = (mel, wav, [self.model.debug_tap(s) for s in range(self.n_taps)], self.model.launches)
        return self.runs[key]

    def snake_prefixes(self, stage):
        nk = len(self.cfg.resblock_kernel_sizes)
        if stage == self.n_taps - 1:
            return ["activation_post"]
        i, r = divmod(stage - 1, nk + 2)
        return [f"resblocks.{i * nk + r - 1}."] if stage >= 1 and 1 <= r <= nk else []


@pytest.fixture(scope="module")
def bundles():
    return {"A": Bundle("A", 11), "B": Bundle("B", 12)}


def check_run(bd, frames):
    """Every tap against the reference's step from the device's own previous taps, and the waveform chained end to end."""
    mel, wav, taps, _ = bd.run(frames)
    hop = bd.cfg.hop_length
    worst = 0.0
    for stage in range(bd.n_taps + 1):                                   # the last "stage" is conv_post + clamp from activation_post
        dev, w64, w32 = [], [], []
        for b, n in enumerate(frames):
            rows = [t[b][:, : n * (t.shape[2] // mel.shape[2])] for t in taps]
            if stage == bd.n_taps:
                w64.append(bd.ref64.final(rows[-1])), w32.append(bd.ref32.final(rows[-1])), dev.append(wav[b, : n * hop])
            else:
                w64.append(bd.ref64.step(stage, rows, mel[b, :, :n]).ravel())
                w32.append(bd.ref32.step(stage, rows, mel[b, :, :n]).ravel())
                dev.append(rows[stage].ravel())
                assert not taps[stage][b][:, rows[stage].shape[1]:].any(), (stage, b)     # zeros behind the row
        dev, w64, w32 = np.concatenate(dev), np.concatenate(w64), np.concatenate(w32)
        assert dev.shape == w64.shape and np.isfinite(dev).all()
        d_ref, d_dev = relrms(w32, w64), relrms(dev, w64)
        pre = bd.snake_prefixes(stage) if stage < bd.n_taps else []
        snake = SIN_SQ_BOUND * bd.ref64.max_rbeta(pre) / np.sqrt(np.mean(w64 ** 2)) if pre else 0.0
        gate = 4.0 * d_ref + snake
        print(f"bigvgan {bd.name} frames {frames} stage {stage}: device {d_dev:.3e} f32-reference {d_ref:.3e} gate {gate:.3e}")
        log_parity(config=bd.name, frames=list(frames), stage=stage, kind="step", device=d_dev, f32_reference=d_ref, gate=gate)
        assert 0.0 < d_ref <= gate, (stage, d_ref, gate)
        worst = max(worst, d_dev / gate)
        assert d_dev <= gate, (bd.name, frames, stage, d_dev, gate)
    dev, w64, w32 = [], [], []
    for b, n in enumerate(frames):
        w64.append(bd.ref64.forward(mel[b, :, :n])[1]), w32.append(bd.ref32.forward(mel[b, :, :n])[1]), dev.append(wav[b, : n * hop])
        assert not wav[b, n * hop:].any()
    dev, w64, w32 = np.concatenate(dev), np.concatenate(w64), np.concatenate(w32)
    d_ref, d_dev = relrms(w32, w64), relrms(dev, w64)
    gate = 4.0 * d_ref + SIN_SQ_BOUND * bd.ref64.max_rbeta([""]) / np.sqrt(np.mean(w64 ** 2))
    print(f"bigvgan {bd.name} frames {frames} chained: device {d_dev:.3e} f32-reference {d_ref:.3e} gate {gate:.3e}")
    log_parity(config=bd.name, frames=list(frames), stage="wav", kind="chained", device=d_dev, f32_reference=d_ref, gate=gate)
    assert 0.0 < d_ref <= gate and d_dev <= gate, (bd.name, frames, d_dev, d_ref, gate)
    assert np.abs(dev).max() > 1e-2
    if not bd.cfg.use_tanh_at_final and len(frames) > 1:
        assert np.abs(dev).max() == 1.0 and (np.abs(dev) == 1.0).sum() < dev.size // 2                # the clip is exercised


# ---------------------------------------------------------------------------------------------- 1. the operator
@pytest.mark.parametrize("C", [3, 12, 33])
def test_aa_act_operator(C):
    """One launch of k_bv_aa_act on a ragged batch against the float64 gather form; NaN lies behind every row."""
    counts = [1, 2, 5, 64, 65, 131]
    rng = np.random.default_rng(C)
    x = np.full((len(counts), C, max(counts)), np.nan, np.float32)
    for b, n in enumerate(counts):
        x[b, :, :n] = rng.standard_normal((C, n), dtype=np.float32)
    alpha, beta = rng.uniform(2.0, 8.0, C).astype(np.float32), rng.uniform(0.2, 1.0, C).astype(np.float32)
    got = mas.bigvgan_aa_act(x, counts, alpha, beta)
    dev, w64, w32 = [], [], []
    for b, n in enumerate(counts):
        assert not got[b, :, n:].any(), b
        dev.append(got[b, :, :n].ravel())
        w64.append(R.aa_gather(x[b, :, :n].astype(np.float64), alpha.astype(np.float64), beta.astype(np.float64)).ravel())
        w32.append(R.aa_gather(x[b, :, :n], alpha, beta).ravel())
    dev, w64, w32 = np.concatenate(dev), np.concatenate(w64), np.concatenate(w32)
    assert np.isfinite(dev).all()
    d_ref, d_dev = relrms(w32, w64), relrms(dev, w64)
    gate = 4.0 * d_ref + SIN_SQ_BOUND * float((1.0 / beta).max()) / np.sqrt(np.mean(w64 ** 2))
    print(f"bigvgan aa_act C {C}: device {d_dev:.3e} f32-reference {d_ref:.3e} gate {gate:.3e}")
    log_parity(config="aa_act", channels=C, counts=counts, kind="operator", device=d_dev, f32_reference=d_ref, gate=gate)
    assert 0.0 < d_ref <= gate and d_dev <= gate, (d_dev, d_ref, gate)


# ---------------------------------------------------------------------------------------------- 2. taps and the chained waveform
@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("frames", [RAGGED, [1], [2], [5]], ids=["ragged", "one", "two", "five"])
def test_taps_and_waveform(bundles, name, frames):
    check_run(bundles[name], frames)


# ---------------------------------------------------------------------------------------------- 3. batch independence
@pytest.mark.parametrize("name", ["A", "B"])
def test_rows_do_not_depend_on_their_batch(bundles, name):
    bd = bundles[name]
    mel, wav, _, _ = bd.run(RAGGED)
    hop = bd.cfg.hop_length
    poisoned = bd.model.decode(bd.mel(RAGGED, junk=np.nan), RAGGED)
    assert np.array_equal(poisoned, wav)
    for b, n in enumerate(RAGGED):
        alone = bd.model.decode(mel[b: b + 1, :, :n])
        assert alone.shape == (1, n * hop) and np.array_equal(alone[0], wav[b, : n * hop]), b
        assert not wav[b, n * hop:].any()
    y = bd.model(mel[:1])
    assert y.shape == (1, 1, RAGGED[0] * hop) and np.array_equal(y[0, 0], wav[0])
    assert np.array_equal(bd.model.decode_audio(mel[:1]), y)
    assert bd.model.hop_length == hop and bd.model.num_samples(7) == 7 * hop and bd.model.codec_sample_rate is None


# ---------------------------------------------------------------------------------------------- 4. launches
@pytest.mark.parametrize("name", ["A", "B"])
def test_launch_count(bundles, name):
    bd = bundles[name]
    per_dilation = 4 if bd.cfg.resblock == "1" else 2
    want = 3 + sum(2 + sum(per_dilation * len(d) for d in bd.cfg.resblock_dilation_sizes) for _ in bd.cfg.upsample_rates)
    assert bd.run(RAGGED)[3] == want == (3 + 2 * (2 + 9 * per_dilation))


# ---------------------------------------------------------------------------------------------- 5. errors
def test_errors(bundles):
    bd = bundles["A"]
    m, nm = bd.model, bd.cfg.num_mels
    for mel, frames, word in ((np.zeros((5, nm, 4), np.float32), None, "max_batch"), (np.zeros((1, nm, 81), np.float32), None, "max_frames"),
                              (np.zeros((2, nm, 4), np.float32), [4, 0], "row 1"), (np.zeros((2, nm, 4), np.float32), [5, 4], "row 0")):
        with pytest.raises(mas.AudioGenerationError) as e:
            m.decode(mel, frames)
        assert e.value.case == "invalidInput" and word in str(e.value), str(e.value)
    raw = mas.BigVGAN(bd.cfg)
    with pytest.raises(mas.AudioGenerationError) as e:
        raw.decode(np.zeros((1, nm, 4), np.float32))
    assert "not finalized" in str(e.value)
    for k, v in bd.W.items():
        if k != "resblocks.1.convs2.2.weight_g":
            raw.set_tensor(k, v if k != "conv_pre.weight_v" else v[:, :3])
    with pytest.raises(mas.AudioGenerationError) as e:
        raw.finalize()
    assert "conv_pre.weight_v" in str(e.value) and "shape" in str(e.value)
    raw.set_tensor("conv_pre.weight_v", bd.W["conv_pre.weight_v"])
    with pytest.raises(mas.AudioGenerationError) as e:
        raw.finalize()
    assert "resblocks.1.convs2.2.weight_g" in str(e.value) and "missing" in str(e.value)
    with pytest.raises(mas.AudioGenerationError):
        mas.BigVGAN.from_weights(bd.cfg, {k: v for k, v in bd.W.items() if k != "conv_pre.bias"})
    with pytest.raises(mas.AudioGenerationError) as e:
        mas.BigVGAN(config("A", upsample_kernel_sizes=[8, 6]))
    assert "upsample_kernel_sizes" in str(e.value)


# ---------------------------------------------------------------------------------------------- 6. the loader
def test_from_model_directory_round_trip(bundles, tmp_path):
    """A torch-layout checkpoint (Conv1d [out, in, k], ConvTranspose1d [in, out, k], weight_g [in, 1, 1]) and config.json."""
    import torch
    from safetensors.torch import save_file
    bd = bundles["B"]
    sd = {}
    for k, v in bd.W.items():
        t = torch.from_numpy(v)
        if k.endswith("weight_v"):
            t = t.permute(2, 0, 1) if k.startswith("ups.") else t.permute(0, 2, 1)
        elif k.endswith("weight_g") and k.startswith("ups."):
            t = t.permute(2, 0, 1)
        sd[k] = t.contiguous()
    sd["conv_pre.num_batches_tracked"] = torch.zeros(1)
    save_file(sd, str(tmp_path / "model.safetensors"))
    keys = ("num_mels", "upsample_rates", "upsample_kernel_sizes", "upsample_initial_channel", "resblock", "resblock_kernel_sizes",
            "resblock_dilation_sizes", "activation", "snake_logscale", "use_bias_at_final", "use_tanh_at_final")
    (tmp_path / "config.json").write_text(json.dumps({k: getattr(bd.cfg, k) for k in keys}))
    m = mas.BigVGAN.from_model_directory(str(tmp_path), max_batch=4, max_frames=80)
    mel, wav, _, _ = bd.run(RAGGED)
    assert np.array_equal(m.decode(mel, RAGGED), wav)


# ---------------------------------------------------------------------------------------------- 7. the published widths
def test_published_widths_two_frames():
    """conv_pre 100 -> 1536, one transposed conv to 768 channels, three AMP blocks of 3 / 7 / 11 taps at dilations 1 / 3 / 5 and the
    tail, on two mel frames: the full-width tiles (K up to 11 x 768) run once."""
    bd = Bundle("P", 13, max_batch=1, max_frames=2)
    check_run(bd, [2])
