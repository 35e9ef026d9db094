"""BigVGAN, CPU side: the reference (tests/bigvgan_ref.py) against an independent build from torch.nn.functional with torch.nn.utils
weight norm, the closed gather form of the anti-aliased activation against the literal pad / conv / crop form (and a mutated form that
must fail), the filter against scipy.signal, the host mirror (config, sanitize, expected keys, output lengths), the create-time refusal,
and the resource bounds of csrc/bigvgan.hip from the compiler's remarks."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlx_audio_swift_amd as mas  # noqa: E402
from mlx_audio_swift_amd import _lib  # noqa: E402
import bigvgan_ref as R  # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"


def small_config(**kw):
    d = dict(num_mels=8, upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], upsample_initial_channel=32, resblock="1",
             resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], activation="snakebeta",
             snake_logscale=True, use_bias_at_final=False, use_tanh_at_final=False)
    d.update(kw)
    return mas.BigVGANConfig(**d)


# ---------------------------------------------------------------------------------------------- an independent torch build
def scipy_filter():
    from scipy.signal.windows import kaiser
    a = 2.285 * 5 * np.pi * 1.2 + 7.95
    t = np.arange(12) - 6 + 0.5
    f = 0.5 * kaiser(12, 0.1102 * (a - 8.7), sym=True) * np.sinc(0.5 * t)
    return f / f.sum()


class TorchBigVGAN(torch.nn.Module):
    """BigVGAN in torch's own layouts (Conv1d [out, in, k], ConvTranspose1d [in, out, k]) under the checkpoint's key names."""

    def __init__(self, cfg):
        super().__init__()
        wn = torch.nn.utils.weight_norm
        self.cfg = cfg
        c0, nk = cfg.upsample_initial_channel, len(cfg.resblock_kernel_sizes)
        self.conv_pre = wn(torch.nn.Conv1d(cfg.num_mels, c0, 7, padding=3))
        self.ups = torch.nn.ModuleList()
        self.resblocks = torch.nn.ModuleList()
        self.acts = torch.nn.ParameterDict()
        for i, (s, k) in enumerate(zip(cfg.upsample_rates, cfg.upsample_kernel_sizes)):
            ch = c0 >> (i + 1)
            self.ups.append(torch.nn.ModuleList([wn(torch.nn.ConvTranspose1d(2 * ch, ch, k, s, padding=(k - s) // 2))]))
            for ks, dil in zip(cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes):
                blk = torch.nn.Module()
                if cfg.resblock == "1":
                    blk.convs1 = torch.nn.ModuleList([wn(torch.nn.Conv1d(ch, ch, ks, dilation=d, padding=(ks - 1) * d // 2)) for d in dil])
                    blk.convs2 = torch.nn.ModuleList([wn(torch.nn.Conv1d(ch, ch, ks, padding=(ks - 1) // 2)) for _ in dil])
                else:
                    blk.convs = torch.nn.ModuleList([wn(torch.nn.Conv1d(ch, ch, ks, dilation=d, padding=(ks - 1) * d // 2)) for d in dil])
                self.resblocks.append(blk)
        self.conv_post = wn(torch.nn.Conv1d(c0 >> len(cfg.upsample_rates), 1, 7, padding=3, bias=cfg.use_bias_at_final))
        self.filt = torch.from_numpy(scipy_filter())

    def act(self, x, alpha, beta):
        ch = x.shape[1]
        if self.cfg.snake_logscale:
            alpha, beta = alpha.exp(), beta.exp()
        f = self.filt.to(x.dtype).view(1, 1, 12).expand(ch, 1, 12)
        u = 2.0 * F.conv_transpose1d(F.pad(x, (5, 5), mode="replicate"), f, stride=2, groups=ch)[..., 15:-15]
        v = u + (1.0 / (beta.view(1, -1, 1) + 1e-9)) * torch.sin(u * alpha.view(1, -1, 1)) ** 2
        return F.conv1d(F.pad(v, (5, 6), mode="replicate"), f, stride=2, groups=ch)

    def forward(self, mel, snakes):
        def a(p, x):
            al = snakes[p + ".act.alpha"]
            return self.act(x, al, snakes.get(p + ".act.beta", al))
        nk = len(self.cfg.resblock_kernel_sizes)
        h = self.conv_pre(mel)
        for i in range(len(self.ups)):
            h = self.ups[i][0](h)
            total = None
            for j in range(nk):
                blk, q, out = self.resblocks[i * nk + j], f"resblocks.{i * nk + j}", h
                for d in range(len(self.cfg.resblock_dilation_sizes[j])):
                    if self.cfg.resblock == "1":
                        out = out + blk.convs2[d](a(f"{q}.activations.{2 * d + 1}", blk.convs1[d](a(f"{q}.activations.{2 * d}", out))))
                    else:
                        out = out + blk.convs[d](a(f"{q}.activations.{d}", out))
                total = out if total is None else total + out
            h = total / nk
        y = self.conv_post(a("activation_post", h))
        return torch.tanh(y) if self.cfg.use_tanh_at_final else torch.clamp(y, -1.0, 1.0)


def torch_checkpoint(cfg, seed):
    """(torch model in float64, its state dict in torch layouts + the act parameters + a num_batches_tracked key)."""
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = TorchBigVGAN(cfg).double()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("weight_g"):
                p.mul_(1.0 + 0.5 * torch.rand(p.shape, generator=g, dtype=torch.float64))
            if n.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g, dtype=torch.float64))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items() if k != "filt"}
    snakes = {}
    for name, shape in mas.bigvgan_expected_shapes(cfg).items():
        if ".act." in name:
            lo, hi = (0.5, 2.0) if cfg.snake_logscale else (2.0, 8.0)
            snakes[name] = lo + (hi - lo) * torch.rand(shape, generator=g, dtype=torch.float64)
    sd.update(snakes)
    sd["conv_pre.num_batches_tracked"] = torch.zeros(1)
    return m, sd, snakes


@pytest.mark.parametrize("resblock,activation,logscale,tanh,bias", [("1", "snakebeta", True, False, False), ("2", "snake", False, True, True)])
def test_reference_matches_an_independent_torch_build(resblock, activation, logscale, tanh, bias):
    cfg = small_config(resblock=resblock, activation=activation, snake_logscale=logscale, use_tanh_at_final=tanh, use_bias_at_final=bias)
    m, sd, snakes = torch_checkpoint(cfg, 5)
    W = {k: v.numpy() for k, v in mas.bigvgan_sanitize(cfg, sd).items()}
    assert {k: tuple(v.shape) for k, v in W.items()} == mas.bigvgan_expected_shapes(cfg)
    mel = torch.randn(1, cfg.num_mels, 13, dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        want = m(mel, snakes)[0, 0].numpy()
    taps, got = R.BigVGANRef(cfg, W).forward(mel[0].numpy())
    assert got.shape == want.shape == (13 * cfg.hop_length,)
    assert len(taps) == 2 + 2 * (3 + 2)
    # Both sides are float64 and differ in summation order only.  One rounding is 1.1e-16; a Snake with alpha / beta up to e^2 / e^0.5
    # has a local gain up to 1 + alpha / beta = 5.5, and a block chains six of them, so round-off can grow by 5.5^6 = 3e4 a stage in the
    # worst case and by 8e8 over two: the bound allows 1e-8.  A transposed layout, a shifted tap or a wrong clamp moves the output by
    # more than 1e-3 of its peak.
    assert np.abs(want).max() > 1e-2
    assert np.abs(got - want).max() < 1e-8


# ---------------------------------------------------------------------------------------------- the two clamps
@pytest.mark.parametrize("T", [1, 2, 5, 6, 13])
def test_gather_form_equals_the_literal_form_and_the_mutant_does_not(T):
    rng = np.random.default_rng(T)
    x = rng.standard_normal((3, T))
    alpha, beta = rng.uniform(2.0, 8.0, 3), rng.uniform(0.2, 1.0, 3)
    lit = R.activation1d(x, alpha, beta)
    assert lit.shape == (3, T)
    scale = np.abs(lit).max()
    assert np.abs(R.aa_gather(x, alpha, beta) - lit).max() < 1e-13 * scale
    wrong = np.abs(R.aa_gather(x, alpha, beta, mutate=True) - lit).max()
    if T == 1:
        # a one-column row is constant under edge padding and each phase of the symmetric filter sums to 1 / 2: u is that constant at
        # every n, inside the row or beyond it, so the two forms are the same function there and no input can tell them apart
        assert wrong < 1e-13 * scale
    else:
        assert wrong > 1e-4 * scale


def test_filter_matches_scipy_and_sums_to_one():
    f = R.kaiser_sinc_filter(0.25, 0.3, 12)
    assert f.shape == (12,) and abs(f.sum() - 1.0) < 1e-15
    assert np.abs(f - scipy_filter()).max() < 1e-12
    assert np.array_equal(f, f[::-1]) or np.abs(f - f[::-1]).max() < 1e-16


# ---------------------------------------------------------------------------------------------- host mirror
def test_config_keys_and_defaults():
    d = dict(num_mels=100, upsample_rates=[4, 4, 2, 2, 2, 2], upsample_kernel_sizes=[8, 8, 4, 4, 4, 4], upsample_initial_channel=1536,
             resblock="1", resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3, activation="snakebeta",
             snake_logscale=True)
    c = mas.BigVGANConfig.from_dict(d)
    assert c.use_bias_at_final is True and c.use_tanh_at_final is True and c.resblock == "1" and c.hop_length == 256
    c2 = mas.BigVGANConfig.from_dict(dict(d, resblock="2", use_bias_at_final=False, use_tanh_at_final=False, unknown_key=1), max_batch=2)
    assert (c2.resblock, c2.use_bias_at_final, c2.use_tanh_at_final, c2.max_batch) == ("2", False, False, 2)
    cc = c.to_c()
    assert (cc.num_mels, cc.n_upsamples, cc.resblock, cc.activation, cc.snake_logscale, cc.use_tanh_at_final) == (100, 6, 1, 1, 1, 1)
    assert list(cc.upsample_kernel_sizes)[:6] == [8, 8, 4, 4, 4, 4] and list(cc.resblock_dilation_sizes[2])[:3] == [1, 3, 5]
    assert C.sizeof(_lib.BigVGANConfigC) == 4 * (1 + 9 + 9 + 1 + 1 + 9 + 8 + 64 + 4 + 2)
    for miss in ("num_mels", "resblock", "activation", "snake_logscale"):
        with pytest.raises(mas.AudioGenerationError):
            mas.BigVGANConfig.from_dict({k: v for k, v in d.items() if k != miss})
    with pytest.raises(mas.AudioGenerationError):
        mas.BigVGANConfig.from_dict(dict(d, resblock="3"))
    with pytest.raises(mas.AudioGenerationError):
        mas.BigVGANConfig.from_dict(dict(d, activation="relu"))


def test_sanitize_layouts():
    cfg = small_config()
    want = mas.bigvgan_expected_shapes(cfg)
    _, sd, _ = torch_checkpoint(cfg, 3)
    assert tuple(sd["conv_pre.weight_v"].shape) == (32, 8, 7) and tuple(sd["ups.0.0.weight_v"].shape) == (32, 16, 8)
    assert tuple(sd["ups.0.0.weight_g"].shape) == (32, 1, 1)
    out = mas.bigvgan_sanitize(cfg, sd)
    assert not [k for k in out if "num_batches_tracked" in k]
    assert {k: tuple(v.shape) for k, v in out.items()} == want
    assert torch.equal(out["conv_pre.weight_v"], sd["conv_pre.weight_v"].permute(0, 2, 1))
    assert torch.equal(out["ups.0.0.weight_v"], sd["ups.0.0.weight_v"].permute(1, 2, 0))
    assert torch.equal(out["ups.0.0.weight_g"].reshape(-1), sd["ups.0.0.weight_g"].reshape(-1))
    again = mas.bigvgan_sanitize(cfg, out)                                # already-correct shapes are untouched
    assert all(again[k] is out[k] for k in out)
    extra = mas.bigvgan_sanitize(cfg, {"somewhere.conv.weight": torch.zeros(2, 3, 4)})
    assert tuple(extra["somewhere.conv.weight"].shape) == (2, 3, 4)      # a key the model does not have passes as it is


def test_snake_has_no_beta():
    s = mas.bigvgan_expected_shapes(small_config(activation="snake"))
    assert "activation_post.act.alpha" in s and not [k for k in s if k.endswith(".beta")]
    b = mas.bigvgan_expected_shapes(small_config())
    assert b["resblocks.0.activations.5.act.beta"] == (16,) and b["ups.1.0.weight_g"] == (1, 1, 16) and "conv_post.bias" not in b
    two = mas.bigvgan_expected_shapes(small_config(resblock="2", use_bias_at_final=True))
    assert "resblocks.5.convs.2.weight_v" in two and "resblocks.0.convs1.0.weight_v" not in two and two["conv_post.bias"] == (1,)


@pytest.mark.parametrize("mels,rates,kernels,hop", [(80, [4, 4, 2, 2, 2, 2], [8, 8, 4, 4, 4, 4], 256),
                                                    (128, [8, 4, 2, 2, 2, 2], [16, 8, 4, 4, 4, 4], 512)])
def test_output_length_of_the_published_configs(mels, rates, kernels, hop):
    """Config arithmetic only: 22 kHz / 80 bands and 44 kHz / 128 bands give T x the product of the rates samples."""
    cfg = mas.BigVGANConfig(num_mels=mels, upsample_rates=rates, upsample_kernel_sizes=kernels, upsample_initial_channel=1536, resblock="1",
                            resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3, activation="snakebeta", snake_logscale=True)
    assert cfg.hop_length == hop
    n = 7
    for s, k in zip(rates, kernels):                                     # a transposed conv of kernel k, stride s, padding (k - s) / 2
        n = (n - 1) * s - 2 * ((k - s) // 2) + k
    assert n == 7 * hop
    s = mas.bigvgan_expected_shapes(cfg)
    assert s["conv_pre.weight_v"] == (1536, 7, mels) and s["conv_post.weight_v"] == (1, 7, 24) and s["ups.5.0.weight_v"] == (24, 4, 48)


def test_kernel_other_than_twice_the_stride_is_refused():
    """Judged before the device is touched, so the refusal is the same with and without a GPU."""
    for kw in (dict(upsample_kernel_sizes=[8, 5]), dict(upsample_kernel_sizes=[16, 4]), dict(upsample_kernel_sizes=[8])):
        with pytest.raises(mas.AudioGenerationError) as e:
            mas.BigVGAN(small_config(**kw))
        assert e.value.case == "invalidInput" and "upsample_kernel_sizes" in str(e.value)


# ---------------------------------------------------------------------------------------------- resources
@pytest.fixture(scope="module")
def usage():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S",
                            os.path.join(ROOT, "mlx-audio-swift_amd", "csrc", "bigvgan.hip"), "-o", os.path.join(td, "k.s"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    use, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = use.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for key, pat in (("vgprs", r"remark:\s+VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m:
                cur[key] = int(m.group(1))
    return use


def test_bigvgan_kernels_do_not_spill(usage):
    """No kernel of bigvgan.hip uses scratch and every one fits 64 KiB of LDS; the 64 x 64 conv tile stays within 128 VGPRs, four of
    its waves per SIMD."""
    mine = {k: v for k, v in usage.items() if "k_bv_" in k}
    for name in ("k_bv_aa_act", "k_bv_conv", "k_bv_mean", "k_bv_final"):
        assert any(name in k for k in mine), name
    for k, v in mine.items():
        assert v["scratch"] == 0, (k, v)
        assert v["lds"] <= 65536, (k, v)
        if "k_bv_conv" in k:
            assert v["vgprs"] <= 128, (k, v)
