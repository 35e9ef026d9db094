"""-m gpu: the outputs of the small audio engines on synthetic models, bit for bit against tests/golden/front_bits.json.

The FFT twiddles, the filter bin ranges and the block reductions are shared between engines (csrc/audio_front.h, csrc/common.h), and so
are pieces of the exact-f32 MFMA contraction of the four f32 engines (csrc/f32_tile.h: the 16-step MFMA loop, the zero-tile exit, the
C/D row map) with the per-frame mean / rstd of common.h; the staging loops of the contractions and the FFT butterfly loops exist once
per engine.  What these engines promise is a row's bits in any batch, and the time: after a change to a shared piece, or to one copy,
no output may move.  Every entry was recorded from kernels that shared none of this (mossformer2 and sortformer from each file's own
copy of the contraction, before f32_tile.h), so a change to a shared piece, or to one kernel, that moves a bit of any engine fails here.
tools/record_front_bits.py holds the cases (and says which path each shape reaches) and regenerates the file when numerics change on
purpose."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("record_front_bits", os.path.join(ROOT, "tools", "record_front_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "front_bits.json")) as f:
        return json.load(f)


def test_the_golden_file_covers_every_engine():
    assert sorted(_golden()) == sorted(_tool().ENGINES)


@pytest.mark.parametrize("engine", ["lasr", "fsmn_vad", "ecapa_lid", "moonshine", "mossformer2", "sortformer"])
def test_outputs_match_the_recorded_bits(engine):
    want, got = _golden()[engine], _tool().ENGINES[engine]()
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name] == want[name], f"{engine}.{name}: {got[name]} != recorded {want[name]}"


def test_sortformer_and_lasr_share_one_log_mel_front_end():
    """The two NeMo front ends are one pair of kernels (csrc/audio_front.h).  With the same mel count, peak normalisation off (a scale of
    one), pre-emphasis 0.97 and pad_to 0, Sortformer's features are LASR's bit for bit: one frame, one hop, the window and several frames
    in one ragged batch, with junk behind every row."""
    import numpy as np

    import mlx_audio_swift_amd as mas
    tool = _tool()
    r = tool.rows([1, 159, 400, 4000])
    enc = mas.LasrEncoderConfig(hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=64, conv_kernel_size=4,
                                num_mel_bins=80, subsampling_conv_channels=32)
    ls = mas.LasrCTCModel.synthetic(mas.LasrCTCConfig(vocab_size=32, encoder_config=enc, max_batch=4, max_seconds=1), seed=tool.SEED)
    try:
        want = ls.features(r, junk=1e30)
    finally:
        ls.close()
    e = mas.FCEncoderConfig(hidden_size=48, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2, intermediate_size=80,
                            num_mel_bins=80, subsampling_conv_channels=24)
    t = mas.TFEncoderConfig(d_model=40, encoder_layers=1, encoder_attention_heads=2, encoder_ffn_dim=72)
    cfg = mas.SortformerConfig(fc_encoder_config=e, tf_encoder_config=t, modules_config=mas.ModulesConfig(num_speakers=4, fc_d_model=48, tf_d_model=40),
                               processor_config=mas.ProcessorConfig(feature_size=80, preemphasis=0.97), max_batch=4, max_seconds=1)
    sf = mas.SortformerModel.synthetic(cfg, seed=tool.SEED)
    try:
        got = sf.features(r, peak_normalize=False, normalize=True, pad_to=0, junk=1e30)
    finally:
        sf.close()
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (4, 26, 80)
    assert got.tobytes() == want.tobytes()
