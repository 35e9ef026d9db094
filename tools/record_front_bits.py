"""sha256 of the raw output bytes of the small audio engines on synthetic (init_synthetic) models -> tests/golden/front_bits.json.

    python tools/record_front_bits.py [--out tests/golden/front_bits.json]

tests/test_gpu_front_bits.py recomputes the same hashes and asserts equality: the shared front-end pieces (the tables of
csrc/audio_front.h, the block reductions of common.h) serve several engines, and a change to one of them must not move a bit of any.
Regenerate the file only when numerics change on purpose, and say why in that commit.

The shapes are the smallest that reach every path of the front ends and of the exact-f32 contractions:
  lasr       128 mels, hidden 64, 1 layer.  features on rows of 1, 159, 400 and 4000 samples (one frame, one hop, the window); forward
             on rows of 1920 and 4000 samples: the conv stem (kernel 5, stride 2) rejects a row below 13 feature frames = 1920 samples
  fsmn_vad   features / scores / silence + decibel; rows of 399, 400 and 4000 samples (no frame, one, several); chunk_frames 16, so the
             longest row spans two chunks and both GEMM tiles and the softmax epilogue run
  ecapa_lid  log_probs / embedding, 60 mels (the edge guards of the GEMM); rows of 160, 1700 and 4000 samples
  moonshine  encode, rows of 895 and 3000 samples
  mossformer2  one block at out_channels 16 (the smallest width the config check takes), otherwise the smallest model of
             tests/test_gpu_mossformer2.py: 16 kHz, window 320, hop 64, 20 mels, so the feature width 60 runs the K guard and 161 bins the N
             guard.  Rows of 319, 320 and 320 + 256 x 64 samples: no frame, one, and 257, which is two groups of k_mf2_linkv and five row
             tiles, whose last four are zero tiles for the short rows.  enhance passes through the six loads (activations, token shift,
             LayerNorm, gate, frame, masked) and the row-scale, column-scale, PReLU and tanh | sigmoid epilogues; mask and features are
             digested on the way
  sortformer   one Conformer block (48 / 2 heads / 80, stem 24 channels, 80 mels) and one BART layer (40 / 2 heads / 72), 4 speakers: no width
             is a multiple of 32.  Rows of 0, 3000 and 81920 samples at pad_to 0: F = 1, 19, 513 and T = 1, 3, 65, so the encoder GEMMs have
             a second row tile that is a zero tile for the short rows.  forward runs the plain, LayerNorm and ReLU loads and the R + a v and
             positional epilogues; pre_encode of the features runs the depthwise-conv load with rowmul > 1 rows
The waveforms come from integer arithmetic alone, so they are the same bytes on every machine."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "front_bits.json")
SEED = 777


def wave(n: int, seed: int) -> np.ndarray:
    """n samples in [-0.25, 0.25): a multiplicative hash of the index, exact in float64."""
    i = np.arange(n, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(40503 * (seed + 1))) & np.uint64(0xFFFFFFFF)
    h = ((h ^ (h >> np.uint64(15))) * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    return ((h.astype(np.float64) / 4294967296.0 - 0.5) * 0.5).astype(np.float32)


def rows(lens):
    return [wave(n, k) for k, n in enumerate(lens)]


def digest(a) -> dict:
    a = np.ascontiguousarray(a)
    return dict(dtype=str(a.dtype), shape=list(a.shape), sha256=hashlib.sha256(a.tobytes()).hexdigest())


def lasr() -> dict:
    import mlx_audio_swift_amd as mas
    enc = mas.LasrEncoderConfig(hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=64, conv_kernel_size=4,
                                num_mel_bins=128, subsampling_conv_channels=32)
    m = mas.LasrCTCModel.synthetic(mas.LasrCTCConfig(vocab_size=32, encoder_config=enc, max_batch=4, max_seconds=1), seed=SEED)
    try:
        return dict(features=digest(m.features(rows([1, 159, 400, 4000]))), forward=digest(m.forward(rows([1920, 4000]))))
    finally:
        m.close()


def fsmn_vad() -> dict:
    import mlx_audio_swift_amd as mas
    enc = mas.FSMNVADEncoderConfig(input_dim=400, input_affine_dim=24, fsmn_layers=2, linear_dim=40, proj_dim=16, lorder=3,
                                   output_affine_dim=20, output_dim=7)
    m = mas.FSMNVAD.synthetic(mas.FSMNVADConfig(encoder=enc, max_batch=4, chunk_frames=16), seed=SEED)
    try:
        r = rows([399, 400, 4000])
        feats, R = m.features_raw(r)
        scores, _ = m.scores_raw(r)
        sil, dec, _, T = m.detect_raw(r)
        return dict(features=digest(feats), scores=digest(scores), silence=digest(sil), decibel=digest(dec), rows=digest(R), frames=digest(T))
    finally:
        m.close()


def ecapa_lid() -> dict:
    import mlx_audio_swift_amd as mas
    cfg = mas.EcapaTdnnConfig(n_mels=60, channels=64, attention_channels=16, se_channels=16, embedding_dim=32, classifier_hidden_dim=64,
                              num_classes=10, max_batch=4, max_samples=4000)
    m = mas.EcapaTdnnLID.synthetic(cfg, seed=SEED)
    try:
        logp, emb, _, _ = m.predict_raw(rows([160, 1700, 4000]), 0)
        return dict(log_probs=digest(logp), embedding=digest(emb))
    finally:
        m.close()


def moonshine() -> dict:
    import mlx_audio_swift_amd as mas
    cfg = mas.MoonshineConfig(vocab_size=2048, hidden_size=288, intermediate_size=1152, encoder_num_hidden_layers=1,
                              decoder_num_hidden_layers=1)
    m = mas.MoonshineModel.synthetic(cfg, seed=SEED)
    try:
        out = m.encode(rows([895, 3000]))
        return {f"encode_row{b}": digest(o) for b, o in enumerate(out)}
    finally:
        m.close()


def mossformer2() -> dict:
    import mlx_audio_swift_amd as mas
    cfg = mas.MossFormer2SEConfig(sample_rate=16000, win_len=320, win_inc=64, fft_len=320, num_mels=20, in_channels=60, out_channels=16,
                                  out_channels_final=161, num_blocks=1, max_batch=4, max_seconds=1.1)
    m = mas.MossFormer2SE.synthetic(cfg, seed=SEED)
    try:
        r = rows([319, 320, 320 + 256 * 64])
        feats, T = m.features_raw(r)
        mask, _ = m.mask_raw(r)
        out = {f"enhance_row{b}": digest(o) for b, o in enumerate(m.enhance_batch(r))}
        return dict(out, features=digest(feats), mask=digest(mask), frames=digest(T))
    finally:
        m.close()


def sortformer() -> dict:
    import mlx_audio_swift_amd as mas
    e = mas.FCEncoderConfig(hidden_size=48, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2, intermediate_size=80,
                            num_mel_bins=80, subsampling_conv_channels=24)
    t = mas.TFEncoderConfig(d_model=40, encoder_layers=1, encoder_attention_heads=2, encoder_ffn_dim=72)
    cfg = mas.SortformerConfig(fc_encoder_config=e, tf_encoder_config=t, modules_config=mas.ModulesConfig(num_speakers=4, fc_d_model=48, tf_d_model=40),
                               processor_config=mas.ProcessorConfig(feature_size=80), max_batch=4, max_seconds=6)
    m = mas.SortformerModel.synthetic(cfg, seed=SEED)
    try:
        r = rows([0, 3000, 81920])
        F, T = m.frames([len(x) for x in r], 0)
        feats = m.features(r, pad_to=0)
        return dict(forward=digest(m.forward(r, pad_to=0)), features=digest(feats), pre_encode=digest(m.pre_encode(feats, F)),
                    feature_frames=digest(F), frames=digest(T))
    finally:
        m.close()


ENGINES = dict(lasr=lasr, fsmn_vad=fsmn_vad, ecapa_lid=ecapa_lid, moonshine=moonshine, mossformer2=mossformer2, sortformer=sortformer)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    got = {name: fn() for name, fn in ENGINES.items()}
    with open(args.out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(got, sort_keys=True))


if __name__ == "__main__":
    main()
