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


ENGINES = dict(lasr=lasr, fsmn_vad=fsmn_vad, ecapa_lid=ecapa_lid, moonshine=moonshine)


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
