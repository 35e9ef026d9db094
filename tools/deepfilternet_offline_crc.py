"""CRC-32 of what DeepFilterNet.enhance_raw returns for the eight rows of tests/deepfilternet_ref.rows on cases S and W, one JSON line a
row: the list a change that must not move the offline numerics is checked with (run on the commit before and after, compare the files).

    python tools/deepfilternet_offline_crc.py --out profiles/deepfilternet_stream/offline_crc_branch.jsonl"""
import argparse
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mlx_audio_swift_amd as mas  # noqa: E402
import deepfilternet_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for name in ("S", "W"):
            cfg, W = R.case(name)
            wav, lsnr = mas.DeepFilterNet.from_weights(cfg, W).enhance_raw(R.rows(cfg), junk=np.nan)
            for b, (w, l) in enumerate(zip(wav, lsnr)):
                line = dict(case=name, row=b, samples=len(w), frames=len(l), waveform_crc32=zlib.crc32(np.ascontiguousarray(w).tobytes()),
                            lsnr_crc32=zlib.crc32(np.ascontiguousarray(l).tobytes()))
                print(json.dumps(line))
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
