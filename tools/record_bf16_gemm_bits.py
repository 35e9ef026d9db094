"""sha256 of the raw output bytes of the bf16 big GEMMs on Gaussian-like operands -> tests/golden/bf16_gemm_bits.json.

    python tools/record_bf16_gemm_bits.py [--out tests/golden/bf16_gemm_bits.json]

tests/test_gpu_bf16_gemm_bits.py recomputes the same hashes and asserts equality.  The Whisper big GEMMs (csrc/whisper_kernels.hip:
k_gemm_big / k_gemm_big2 / k_gemm_big3) and the LASR GEMM (csrc/lasr.hip: k_lasr_gemm) are close relatives: k_gemm_big and k_lasr_gemm
share their main loop through csrc/bf16_tile.h, the three Whisper kernels share one epilogue, and all four the bf16 quad pack.  The
operator tests (tests/test_gpu_enc_ops.py,
tests/test_gpu_lasr_ops.py) compare bit for bit on operands whose sums are exact in any order; on operands whose sums round they hold a
bound only.  Here the sums round: a change to the k order, to a rounding point of an epilogue or to the staging of an edge tile moves a
hash.  The file was recorded from the kernels as they stood before bf16_tile.h, each with its own copy of the loop and the epilogue.
Regenerate it only when numerics change on purpose, and say why in that commit.

Only the mis_debug_* entry points are driven, through tests/enc_ref.run_gemm and tests/lasr_ops_ref.run_gemm.  The cases are the smallest
that reach every instantiation and edge:
  k_gemm_big    the four epilogues at M 130, N 132, K 96: K % 64 != 0, one full and one edge tile each way, pos_rows 7 wraps inside a tile;
                one case with ldx 48 < K (rows that overlap, as in the Moonshine convs)
  k_gemm_big2   MIS_GEMM_BIG3=0, the same M and N at K 128 and 192 (an even and an odd count of 64-wide k-tiles); every (epilogue, K)
                once with and once without a bias
  k_gemm_big3   MIS_GEMM_BIG3=2: M 258, N 260, K 128 on the <4, 2> wave grid, M 17, N 4096, K 128 on the <2, 4> one
  k_lasr_gemm   the five epilogues on both tiles at M 130, N 132, K 96; LG_F32 also at N 131; LG_SILU with row counts that mask rows inside
                a tile and a whole tile (Tp 64, counts 3, 0, 1 on the 64-tile; Tp 128, counts 0, 5 on the 128-tile); LG_AXPBY in place
Each entry keeps what the launch reported ("ran": kernel, epilogue, WM, WN / epilogue, TI), so the file itself says which
instantiations it covers.

The operands are sums of four 6-bit fields of an integer hash of the element index (Irwin-Hall, close to Gaussian), scaled by a power of
two: at most seven significant bits, so exact in bf16, and the same bytes on every machine."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden", "bf16_gemm_bits.json")


def gauss(shape, seed: int, log2_scale: int) -> np.ndarray:
    """float64 values k 2^log2_scale, k an integer in [-126, 126] of standard deviation 37: a hash of the index, four 6-bit fields summed"""
    i = np.arange(int(np.prod(shape)), dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(40503 * (seed + 1))) & np.uint64(0xFFFFFFFF)
    h = ((h ^ (h >> np.uint64(15))) * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    k = sum(((h >> np.uint64(s)) & np.uint64(63)).astype(np.int64) for s in (0, 8, 16, 24)) - 126
    return (k.astype(np.float64) * 2.0 ** log2_scale).reshape(shape)


def digest(a, ran) -> dict:
    a = np.ascontiguousarray(a)
    return dict(dtype=str(a.dtype), shape=list(a.shape), sha256=hashlib.sha256(a.tobytes()).hexdigest(), ran=list(ran))


# x ~ 0.58, w ~ 0.07: sums of standard deviation about 0.5 at K 96 .. 192, the range in which GELU and SiLU bend
X_LOG2, W_LOG2, B_LOG2, R_LOG2 = -6, -9, -7, -6
EPI_NAMES = ["none", "gelu", "resid", "gelu_pos"]
LG_NAMES = ["bias", "relu", "silu", "axpby", "f32"]


def whisper_cases() -> dict:
    cases = {}

    def add(name, mode, M, N, K, epi, bias, ldx=None):
        cases[name] = dict(mode=mode, M=M, N=N, K=K, ldx=K if ldx is None else ldx, epi=epi, bias=bias, pos_rows=7, seed=100 + len(cases))

    for e, en in enumerate(EPI_NAMES):
        add(f"big_{en}", 1, 130, 132, 96, e, True)
    add("big_resid_ldx48", 1, 130, 132, 96, 2, False, ldx=48)
    for K in (128, 192):
        for e, en in enumerate(EPI_NAMES):
            add(f"big2_{en}_k{K}_bias", 0, 130, 132, K, e, True)
            add(f"big2_{en}_k{K}_nobias", 0, 130, 132, K, e, False)
    for e, en in enumerate(EPI_NAMES):
        add(f"big3_42_{en}", 2, 258, 260, 128, e, e % 2 == 0)
        add(f"big3_24_{en}", 2, 17, 4096, 128, e, e % 2 == 1)
    return cases


def run_whisper(c) -> dict:
    import enc_ref as er
    M, N, K, ldx, s = c["M"], c["N"], c["K"], c["ldx"], c["seed"]
    R = gauss((M, N), 4 * s + 3, R_LOG2) if c["epi"] == er.BG_RESID else gauss((c["pos_rows"], N), 4 * s + 3, R_LOG2) if c["epi"] == er.BG_GELU_POS else None
    d = dict(img=gauss(((M - 1) * ldx + K,), 4 * s, X_LOG2), w=gauss((N, K), 4 * s + 1, W_LOG2), bias=gauss((N,), 4 * s + 2, B_LOG2) if c["bias"] else None, R=R)
    st, out, rep = er.run_gemm(c, d)
    assert st == er.OK, f"mis_debug_gemm_big: status {st} for {c}"
    return digest(out, rep)


def lasr_cases() -> dict:
    cases = {}

    def add(name, epi, tile, N=132, cnt=None, Tp=1, in_place=False):
        cases[name] = dict(epi=epi, tile=tile, M=130, N=N, K=96, ldx=96, bias=True, a=0.75, b=0.5, cnt=cnt, Tp=Tp, in_place=in_place, seed=500 + len(cases))

    for tile in (2, 4):
        for e, en in enumerate(LG_NAMES):
            add(f"lasr_{en}_t{tile}", e, tile)
        add(f"lasr_f32_n131_t{tile}", 4, tile, N=131)
        add(f"lasr_axpby_in_place_t{tile}", 3, tile, in_place=True)
    add("lasr_silu_counts_t2", 2, 2, cnt=[3, 0, 1], Tp=64)
    add("lasr_silu_counts_t4", 2, 4, cnt=[0, 5], Tp=128)
    return cases


def run_lasr(c) -> dict:
    import gemm_ref as gr
    import lasr_ops_ref as lo
    M, N, K, s = c["M"], c["N"], c["K"], c["seed"]
    d = dict(img=gr.exact_bits(gauss((M * K,), 4 * s, X_LOG2)), w=gauss((N, K), 4 * s + 1, W_LOG2), bias=gauss((N,), 4 * s + 2, B_LOG2),
             Rb=gr.exact_bits(gauss((M, N), 4 * s + 3, R_LOG2)) if c["epi"] == lo.LG_AXPBY else None,
             cnt=None if c["cnt"] is None else np.asarray(c["cnt"], np.int32), Tp=c["Tp"])
    st, out, _, rep = lo.run_gemm(c, d, c["tile"])
    assert st == lo.OK, f"mis_debug_lasr_gemm: status {st} for {c}"
    return digest(out, rep)


def cases() -> dict:
    """name -> a function that launches the case and returns its digest"""
    out = {name: (lambda c=c: run_whisper(c)) for name, c in whisper_cases().items()}
    out.update({name: (lambda c=c: run_lasr(c)) for name, c in lasr_cases().items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    got = {name: fn() for name, fn in cases().items()}
    with open(args.out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(got, sort_keys=True))


if __name__ == "__main__":
    main()
