// quant_intake.h - one intake for a Linear / Embedding in MLX's affine-quantised form (mlx quantize: `weight` uint32 [N, K*bits/32],
// `scales` / `biases` [N, K/group]): the argument check, the staged device copy with its dequantiser, and the rule for what the
// code-streaming GEMMs (lm_qgemm.hip) take as it is.  Used by the LM handle, Whisper, Qwen3-TTS and Marvis; Soprano's decoder widens on
// the host in float32 (soprano.hip) and takes the argument check only.
#pragma once
#include "common.h"
#include "lm_kernels.h"

// everything launch_dequant_affine (and the host widening) relies on
static inline void quant_check_args(const char* name, mis_dtype sb_dtype, int64_t N, int64_t K, int group_size, int bits) {
    MIS_REQUIRE(bits == 2 || bits == 4 || bits == 8, MIS_ERR_INVALID_INPUT, "unsupported quantisation width %d (2, 4 or 8 bits)", bits);
    MIS_REQUIRE(group_size >= 1 && N >= 1 && K >= 1 && K % group_size == 0 && K % (32 / bits) == 0, MIS_ERR_INVALID_INPUT,
                "bad quantised shape for %s", name);
    MIS_REQUIRE(sb_dtype == MIS_F32 || sb_dtype == MIS_F16 || sb_dtype == MIS_BF16, MIS_ERR_INVALID_INPUT, "unsupported scale dtype");
}

enum { QUANT_SB_BF16 = 1 << MIS_BF16, QUANT_SB_F16 = 1 << MIS_F16 };       // scale dtypes a streaming kernel reads
// 8 / 4 bit, group 64, whole 64-wide k-blocks, scales in one of sb_set: the form k_gemm_skinny_q streams.  MIS_QUANT_NATIVE=0: nothing is.
static inline bool quant_streamable(int bits, int group_size, int64_t K, mis_dtype sb_dtype, unsigned sb_set) {
    static const bool native = !(getenv("MIS_QUANT_NATIVE") && atoi(getenv("MIS_QUANT_NATIVE")) == 0);
    return native && (bits == 8 || bits == 4) && group_size == 64 && K % 64 == 0 && ((sb_set >> (int)sb_dtype) & 1u);
}

// codes | scales | biases of one matrix in one device buffer
struct QuantStaged {
    DevBuf<uint8_t> buf;
    int64_t N = 0, K = 0;
    int group = 0, bits = 0;
    mis_dtype sbt = MIS_BF16;
    size_t sc_off = 0, bi_off = 0;           // byte offsets of scales and biases
    const uint32_t* wq() const { return reinterpret_cast<const uint32_t*>(buf.p); }
    const void* sc() const { return buf.p + sc_off; }
    const void* bi() const { return buf.p + bi_off; }
    // host or device pointers; the copies are asynchronous on s (checked arguments: quant_check_args)
    void stage(const uint32_t* codes, const void* scales, const void* biases, mis_dtype sb_dtype, int64_t N_, int64_t K_, int group_size,
               int bits_, hipStream_t s) {
        N = N_; K = K_; group = group_size; bits = bits_; sbt = sb_dtype;
        const size_t words = (size_t)N * K * bits / 32, sb_bytes = (size_t)N * (K / group) * (sbt == MIS_F32 ? 4 : 2);
        sc_off = round_up(words * 4, 256); bi_off = sc_off + round_up(sb_bytes, 256);
        buf.alloc(bi_off + sb_bytes);
        HIP_CHECK(hipMemcpyAsync(buf.p, codes, words * 4, hipMemcpyDefault, s));
        HIP_CHECK(hipMemcpyAsync(buf.p + sc_off, scales, sb_bytes, hipMemcpyDefault, s));
        HIP_CHECK(hipMemcpyAsync(buf.p + bi_off, biases, sb_bytes, hipMemcpyDefault, s));
    }
    // bf16 rows [N][K] of s * q + b
    void dequantise(bf16_t* rows, hipStream_t s) const {
        launch_dequant_affine(wq(), sc(), bi(), (int)sbt, rows, (int)N, (int)K, group, bits, s);
    }
};
