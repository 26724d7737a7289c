// MFMA attention core of the bf16x3 precision (split-f32 operands, common.h `sf32`; f32 arithmetic): the split-f32 instantiation of attn_core.h.
// Every product is formed as hi*hi + hi*lo + lo*hi: the Q / K / V / dO fragments come as (hi, lo) pairs straight from the split layout (a head's 64 dims
// are two 128-byte lines [32 hi | 32 lo]), the probabilities / dS / dropout(P) are split in registers after the f32 softmax arithmetic.  The bf16 kernels
// keep their matrix pipe 3-5 % busy, so tripling the MFMAs is cheap next to the doubled operand bytes.
#include "attn_core.h"

struct AttnSplitF32 {
    typedef sf32 elem;
    static constexpr int PLANES = 2;      // hi, lo
    static __device__ __forceinline__ void split(float x, bf16_t* o) { sf_split(x, o[0], o[1]); }
    // c += A * B on split operands: the two cross terms first, the leading term last
    static __device__ __forceinline__ f32x4 mma(const frag8<2>& A, const frag8<2>& B, f32x4 c) {
        c = MFMA(A.p[1], B.p[0], c);
        c = MFMA(A.p[0], B.p[1], c);
        return MFMA(A.p[0], B.p[0], c);
    }
    // operand check: every row is whole 128-byte lines, and so is every operand's start
    static constexpr const char* NAME = "x3";
    static constexpr int LD_MULT = 32, OUT_LD_MULT = 32, ALIGN = 128, OUT_ALIGN = 128;
};

ATTN_CORE_UNIT(sf32, AttnSplitF32, attn_fwd_x3_kernel, attn_bwd_x3_kernel, attn_fwd_x3_pair_kernel, attn_bwd_x3_pair_kernel)
