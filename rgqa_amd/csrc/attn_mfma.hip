// MFMA attention core, bf16 operands (f32 softmax): the bf16 instantiation of attn_core.h.
// An operand is one bf16 plane, a product one MFMA, the pack step a rounding; rows are 128-byte head slices.
#include "attn_core.h"

struct AttnBf16 {
    typedef bf16_t elem;
    static constexpr int PLANES = 1;
    static __device__ __forceinline__ void split(float x, bf16_t* o) { o[0] = (bf16_t)x; }
    static __device__ __forceinline__ f32x4 mma(const frag8<1>& A, const frag8<1>& B, f32x4 c) { return MFMA(A.p[0], B.p[0], c); }
    // operand check: input strides in elements, input pointers in bytes (16-byte fragment loads); gradient / output strides.  The output pointers have
    // never been constrained here (OUT_ALIGN 1)
    static constexpr const char* NAME = "mfma";
    static constexpr int LD_MULT = 8, OUT_LD_MULT = 4, ALIGN = 16, OUT_ALIGN = 1;
};

ATTN_CORE_UNIT(bf16_t, AttnBf16, attn_fwd_mfma_kernel, attn_bwd1_mfma_kernel, attn_fwd_mfma_pair_kernel, attn_bwd1_mfma_pair_kernel)
