// The tap points of the layer-wise confidence branch (reference tasks/gqa_branched_layer.py:47-59, :104-110, :313-320; rgqa_config.conf_branch = 2): the head
// reads the [CLS] row of EVERY cross-modality layer's language output, so the engine needs those rows out of the recorded forward and their gradients back into
// the single encoder backward.
//   gather   taps[i][b][:] = x<i>_lang[row_i(b)][:] for all X layers in ONE launch                    forward, behind the encoder
//   inject   dy[row(b)][:] += dtap[b][:]            one layer per launch                              backward, in front of the layer's FFN stage
// row(b) = cu ? cu[b] : b * stride_rows (padded / packed language rows); a layer whose rows are already the B compact [CLS] rows (the last layer under the
// [CLS]-tail) has row(b) = b.  Both are pure data movement: one wave per row, 16 bytes per lane and access, no LDS, no atomics.
// gather copies the row's bytes unchanged, whatever the element type (split-f32 rows are whole 128-byte lines: [32 hi | 32 lo], so the copy keeps both parts bit
// for bit); for split-f32 rows it can also leave their bf16 image (the hi parts, what the bf16 backward of the bf16x3_fwd precision reads) - chunk c of a row's
// lines (16 bytes) is a hi chunk when (c & 7) < 4 and lands at 16-byte chunk (c >> 3) * 4 + (c & 3) of the image row.
// inject adds in f32 and rounds once to the gradient's element type.
#include <type_traits>
#include "kernels.h"
#include "layer_taps.h"

#define TAP_T 256             // 4 waves = 4 rows per workgroup

struct alignas(16) TapChunk { uint32_t w[4]; };

__global__ __launch_bounds__(TAP_T) void tap_gather_kernel(const TapSrcs srcs, int X, int B, const int* __restrict__ cu, int stride_rows, int row_bytes,
                                                           unsigned char* __restrict__ dst, unsigned char* __restrict__ img) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (TAP_T / 64) + (threadIdx.x >> 6);      // (layer, sample)
    if (r >= X * B) return;
    const int i = r / B, b = r % B;
    const size_t row = srcs.compact[i] ? (size_t)b : (cu ? (size_t)cu[b] : (size_t)b * stride_rows);
    const TapChunk* sp = reinterpret_cast<const TapChunk*>(reinterpret_cast<const unsigned char*>(srcs.p[i]) + row * row_bytes);
    TapChunk* dp = reinterpret_cast<TapChunk*>(dst + (size_t)r * row_bytes);
    TapChunk* ip = img ? reinterpret_cast<TapChunk*>(img + (size_t)r * (row_bytes >> 1)) : nullptr;
    const int nch = row_bytes >> 4;
    for (int c = lane; c < nch; c += 64) {
        const TapChunk v = sp[c];
        dp[c] = v;
        if (ip != nullptr && (c & 7) < 4) ip[(c >> 3) * 4 + (c & 3)] = v;
    }
}

// VE consecutive elements of type T <-> f32, one 16-byte access per lane where the type has one (float: 4 elements; bf16: 8; split f32: 8 as two 16-byte
// accesses, hi and lo); the host emulation of the tests runs the float form and compiles the others element by element
template <typename T> struct TapVec {
    static constexpr int VE = 1;
    static __device__ __forceinline__ void load(const T* p, float* v) { v[0] = ld_elem(p); }
    static __device__ __forceinline__ void store(T* p, const float* v) { st_elem(p, v[0]); }
};
template <> struct TapVec<float> {
    static constexpr int VE = 4;
    static __device__ __forceinline__ void load(const float* p, float* v) { load4(p, v); }
    static __device__ __forceinline__ void store(float* p, const float* v) { store4(p, v); }
};
#if defined(__HIPCC__)
template <> struct TapVec<bf16_t> {
    static constexpr int VE = 8;
    static __device__ __forceinline__ void load(const bf16_t* p, float* v) {
        const bf16x8 t = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (float)t[i];
    }
    static __device__ __forceinline__ void store(bf16_t* p, const float* v) {
        bf16x8 t;
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i] = (bf16_t)v[i];
        *reinterpret_cast<bf16x8*>(p) = t;
    }
};
template <> struct TapVec<sf32> {
    static constexpr int VE = 8;
    static __device__ __forceinline__ void load(const sf32* p, float* v) { sf_load8(p, v); }
    static __device__ __forceinline__ void store(sf32* p, const float* v) { sf_store8(p, v); }
};
#endif

template <typename T>
__global__ __launch_bounds__(TAP_T) void tap_inject_kernel(const T* __restrict__ dtap, int ldt, T* __restrict__ dy, int ldy, const int* __restrict__ cu, int stride_rows,
                                                           int B, int cols) {
    constexpr int VE = TapVec<T>::VE;
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (TAP_T / 64) + (threadIdx.x >> 6);
    if (b >= B) return;
    const size_t row = cu ? (size_t)cu[b] : (size_t)b * stride_rows;
    const T* sp = dtap + (size_t)b * ldt;
    T* dp = dy + row * ldy;
    // (left to itself the loop vectoriser interleaves two trips of the float form and takes its 16-byte stores apart into dword stores)
#pragma clang loop vectorize(disable) interleave(disable)
    for (int c = lane * VE; c < cols; c += 64 * VE) {
        float a[VE], g[VE];
        TapVec<T>::load(dp + c, a);
        TapVec<T>::load(sp + c, g);
#pragma unroll
        for (int k = 0; k < VE; ++k) a[k] += g[k];
        TapVec<T>::store(dp + c, a);
    }
}

int k_tap_gather(const TapSrcs& srcs, int X, int B, const int* cu, int stride_rows, int row_bytes, void* dst, void* img, hipStream_t s) {
    RGQA_REQUIRE(X >= 1 && X <= TAP_MAX_LAYERS && B > 0 && dst != nullptr, "tap_gather: bad shape X=%d B=%d (X <= %d)", X, B, TAP_MAX_LAYERS);
    RGQA_REQUIRE(row_bytes > 0 && row_bytes % 16 == 0 && ((uintptr_t)dst & 15) == 0, "tap_gather: rows must be whole 16-byte chunks (row_bytes=%d)", row_bytes);
    RGQA_REQUIRE(img == nullptr || (row_bytes % 128 == 0 && ((uintptr_t)img & 15) == 0), "tap_gather: the bf16 image needs split-f32 rows of whole 128-byte lines (row_bytes=%d)", row_bytes);
    for (int i = 0; i < X; ++i)
        RGQA_REQUIRE(srcs.p[i] != nullptr && ((uintptr_t)srcs.p[i] & 15) == 0, "tap_gather: source %d is null or not 16-byte aligned", i);
    hipLaunchKernelGGL(tap_gather_kernel, dim3(cdiv((long)X * B, TAP_T / 64)), dim3(TAP_T), 0, s, srcs, X, B, cu, stride_rows, row_bytes, (unsigned char*)dst,
                       (unsigned char*)img);
    RGQA_LAUNCH_CHECK("tap_gather_kernel");
    return RGQA_OK;
}

template <typename T>
int k_tap_inject(const T* dtap, int ldt, T* dy, int ldy, const int* cu, int stride_rows, int B, int cols, hipStream_t s) {
    RGQA_REQUIRE(dtap != nullptr && dy != nullptr && B > 0 && cols > 0, "tap_inject: bad argument (B=%d cols=%d)", B, cols);
    // whole vectors of 8 elements whatever the type (float moves 4 per access): rows of the encoder's hidden size
    RGQA_REQUIRE(cols % 8 == 0 && ldt % 8 == 0 && ldy % 8 == 0 && ldt >= cols && ldy >= cols && ((uintptr_t)dtap & 15) == 0 && ((uintptr_t)dy & 15) == 0,
                 "tap_inject: cols, ldt, ldy must be multiples of 8 and the rows 16-byte aligned (cols=%d ldt=%d ldy=%d)", cols, ldt, ldy);
    if (std::is_same<T, sf32>::value)
        RGQA_REQUIRE(cols % 32 == 0 && ldt % 32 == 0 && ldy % 32 == 0 && ((uintptr_t)dtap & 127) == 0 && ((uintptr_t)dy & 127) == 0, "tap_inject: split-f32 rows must be whole 128-byte lines");
    hipLaunchKernelGGL(tap_inject_kernel<T>, dim3(cdiv(B, TAP_T / 64)), dim3(TAP_T), 0, s, dtap, ldt, dy, ldy, cu, stride_rows, B, cols);
    RGQA_LAUNCH_CHECK("tap_inject_kernel");
    return RGQA_OK;
}
template int k_tap_inject<float>(const float*, int, float*, int, const int*, int, int, int, hipStream_t);
template int k_tap_inject<bf16_t>(const bf16_t*, int, bf16_t*, int, const int*, int, int, int, hipStream_t);
template int k_tap_inject<sf32>(const sf32*, int, sf32*, int, const int*, int, int, int, hipStream_t);
