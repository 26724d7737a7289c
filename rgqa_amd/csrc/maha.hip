// The Mahalanobis test method (tasks/gqa_maha.py) on the device: the per-batch scorer and input step (:223-270) and the accumulate step of the
// one-off estimator (:139-168).
//
// The reference scores every class in a loop, score[b, c] = -0.5 (x_b - mu_c)^T P (x_b - mu_c), two H x H products per class.  With the precision
// matrix factored once on the host, P = W W^T (W [H, R], R = the rank pinvh keeps), the same number is
//     y = x W  [B, R],   nu = mu W  [NC, R] (once per pack),   score[b, c] = -0.5 sum_r (y[b, r] - nu[c, r])^2
// - differences first, then squares: the expanded |y|^2 - 2 y.nu + |nu|^2 form cancels and was 4-10x less accurate in f32.  The gradient of
// loss = mean_b(-score[b, pred_b]) w.r.t. the pooled vector is computed as (1 / B) W (W^T (x_b - mu_pred_b)), the difference taken in the pooled
// space as the reference takes it (y_b - nu_pred_b is the same vector in exact arithmetic, but cancels after the rounded products:
// tools/maha_precision_study.py).
//
// All arithmetic is f32 FMA on the vector ALU (f64 in the estimator), every sum runs in ascending index order in ONE accumulator owned by one
// thread, nothing is atomic: results do not depend on the engine's precision, on the tile variant chosen, or on B, and repeat bit for bit.
#include "kernels.h"
#include "../../include/rgqa.h"

// ---------------------------------------------------------------- C[b, n] = scale * sum_k A'[b, k] Bm[k, n]
// 8 rows x 64 columns per workgroup (B = 32, R = 768: 48 workgroups; B = 256: 384), K in chunks of 32 through LDS.
// TRANS = 0: Bm[k, n] = Wm[k * ldw + n] (y = x W);  TRANS = 1: Bm[k, n] = Wm[n * ldw + k] (g = W d).  SUB = 1: A'[b, k] = A[b, k] - sub[label[b], k]
// (the input step's d = (x - mu_pred) W); a label outside [0, NC) gives a row of zeros.  SUB = 0: A' = A.
#define MG_ROWS 8
#define MG_COLS 64
#define MG_K 32
template <int TRANS, int SUB>
__global__ __launch_bounds__(256) void maha_gemm_kernel(const float* __restrict__ A, int lda, const float* __restrict__ Wm, int ldw, const float* __restrict__ sub,
                                                        const int64_t* __restrict__ label, int NC, float scale, int M, int N, int K, float* __restrict__ Cm, int ldc) {
    __shared__ float as[MG_ROWS][MG_K];
    __shared__ float bs[MG_K][MG_COLS + 1];
    const int t = threadIdx.x;
    const int n0 = blockIdx.x * MG_COLS, m0 = blockIdx.y * MG_ROWS;
    const int c = t & 63, g = t >> 6;
    float acc0 = 0.f, acc1 = 0.f;
    // this thread's element of the A chunk: row t / 32, column t % 32
    const int ar = t >> 5, ak = t & 31;
    const int arow = m0 + ar;
    const float* nurow = nullptr;
    bool arow_ok = arow < M;
    if (SUB && arow_ok) {
        const int64_t l = label[arow];
        if (l >= 0 && l < NC) nurow = sub + (size_t)l * K; else arow_ok = false;
    }
    for (int k0 = 0; k0 < K; k0 += MG_K) {
        float a = 0.f;
        if (arow_ok && k0 + ak < K) {
            a = A[(size_t)arow * lda + k0 + ak];
            if (SUB) a -= nurow[k0 + ak];
        }
        as[ar][ak] = a;
        if (!TRANS) {
#pragma unroll
            for (int i = 0; i < MG_K / 4; ++i) {
                const int k = g + 4 * i;
                bs[k][c] = (k0 + k < K && n0 + c < N) ? Wm[(size_t)(k0 + k) * ldw + n0 + c] : 0.f;
            }
        } else {
#pragma unroll
            for (int i = 0; i < MG_COLS / 8; ++i) {
                const int n = ar + 8 * i;
                bs[ak][n] = (k0 + ak < K && n0 + n < N) ? Wm[(size_t)(n0 + n) * ldw + k0 + ak] : 0.f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MG_K; ++k) {
            const float b = bs[k][c];
            acc0 = fmaf(as[2 * g][k], b, acc0);
            acc1 = fmaf(as[2 * g + 1][k], b, acc1);
        }
        __syncthreads();
    }
    if (!TRANS && !SUB) {      // y = x W: a non-finite pooled value (or an overflowing product) makes the whole row of y NaN, and with it every score of the row
        if (!isfinite(acc0)) acc0 = __builtin_nanf("");
        if (!isfinite(acc1)) acc1 = __builtin_nanf("");
    }
    if (n0 + c < N) {
        if (m0 + 2 * g < M) Cm[(size_t)(m0 + 2 * g) * ldc + n0 + c] = acc0 * scale;
        if (m0 + 2 * g + 1 < M) Cm[(size_t)(m0 + 2 * g + 1) * ldc + n0 + c] = acc1 * scale;
    }
}

// ---------------------------------------------------------------- class distances
// torch.max's rule on (value, index) pairs: NaN is the greatest value, and among equal values the lowest index wins.
__device__ __forceinline__ bool maha_better(float a, int ai, float b, int bi) {
    const bool an = a != a, bn = b != b;
    if (an || bn) return an && (!bn || ai < bi);
    return a > b || (a == b && ai < bi);
}

// One workgroup = (16 * T) samples x (16 * T) classes, each thread a T x T register tile of (b, c) pairs over r, R in chunks of 64 through LDS.
// Writes score[b, c] to `all` (optional) and, per row and class tile, the tile's best (value, class) to part_v / part_i [B, ntiles].
// T = 2: 32 x 32 tiles; T = 1: 16 x 16, chosen when the larger tile would leave most of the chip without a workgroup (B = 32: 58 -> 232).
#define MD_R 64
template <int T>
__global__ __launch_bounds__(256) void maha_dist_kernel(const float* __restrict__ y, const float* __restrict__ nu, int B, int R, int NC, float* __restrict__ all, int ld_all,
                                                        float* __restrict__ part_v, int* __restrict__ part_i, int ntiles) {
    constexpr int TILE = 16 * T;
    __shared__ float ys[TILE][MD_R + 1];
    __shared__ float ns[TILE][MD_R + 1];
    __shared__ float rv[TILE][16];
    __shared__ int ri[TILE][16];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int c0 = blockIdx.x * TILE, b0 = blockIdx.y * TILE;
    float acc[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) acc[i][j] = 0.f;
    const int lr = t & 63, lrow = t >> 6;           // loads: 4 tile rows per pass, 64 consecutive r
    for (int r0 = 0; r0 < R; r0 += MD_R) {
#pragma unroll
        for (int i = 0; i < TILE / 4; ++i) {
            const int row = lrow + 4 * i;
            const bool rok = r0 + lr < R;
            ys[row][lr] = (rok && b0 + row < B) ? y[(size_t)(b0 + row) * R + r0 + lr] : 0.f;
            ns[row][lr] = (rok && c0 + row < NC) ? nu[(size_t)(c0 + row) * R + r0 + lr] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int r = 0; r < MD_R; ++r) {
            float yv[T], nv[T];
#pragma unroll
            for (int i = 0; i < T; ++i) { yv[i] = ys[ty + 16 * i][r]; nv[i] = ns[tx + 16 * i][r]; }
#pragma unroll
            for (int i = 0; i < T; ++i)
#pragma unroll
                for (int j = 0; j < T; ++j) { const float d = yv[i] - nv[j]; acc[i][j] = fmaf(d, d, acc[i][j]); }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < T; ++i) {
        const int b = b0 + ty + 16 * i;
        float bv = 0.f; int bi = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < T; ++j) {                  // ascending class index
            const int c = c0 + tx + 16 * j;
            // NaN where y is NaN (a non-finite pooled value: maha_gemm_kernel), as the reference's mm() products give; a squared distance that
            // overflows f32 scores -inf for that class alone, as the reference's does
            const float s = -0.5f * acc[i][j];
            if (c < NC) {
                if (all != nullptr && b < B) all[(size_t)b * ld_all + c] = s;
                if (bi == 0x7fffffff || maha_better(s, c, bv, bi)) { bv = s; bi = c; }
            }
        }
        rv[ty + 16 * i][tx] = bv; ri[ty + 16 * i][tx] = bi;
    }
    __syncthreads();
    if (t < TILE && b0 + t < B) {
        float bv = rv[t][0]; int bi = ri[t][0];         // tx = 0 always owns class c0 < NC
        for (int k = 1; k < 16; ++k)
            if (ri[t][k] != 0x7fffffff && maha_better(rv[t][k], ri[t][k], bv, bi)) { bv = rv[t][k]; bi = ri[t][k]; }
        part_v[(size_t)(b0 + t) * ntiles + blockIdx.x] = bv;
        part_i[(size_t)(b0 + t) * ntiles + blockIdx.x] = bi;
    }
}

// one wave per row folds the class tiles' winners: score, label = max / argmax over all classes
__global__ __launch_bounds__(256) void maha_fold_kernel(const float* __restrict__ part_v, const int* __restrict__ part_i, int B, int ntiles, float* __restrict__ score,
                                                        int64_t* __restrict__ label) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;                               // wave-uniform
    float bv = 0.f; int bi = 0x7fffffff;
    for (int k = lane; k < ntiles; k += 64) {
        const float v = part_v[(size_t)row * ntiles + k];
        const int i = part_i[(size_t)row * ntiles + k];
        if (bi == 0x7fffffff || maha_better(v, i, bv, bi)) { bv = v; bi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (oi != 0x7fffffff && (bi == 0x7fffffff || maha_better(ov, oi, bv, bi))) { bv = ov; bi = oi; }
    }
    if (lane == 0) {
        if (score) score[row] = bv;
        if (label) label[row] = bi;
    }
}

static int maha_dist_variant(int B, int NC) { return (long)cdiv(B, 32) * cdiv(NC, 32) < 256 ? 1 : 2; }

static size_t maha_score_scratch(int B, int NC) { return (size_t)B * cdiv(NC, 16) * (sizeof(float) + sizeof(int)); }

// ---------------------------------------------------------------- estimator: accumulate one batch into the f64 state
// state = n [NC] | sums [NC, H] | G [H, H] doubles.  Every destination is owned by one thread, which adds the batch's rows in ascending b to the
// value it found: two batches in sequence give the bits of the concatenated batch.
__global__ __launch_bounds__(256) void maha_rowcount_kernel(const float* __restrict__ target, int ldt, int B, int NC, int* __restrict__ kb) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;
    int n = 0;
    for (int c = lane; c < NC; c += 64) n += target[(size_t)row * ldt + c] != 0.f ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);      // integers: exact in any order
    if (lane == 0) kb[row] = n;
}

// one workgroup per class: membership flags of a chunk of 256 samples in LDS, then every thread walks them for its columns of the class sum
__global__ __launch_bounds__(256) void maha_class_sums_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ target, int ldt, int B, int H, int NC,
                                                              double* __restrict__ cnt, double* __restrict__ sums) {
    __shared__ int flag[256];
    const int c = blockIdx.x, t = threadIdx.x;
    constexpr int MAXH = 8;                             // columns per thread: H <= 2048
    double s[MAXH];
#pragma unroll
    for (int i = 0; i < MAXH; ++i) { const int h = t + 256 * i; s[i] = h < H ? sums[(size_t)c * H + h] : 0.0; }
    int n = 0;
    for (int b0 = 0; b0 < B; b0 += 256) {
        flag[t] = (b0 + t < B && target[(size_t)(b0 + t) * ldt + c] != 0.f) ? 1 : 0;
        __syncthreads();
        const int nb = min(256, B - b0);
        for (int b = 0; b < nb; ++b) {
            if (!flag[b]) continue;                     // uniform over the workgroup
            ++n;
#pragma unroll
            for (int i = 0; i < MAXH; ++i) { const int h = t + 256 * i; if (h < H) s[i] += (double)x[(size_t)(b0 + b) * ldx + h]; }
        }
        __syncthreads();
    }
    if (n == 0) return;
#pragma unroll
    for (int i = 0; i < MAXH; ++i) { const int h = t + 256 * i; if (h < H) sums[(size_t)c * H + h] = s[i]; }
    if (t == 0) cnt[c] += (double)n;
}

// G[i, j] += sum_b k_b x[b, i] x[b, j]: 64 x 64 tile per workgroup, 4 x 4 per thread, 16 samples per LDS chunk.  The product of two f32 values is exact
// in f64, so G comes out exactly symmetric.
__global__ __launch_bounds__(256) void maha_gram_kernel(const float* __restrict__ x, int ldx, const int* __restrict__ kb, int B, int H, double* __restrict__ G) {
    __shared__ float xi[16][64], xj[16][64];
    __shared__ double ks[16];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int j0 = blockIdx.x * 64, i0 = blockIdx.y * 64;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
            acc[a][b] = (i < H && j < H) ? G[(size_t)i * H + j] : 0.0;
        }
    const int lc = t & 63, lrow = t >> 6;
    for (int b0 = 0; b0 < B; b0 += 16) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int r = lrow + 4 * p;
            const bool ok = b0 + r < B;
            xi[r][lc] = (ok && i0 + lc < H) ? x[(size_t)(b0 + r) * ldx + i0 + lc] : 0.f;
            xj[r][lc] = (ok && j0 + lc < H) ? x[(size_t)(b0 + r) * ldx + j0 + lc] : 0.f;
        }
        if (t < 16) ks[t] = b0 + t < B ? (double)kb[b0 + t] : 0.0;
        __syncthreads();
        const int nb = min(16, B - b0);
        for (int r = 0; r < nb; ++r) {
            const double k = ks[r];
            if (k == 0.0) continue;                     // a sample in no class (uniform over the workgroup): adds nothing
            double vi[4], vj[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) { vi[a] = (double)xi[r][ty + 16 * a]; vj[a] = (double)xj[r][tx + 16 * a]; }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = fma(k, vi[a] * vj[b], acc[a][b]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
            if (i < H && j < H) G[(size_t)i * H + j] = acc[a][b];
        }
}

// ---------------------------------------------------------------- C ABI
#define S(x) reinterpret_cast<hipStream_t>(x)
extern "C" {

int rgqa_maha_scratch_bytes(int B, int NC, size_t* out) {
    RGQA_REQUIRE(out != nullptr && B > 0 && NC > 0, "maha_scratch_bytes: bad argument");
    const size_t a = maha_score_scratch(B, NC), b = (size_t)B * sizeof(int);
    *out = a > b ? a : b;
    return RGQA_OK;
}

int rgqa_maha_score_rows(const float* pooled, int ld, const float* W, const float* nu, int B, int H, int R, int NC, float* y, float* score, int64_t* label,
                         float* all_scores, int ld_all, void* scratch, size_t scratch_bytes, void* stream) {
    RGQA_REQUIRE(pooled != nullptr && W != nullptr && nu != nullptr && y != nullptr && scratch != nullptr, "maha_score_rows: null argument");
    RGQA_REQUIRE(B > 0 && H > 0 && R > 0 && NC > 0 && ld >= H, "maha_score_rows: bad shape B=%d H=%d R=%d NC=%d ld=%d", B, H, R, NC, ld);
    RGQA_REQUIRE(all_scores == nullptr || ld_all >= NC, "maha_score_rows: ld_all=%d < NC=%d", ld_all, NC);
    RGQA_REQUIRE(scratch_bytes >= maha_score_scratch(B, NC), "maha_score_rows: scratch of %zu bytes, %zu needed", scratch_bytes, maha_score_scratch(B, NC));
    hipStream_t s = S(stream);
    hipLaunchKernelGGL((maha_gemm_kernel<0, 0>), dim3(cdiv(R, MG_COLS), cdiv(B, MG_ROWS)), dim3(256), 0, s, pooled, ld, W, R, (const float*)nullptr, (const int64_t*)nullptr, 0,
                       1.0f, B, R, H, y, R);
    RGQA_LAUNCH_CHECK("maha_gemm_kernel<0, 0>");
    const int T = maha_dist_variant(B, NC);
    const int ntiles = cdiv(NC, 16 * T);
    float* pv = reinterpret_cast<float*>(scratch);
    int* pi = reinterpret_cast<int*>(pv + (size_t)B * ntiles);
    if (T == 1) hipLaunchKernelGGL(maha_dist_kernel<1>, dim3(ntiles, cdiv(B, 16)), dim3(256), 0, s, y, nu, B, R, NC, all_scores, ld_all, pv, pi, ntiles);
    else hipLaunchKernelGGL(maha_dist_kernel<2>, dim3(ntiles, cdiv(B, 32)), dim3(256), 0, s, y, nu, B, R, NC, all_scores, ld_all, pv, pi, ntiles);
    RGQA_LAUNCH_CHECK("maha_dist_kernel");
    hipLaunchKernelGGL(maha_fold_kernel, dim3(cdiv(B, 4)), dim3(256), 0, s, pv, pi, B, ntiles, score, label);
    RGQA_LAUNCH_CHECK("maha_fold_kernel");
    return RGQA_OK;
}

int rgqa_maha_dpooled(const float* pooled, int ld, const float* mean, const int64_t* label, const float* W, float scale, int B, int H, int R, int NC, float* d,
                      float* dpooled, int ldd, void* stream) {
    RGQA_REQUIRE(pooled != nullptr && mean != nullptr && label != nullptr && W != nullptr && d != nullptr && dpooled != nullptr, "maha_dpooled: null argument");
    RGQA_REQUIRE(B > 0 && H > 0 && R > 0 && NC > 0 && ld >= H && ldd >= H, "maha_dpooled: bad shape B=%d H=%d R=%d NC=%d ld=%d ldd=%d", B, H, R, NC, ld, ldd);
    hipStream_t s = S(stream);
    hipLaunchKernelGGL((maha_gemm_kernel<0, 1>), dim3(cdiv(R, MG_COLS), cdiv(B, MG_ROWS)), dim3(256), 0, s, pooled, ld, W, R, mean, label, NC, 1.0f, B, R, H, d, R);
    RGQA_LAUNCH_CHECK("maha_gemm_kernel<0, 1>");
    hipLaunchKernelGGL((maha_gemm_kernel<1, 0>), dim3(cdiv(H, MG_COLS), cdiv(B, MG_ROWS)), dim3(256), 0, s, d, R, W, R, (const float*)nullptr, (const int64_t*)nullptr, 0, scale,
                       B, H, R, dpooled, ldd);
    RGQA_LAUNCH_CHECK("maha_gemm_kernel<1, 0>");
    return RGQA_OK;
}

int rgqa_maha_state_doubles(int NC, int H, size_t* out) {
    RGQA_REQUIRE(out != nullptr && NC > 0 && H > 0, "maha_state_doubles: bad argument");
    *out = (size_t)NC + (size_t)NC * H + (size_t)H * H;
    return RGQA_OK;
}

int rgqa_maha_accumulate(const float* pooled, int ld, const float* target, int ld_target, int B, int H, int NC, double* state, void* scratch, size_t scratch_bytes,
                         void* stream) {
    RGQA_REQUIRE(pooled != nullptr && target != nullptr && state != nullptr && scratch != nullptr, "maha_accumulate: null argument");
    RGQA_REQUIRE(B > 0 && H > 0 && H <= 2048 && NC > 0 && ld >= H && ld_target >= NC, "maha_accumulate: bad shape B=%d H=%d (<= 2048) NC=%d ld=%d ld_target=%d", B, H, NC, ld,
                 ld_target);
    RGQA_REQUIRE(scratch_bytes >= (size_t)B * sizeof(int), "maha_accumulate: scratch of %zu bytes, %zu needed", scratch_bytes, (size_t)B * sizeof(int));
    hipStream_t s = S(stream);
    int* kb = reinterpret_cast<int*>(scratch);
    double* cnt = state;
    double* sums = state + NC;
    double* G = sums + (size_t)NC * H;
    hipLaunchKernelGGL(maha_rowcount_kernel, dim3(cdiv(B, 4)), dim3(256), 0, s, target, ld_target, B, NC, kb);
    RGQA_LAUNCH_CHECK("maha_rowcount_kernel");
    hipLaunchKernelGGL(maha_class_sums_kernel, dim3(NC), dim3(256), 0, s, pooled, ld, target, ld_target, B, H, NC, cnt, sums);
    RGQA_LAUNCH_CHECK("maha_class_sums_kernel");
    hipLaunchKernelGGL(maha_gram_kernel, dim3(cdiv(H, 64), cdiv(H, 64)), dim3(256), 0, s, pooled, ld, kb, B, H, G);
    RGQA_LAUNCH_CHECK("maha_gram_kernel");
    return RGQA_OK;
}

}  // extern "C"
