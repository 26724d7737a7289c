// The tail of the confidence branch (reference tasks/gqa_model_branched.py:28-33, conf_fc = Linear(H, 2H) -> GeLU -> LayerNorm(2H) -> Linear(2H, 1)) behind
// the conf_fc.0 GEMM, whose GELU epilogue leaves x = gelu(pre) and gelu'(pre):
//   forward   conf_logit_b = sum_j LN(x_b)_j w3_j + b3                      one workgroup per row; LayerNorm statistics, the normalised row and the dot in f32
//   backward  d x_b = LN-backward(dconf_b w3) ; gc_b = d x_b gelu'(pre_b)    one workgroup per row -> the gradient entering conf_fc.0's output
//             dgamma_j = sum_b dconf_b w3_j xhat_bj, dbeta_j = sum_b dconf_b w3_j, dw3_j = sum_b dconf_b LN(x_b)_j, db3 = sum_b dconf_b
// The normalised row is not stored: an N = 1 GEMM would read it once, and so does the dot here; the backward re-forms it from x, mean and rstd.
// Column sums: a workgroup owns 64 columns, its four waves take the rows b = w, w + 4, ... in ascending order and their partials are added as
// (p0 + p1) + (p2 + p3): a fixed order, no float atomics - results repeat bit for bit.
// Hidden sizes up to 1024 (engine_create's limit): rows of N = 2H <= 2048 elements, 8 per thread.
#include "kernels.h"

#define CH_T 256
#define CH_MAXE 8

// sum over the workgroup, every thread gets it; the same order whatever the caller (wave butterflies, then (s0 + s1) + (s2 + s3))
__device__ __forceinline__ float ch_block_sum(float v, float* sh) {
    v = wave_sum(v);
    __syncthreads();                 // sh may still be read from the previous call
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

template <typename T>
__global__ __launch_bounds__(CH_T) void conf_tail_fwd_kernel(const T* __restrict__ x, int ld, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ w3, const float* __restrict__ b3, float* __restrict__ conf,
                                                             float* __restrict__ mean, float* __restrict__ rstd, int N, float eps) {
    __shared__ float sh[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const T* row = x + (size_t)b * ld;
    float v[CH_MAXE];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < CH_MAXE; ++i) {
        const int j = tid + CH_T * i;
        v[i] = j < N ? ld_elem(row + j) : 0.f;
        s += v[i];
    }
    const float mu = ch_block_sum(s, sh) / (float)N;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < CH_MAXE; ++i) {
        const int j = tid + CH_T * i;
        const float d = j < N ? v[i] - mu : 0.f;
        q += d * d;
    }
    const float rs = rsqrtf(ch_block_sum(q, sh) / (float)N + eps);
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < CH_MAXE; ++i) {
        const int j = tid + CH_T * i;
        if (j < N) dot += ((v[i] - mu) * rs * gamma[j] + beta[j]) * w3[j];
    }
    dot = ch_block_sum(dot, sh);
    if (tid == 0) { conf[b] = dot + b3[0]; mean[b] = mu; rstd[b] = rs; }
}

template <typename T>
__global__ __launch_bounds__(CH_T) void conf_tail_bwd_kernel(const float* __restrict__ dconf, const T* __restrict__ x, const T* __restrict__ dgelu, int ld,
                                                             const float* __restrict__ gamma, const float* __restrict__ w3, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, T* __restrict__ gc, int ldg, int N) {
    __shared__ float sh[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const T* row = x + (size_t)b * ld;
    const float dc = dconf[b], mu = mean[b], rs = rstd[b];
    float g[CH_MAXE], xh[CH_MAXE];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < CH_MAXE; ++i) {
        const int j = tid + CH_T * i;
        g[i] = 0.f; xh[i] = 0.f;
        if (j < N) { xh[i] = (ld_elem(row + j) - mu) * rs; g[i] = dc * w3[j] * gamma[j]; }
        s1 += g[i]; s2 += g[i] * xh[i];
    }
    const float m1 = ch_block_sum(s1, sh) / (float)N;
    const float m2 = ch_block_sum(s2, sh) / (float)N;
#pragma unroll
    for (int i = 0; i < CH_MAXE; ++i) {
        const int j = tid + CH_T * i;
        if (j < N) st_elem(gc + (size_t)b * ldg + j, rs * (g[i] - m1 - xh[i] * m2) * ld_elem(dgelu + (size_t)b * ld + j));
    }
}

template <typename T>
__global__ __launch_bounds__(CH_T) void conf_tail_colsum_kernel(const float* __restrict__ dconf, const T* __restrict__ x, int ld, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, const float* __restrict__ w3, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                float* __restrict__ dw3, float* __restrict__ db3, int accumulate, int B, int N) {
    __shared__ float sh[3][4][64];
    __shared__ float sb[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j = blockIdx.x * 64 + lane;
    float ag = 0.f, ab = 0.f, aw = 0.f;
    if (j < N) {
        const float wj = w3[j], gj = gamma[j], bj = beta[j];
        for (int b = w; b < B; b += 4) {
            const float dc = dconf[b];
            const float xh = (ld_elem(x + (size_t)b * ld + j) - mean[b]) * rstd[b];
            ag += dc * wj * xh; ab += dc * wj; aw += dc * (xh * gj + bj);
        }
    }
    sh[0][w][lane] = ag; sh[1][w][lane] = ab; sh[2][w][lane] = aw;
    __syncthreads();
    if (w == 0 && j < N) {
        const float vg = (sh[0][0][lane] + sh[0][1][lane]) + (sh[0][2][lane] + sh[0][3][lane]);
        const float vb = (sh[1][0][lane] + sh[1][1][lane]) + (sh[1][2][lane] + sh[1][3][lane]);
        const float vw = (sh[2][0][lane] + sh[2][1][lane]) + (sh[2][2][lane] + sh[2][3][lane]);
        dgamma[j] = accumulate ? dgamma[j] + vg : vg;
        dbeta[j] = accumulate ? dbeta[j] + vb : vb;
        dw3[j] = accumulate ? dw3[j] + vw : vw;
    }
    if (blockIdx.x == 0) {           // db3 = sum_b dconf_b
        float a = 0.f;
        for (int b = tid; b < B; b += CH_T) a += dconf[b];
        a = ch_block_sum(a, sb);
        if (tid == 0) db3[0] = accumulate ? db3[0] + a : a;
    }
}

template <typename T>
__global__ void add_inplace_kernel(T* __restrict__ a, const T* __restrict__ b, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        st_elem(a + i, ld_elem(a + i) + ld_elem(b + i));
}

template <typename T>
int k_conf_tail_fwd(const T* x, int ld, const float* gamma, const float* beta, const float* w3, const float* b3, float* conf, float* mean, float* rstd, int B, int N,
                    float eps, hipStream_t s) {
    RGQA_REQUIRE(x && gamma && beta && w3 && b3 && conf && mean && rstd, "conf_tail_fwd: null argument");
    RGQA_REQUIRE(B > 0 && N > 0 && N <= CH_T * CH_MAXE && ld >= N, "conf_tail_fwd: bad shape B=%d N=%d ld=%d (N <= %d)", B, N, ld, CH_T * CH_MAXE);
    hipLaunchKernelGGL(conf_tail_fwd_kernel<T>, dim3(B), dim3(CH_T), 0, s, x, ld, gamma, beta, w3, b3, conf, mean, rstd, N, eps);
    RGQA_LAUNCH_CHECK("conf_tail_fwd_kernel");
    return RGQA_OK;
}

template <typename T>
int k_conf_tail_bwd(const float* dconf, const T* x, const T* dgelu, int ld, const float* gamma, const float* beta, const float* w3, const float* mean, const float* rstd,
                    T* gc, int ldg, float* dgamma, float* dbeta, float* dw3, float* db3, int accumulate, int B, int N, hipStream_t s) {
    RGQA_REQUIRE(dconf && x && dgelu && gamma && beta && w3 && mean && rstd && gc && dgamma && dbeta && dw3 && db3, "conf_tail_bwd: null argument");
    RGQA_REQUIRE(B > 0 && N > 0 && N <= CH_T * CH_MAXE && ld >= N && ldg >= N, "conf_tail_bwd: bad shape B=%d N=%d ld=%d ldg=%d (N <= %d)", B, N, ld, ldg, CH_T * CH_MAXE);
    hipLaunchKernelGGL(conf_tail_bwd_kernel<T>, dim3(B), dim3(CH_T), 0, s, dconf, x, dgelu, ld, gamma, w3, mean, rstd, gc, ldg, N);
    RGQA_LAUNCH_CHECK("conf_tail_bwd_kernel");
    hipLaunchKernelGGL(conf_tail_colsum_kernel<T>, dim3(cdiv(N, 64)), dim3(CH_T), 0, s, dconf, x, ld, gamma, beta, w3, mean, rstd, dgamma, dbeta, dw3, db3, accumulate, B, N);
    RGQA_LAUNCH_CHECK("conf_tail_colsum_kernel");
    return RGQA_OK;
}

template <typename T>
int k_add_inplace(T* a, const T* b, size_t n, hipStream_t s) {
    if (n == 0) return RGQA_OK;
    int nb = (int)((n + 255) / 256); if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(add_inplace_kernel<T>, dim3(nb), dim3(256), 0, s, a, b, n);
    RGQA_LAUNCH_CHECK("add_inplace_kernel");
    return RGQA_OK;
}

#define CH_INST(T)                                                                                                                                              \
    template int k_conf_tail_fwd<T>(const T*, int, const float*, const float*, const float*, const float*, float*, float*, float*, int, int, float, hipStream_t); \
    template int k_conf_tail_bwd<T>(const float*, const T*, const T*, int, const float*, const float*, const float*, const float*, const float*, T*, int, float*,  \
                                    float*, float*, float*, int, int, int, hipStream_t);                                                                        \
    template int k_add_inplace<T>(T*, const T*, size_t, hipStream_t);
CH_INST(float)
CH_INST(bf16_t)
CH_INST(sf32)
