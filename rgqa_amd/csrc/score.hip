// Test-time scoring of answer logits: what every RVQA test script of the reference computes on the
// [B, num_answers] logits, fused into one pass over each row.
//   max_score, label = torch.sigmoid(logit / temperature).max(1)     tasks/gqa_conf.py:344, gqa_energy.py:184,204; gqa_odin.py:130-131
//   energy           = torch.log(1 + torch.exp(logit)).sum(1)        tasks/gqa_energy.py:135,185
//   topk             = logit.topk(k)                                 tasks/gqa_energy.py:205, gqa_check_topk_preds.py:189
//   topk_energy      = torch.log(1 + torch.exp(topk.values)).sum(1)  tasks/gqa_energy.py:206
// One wave per row (1842 answers = 29 elements per lane), HBM-bound: 4 B per logit read once (the k selection passes re-read
// the 7-KiB row from L1/L2).  Formulas are kept as the reference writes them (the naive softplus overflows to +inf above
// logit 88.7 exactly as torch's does); the max runs over the SIGMOID values, so saturated ties resolve to the first index
// as on the reference's CPU path.
#include "kernels.h"

__global__ __launch_bounds__(256) void score_rows_kernel(const float* __restrict__ logits, int ld, int B, int NA, float temperature, int k,
                                                         float* __restrict__ max_score, int64_t* __restrict__ label, float* __restrict__ energy,
                                                         float* __restrict__ topk_val, int64_t* __restrict__ topk_idx, float* __restrict__ topk_energy) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;                               // wave-uniform
    const float* x = logits + (size_t)row * ld;
    float e = 0.f, best = -1.0f;                        // sigmoid values are >= 0
    int besti = 0x7fffffff;
    for (int j = lane; j < NA; j += 64) {
        const float v = x[j];
        e += softplus_naive(v);
        const float sg = 1.0f / (1.0f + expf(-(v / temperature)));
        if (sg > best) { best = sg; besti = j; }         // ascending j per lane: the first maximum stays
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        e += __shfl_xor(e, o);
        const float ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(besti, o);
        if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
    }
    if (lane == 0) {
        if (energy) energy[row] = e;
        if (max_score) max_score[row] = best;
        if (label) label[row] = besti;
    }
    if (k <= 0) return;
    // top-k of the raw logits, descending, ties by ascending index: k selection passes in (value desc, index asc) order
    float last_v = INFINITY, te = 0.f;
    int last_i = -1;
    for (int r = 0; r < k; ++r) {
        float bv = -INFINITY; int bi = 0x7fffffff;
        for (int j = lane; j < NA; j += 64) {
            const float v = x[j];
            const bool after = v < last_v || (v == last_v && j > last_i);      // not selected yet
            if (after && (v > bv || (v == bv && j < bi))) { bv = v; bi = j; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
        }
        last_v = bv; last_i = bi;
        te += softplus_naive(bv);
        if (lane == 0) {
            if (topk_val) topk_val[(size_t)row * k + r] = bv;
            if (topk_idx) topk_idx[(size_t)row * k + r] = bi;
        }
    }
    if (lane == 0 && topk_energy) topk_energy[row] = te;
}

int k_score_rows(const float* logits, int ld, int B, int NA, float temperature, int k, float* max_score, int64_t* label, float* energy,
                 float* topk_val, int64_t* topk_idx, float* topk_energy, hipStream_t s) {
    RGQA_REQUIRE(logits != nullptr && B > 0 && NA > 0 && ld >= NA, "score_rows: bad shape B=%d NA=%d ld=%d", B, NA, ld);
    RGQA_REQUIRE(k >= 0 && k <= NA, "score_rows: k=%d outside [0, %d]", k, NA);
    RGQA_REQUIRE(temperature > 0.f, "score_rows: temperature must be positive");
    hipLaunchKernelGGL(score_rows_kernel, dim3(cdiv(B, 4)), dim3(256), 0, s, logits, ld, B, NA, temperature, k, max_score, label, energy, topk_val, topk_idx, topk_energy);
    RGQA_LAUNCH_CHECK("score_rows_kernel");
    return RGQA_OK;
}

// ---------------------------------------------------------------- ODIN's two extra steps (tasks/gqa_odin.py:101-121)
// The loss of the reference's scorer is the mean over rows of BCEWithLogits(logit[b, idx[b]], labels[b, idx[b]]) with idx = argmax of
// sigmoid(logit / T) and labels = (sigmoid(logit / T) >= 0.5): one column per row.  idx and the value the target is taken from come from
// score_rows_kernel for the same logits and temperature (label, max_score), so the "first maximum of the f32 sigmoid values" rule lives there
// alone; the target is max_score >= 0.5 - NOT logit >= 0: at T = 1e5 the f32 sigmoid of a small negative logit is exactly 0.5.
// One workgroup per row writes the row of dlogits: (sigmoid(z) - y) / B at the chosen column (the un-tempered logit, as bceloss(logit, labels)
// is), exact zeros elsewhere up to column NAp.  Workgroup 0 also folds the loss over the rows in a fixed order.
// (not rowops.h's bce_term: that one takes __expf, this one expf - the two give different bits)
__device__ __forceinline__ float bce_logit(float z, float y) { return fmaxf(z, 0.f) - z * y + log1pf(expf(-fabsf(z))); }

__global__ __launch_bounds__(256) void odin_dlogits_kernel(const float* __restrict__ logits, int ld, const int64_t* __restrict__ label, const float* __restrict__ max_score,
                                                           int B, int NA, int NAp, float* __restrict__ dlogits, int ldd, float* __restrict__ loss) {
    const int row = blockIdx.x;
    const int64_t col = label[row];
    float* d = dlogits + (size_t)row * ldd;
    float chosen = 0.f;
    if (col >= 0 && col < NA) {
        const float z = logits[(size_t)row * ld + col], y = max_score[row] >= 0.5f ? 1.0f : 0.0f;
        chosen = (1.0f / (1.0f + expf(-z)) - y) / (float)B;
    }
    for (int j = threadIdx.x; j < NAp; j += 256) d[j] = (j == col) ? chosen : 0.f;
    if (row != 0 || loss == nullptr) return;
    __shared__ float red[4];
    float acc = 0.f;
    for (int r = threadIdx.x; r < B; r += 256) {
        const int64_t c = label[r];
        if (c >= 0 && c < NA) acc += bce_logit(logits[(size_t)r * ld + c], max_score[r] >= 0.5f ? 1.0f : 0.0f);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = (red[0] + red[1] + red[2] + red[3]) / (float)B;
}
int k_odin_dlogits(const float* logits, int ld, const int64_t* label, const float* max_score, int B, int NA, int NAp, float* dlogits, int ldd, float* loss, hipStream_t s) {
    RGQA_REQUIRE(logits != nullptr && label != nullptr && max_score != nullptr && dlogits != nullptr, "odin_dlogits: null argument");
    RGQA_REQUIRE(B > 0 && NA > 0 && ld >= NA && NAp >= NA && ldd >= NAp, "odin_dlogits: bad shape B=%d NA=%d NAp=%d ld=%d ldd=%d", B, NA, NAp, ld, ldd);
    hipLaunchKernelGGL(odin_dlogits_kernel, dim3(B), dim3(256), 0, s, logits, ld, label, max_score, B, NA, NAp, dlogits, ldd, loss);
    RGQA_LAUNCH_CHECK("odin_dlogits_kernel");
    return RGQA_OK;
}

// out = x - noise * (grad >= 0 ? 1 : -1)   (gqa_odin.py:115-121: torch.ge, so 0 and -0.0 step by -noise and NaN by +noise); out may alias x
__device__ __forceinline__ float sign_step1(float x, float g, float noise) { return x + (g >= 0.f ? -noise : noise); }
__global__ __launch_bounds__(256) void sign_step_kernel(const float* x, const float* __restrict__ grad, float noise, float* out, size_t n, int vec) {
    const size_t stride = (size_t)gridDim.x * 256, t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t n4 = vec ? n >> 2 : 0;
    for (size_t i = t; i < n4; i += stride) {
        const float4 a = reinterpret_cast<const float4*>(x)[i], g = reinterpret_cast<const float4*>(grad)[i];
        reinterpret_cast<float4*>(out)[i] = make_float4(sign_step1(a.x, g.x, noise), sign_step1(a.y, g.y, noise), sign_step1(a.z, g.z, noise), sign_step1(a.w, g.w, noise));
    }
    for (size_t i = (n4 << 2) + t; i < n; i += stride) out[i] = sign_step1(x[i], grad[i], noise);
}
int k_sign_step(const float* x, const float* grad, float noise, float* out, size_t n, hipStream_t s) {
    RGQA_REQUIRE(x != nullptr && grad != nullptr && out != nullptr, "sign_step: null argument");
    if (n == 0) return RGQA_OK;
    const int vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const size_t work = vec ? (n + 3) / 4 : n;
    const size_t blocks = (work + 255) / 256;
    hipLaunchKernelGGL(sign_step_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, s, x, grad, noise, out, n, vec);
    RGQA_LAUNCH_CHECK("sign_step_kernel");
    return RGQA_OK;
}
