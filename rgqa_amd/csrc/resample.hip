// The step of the reference's soft resampling of the hard unanswerable questions (tasks/gqa_resampling.py:176-220, lxmert / uniter order), fused.
// theta [N] are the learnable weight parameters (one per negative training question, N ~ 1e5 - 1e6), wid[b] the parameter of negative row b:
//   w = softplus(theta);  weights_b = (mean(sqrt w) / sqrt(mean w)) * sqrt(w[wid_b] / mean w) = (mh / m1) sqrt(w[wid_b])                    :184-186
//   loss_pos = (1 / Bp) sum_b r_b,  loss_neg = (1 / Bn) sum_b weights_b r_b,  r_b = sum_c BCEWithLogits(z[b, c], t[b, c])                   :196-200
//   loss = loss_pos + loss_neg (the model's),  loss_w = -loss_neg (theta's: optim_w.zero_grad() at :218 discards what loss.backward() left)  :202-203, :214-220
//   dlogits = (sigmoid(z) - t) c_b,  c_b = 1 / Bp (positive rows), weights_b / Bn (negative rows)
// and, with S = sum_b r_b sqrt(w[wid_b]) and s_j = sum over {b: wid_b = j} of r_b,
//   d loss_w / d w_j = -(1 / Bn) [ S / (2 N m1 sqrt w_j) - mh S / (N m1^2) + (mh / (2 m1)) s_j / sqrt w_j ]
//   g_j = d loss_w / d w_j * sigmoid(theta_j);   buf <- momentum buf + g;   theta <- theta - lr_w buf                                       (torch SGD, :140)
// The gradient is dense: every theta_j moves every step through m1 and mh.
//
// Three calls.  k_resample_weights: the two means over N in f64 - per-thread and per-workgroup partials, folded in a fixed order by one workgroup,
// which also gathers the Bn batch weights.  k_resample_loss: one workgroup per row, bce_kernel's element formulas (rowops.h), one sweep for the
// row's BCE sum (f64) and its dlogits; a one-workgroup launch folds the row shares.  k_resample_step: one workgroup names an OWNER for every index
// that occurs in wid - its first occurrence, which adds the row losses of all occurrences in batch order - and forms S and the three coefficients
// of the gradient in f64; the pass over N then gives every workgroup a contiguous 1024-index chunk, the owners inside the chunk drop their sum into an
// LDS image of it (one owner per index: no two writers, no atomics), and each thread updates one quad of theta and buf.
// No float atomics anywhere, every sum has a fixed order: results repeat bit for bit.  Thread -> element mappings are the same whether a quad moves by
// one 16-byte access or four 4-byte ones, so results do not depend on the operands' alignment; doubles travel through the float scratch as two words.
// An index outside [0, N) is skipped everywhere (its batch weight is 0).
#include "kernels.h"
#include <string.h>

#define RS_T 256
#define RS_CHUNK 1024            // indices per workgroup of the step pass: one quad per thread
#define RS_MAX_PARTS 1024        // workgroups of the sum pass: at most 4 partials per thread of the fold

__device__ __forceinline__ void rs_put_d(float* p, double v) { memcpy(p, &v, 8); }            // p is 4-byte aligned only: two word stores
__device__ __forceinline__ double rs_get_d(const float* p) { double v; memcpy(&v, p, 8); return v; }
// torch's softplus (beta 1, threshold 20)
__device__ __forceinline__ float rs_softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ double rs_softplus_d(double x) { return x > 20.0 ? x : log1p(exp(x)); }
__device__ __forceinline__ float rs_dsoftplus(float x) { return x > 20.f ? 1.f : 1.f / (1.f + expf(-x)); }

// ------------------------------------------------------------------------------------------------ weights
// parts[4 g .. 4 g + 3] = workgroup g's sums of w and sqrt(w) (two doubles as four words).  Thread (g, t) owns the quads 4 ((g + G i) 256 + t).
__global__ __launch_bounds__(RS_T) void resample_sum_kernel(const float* __restrict__ theta, int N, int vec, float* __restrict__ parts) {
    __shared__ double sh[4];
    const int tid = threadIdx.x;
    double s1 = 0.0, sh_ = 0.0;
    for (size_t q = (size_t)blockIdx.x * RS_T + tid; 4 * q < (size_t)N; q += (size_t)gridDim.x * RS_T) {
        float x[4];
        const int n = (int)(4 * q);
        row_load4(theta, n, N, vec, 0.f, x);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (n + j < N) {
                const double w = rs_softplus_d((double)x[j]);
                s1 += w; sh_ += sqrt(w);
            }
        }
    }
    s1 = block_sum_d(s1, sh);
    sh_ = block_sum_d(sh_, sh);
    if (tid == 0) { rs_put_d(parts + 4 * (size_t)blockIdx.x, s1); rs_put_d(parts + 4 * (size_t)blockIdx.x + 2, sh_); }
}

// stats = {m1, mh};  weights[b] = (float)(mh / m1) sqrtf(softplus(theta[wid[b]]))
__global__ __launch_bounds__(RS_T) void resample_weights_kernel(const float* __restrict__ parts, int G, const float* __restrict__ theta, int N, const int64_t* __restrict__ wid,
                                                                int Bn, double* __restrict__ stats, float* __restrict__ weights) {
    __shared__ double sh[4];
    const int tid = threadIdx.x;
    double s1 = 0.0, sh_ = 0.0;
    for (int g = tid; g < G; g += RS_T) { s1 += rs_get_d(parts + 4 * (size_t)g); sh_ += rs_get_d(parts + 4 * (size_t)g + 2); }
    s1 = block_sum_d(s1, sh);
    sh_ = block_sum_d(sh_, sh);
    const double m1 = s1 / (double)N, mh = sh_ / (double)N;
    if (tid == 0) { stats[0] = m1; stats[1] = mh; }
    const float scale = (float)(mh / m1);
    for (int b = tid; b < Bn; b += RS_T) {
        const int64_t j = wid[b];
        weights[b] = j >= 0 && j < (int64_t)N ? scale * sqrtf(rs_softplus(theta[j])) : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------ loss
struct ResampleLossArgs {
    const float* z; int ld;
    const float* t; int ldt;
    const float* weights;           // [B - n_pos]
    int B, n_pos, NA, NAp;
    float gscale;
    float* dz; int ldd;
    float* row_loss;                // [B - n_pos]
    float* rows;                    // [B][2]: the row's BCE sum, hi and lo  (null: no loss asked for)
    int vz, vt, vd;                 // 16-byte accesses allowed for z / t / dz
};

__global__ __launch_bounds__(RS_T) void resample_loss_kernel(ResampleLossArgs a) {
    __shared__ double sh[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const float* z = a.z + (size_t)b * a.ld;
    const float* t = a.t + (size_t)b * a.ldt;
    float* d = a.dz ? a.dz + (size_t)b * a.ldd : nullptr;
    const bool pos = b < a.n_pos;
    const float cb = pos ? 1.0f / (float)a.n_pos : a.weights[b - a.n_pos] * (1.0f / (float)(a.B - a.n_pos));
    double acc = 0.0;
    for (int n = 4 * tid; n < a.NAp; n += 4 * RS_T) {
        float x[4], y[4], g[4];
        row_load4(z, n, a.NA, a.vz, 0.f, x);
        row_load4(t, n, a.NA, a.vt, 0.f, y);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = 0.f;
            if (n + j < a.NA) {
                acc += (double)bce_term(x[j], y[j]);
                const float sg = bce_sigmoid(x[j]);
                v = (sg - y[j]) * cb * a.gscale;          // bce_kernel's (sg - y) * inv_b * gscale with c_b for inv_b
            }
            g[j] = v;
        }
        if (d) row_store4(d, n, a.NAp, a.vd, g);         // columns NA .. NAp: exact zeros (they feed K-padded GEMMs)
    }
    acc = block_sum_d(acc, sh);
    if (tid == 0) {
        if (!pos && a.row_loss) a.row_loss[b - a.n_pos] = (float)acc;
        if (a.rows) split_store(a.rows + 2 * (size_t)b, acc);
    }
}

// loss3 = {loss_pos + loss_neg, loss_pos, loss_neg}: the B row sums added in a fixed order, in f64
__global__ __launch_bounds__(RS_T) void resample_loss_fold_kernel(const float* __restrict__ rows, const float* __restrict__ weights, int B, int n_pos, float* __restrict__ loss3) {
    __shared__ double sh[4];
    const int tid = threadIdx.x;
    double sp = 0.0, sn = 0.0;
    for (int b = tid; b < B; b += RS_T) {
        const double r = (double)rows[2 * (size_t)b] + (double)rows[2 * (size_t)b + 1];
        if (b < n_pos) sp += r; else sn += (double)weights[b - n_pos] * r;
    }
    sp = block_sum_d(sp, sh);
    sn = block_sum_d(sn, sh);
    if (tid != 0) return;
    const double lp = sp / (double)n_pos, ln = sn / (double)(B - n_pos);
    loss3[0] = (float)(lp + ln); loss3[1] = (float)lp; loss3[2] = (float)ln;
}

// ------------------------------------------------------------------------------------------------ step
// scr: [0..2] the coefficients A, Bc, Cc of g_w = A / sqrt w + Bc + Cc s_j / sqrt w;  own_j [Bn] (int; -1: row b owns no index);  own_s [Bn]
__global__ __launch_bounds__(RS_T) void resample_owner_kernel(const float* __restrict__ theta, int N, const int64_t* __restrict__ wid, const float* __restrict__ row_loss, int Bn,
                                                              const double* __restrict__ stats, float* __restrict__ scr) {
    __shared__ double sh[4];
    const int tid = threadIdx.x;
    int* own_j = reinterpret_cast<int*>(scr + 4);
    float* own_s = scr + 4 + Bn;
    double term = 0.0;
    for (int b = tid; b < Bn; b += RS_T) {
        const int64_t j = wid[b];
        const bool valid = j >= 0 && j < (int64_t)N;
        bool first = valid;
        for (int c = 0; c < b && first; ++c) first = wid[c] != j;
        double s = 0.0;
        if (first) for (int c = b; c < Bn; ++c) if (wid[c] == j) s += (double)row_loss[c];         // batch order
        own_j[b] = first ? (int)j : -1;
        own_s[b] = (float)s;
        if (first) term += (double)(float)s * sqrt(rs_softplus_d((double)theta[j]));               // S from the owners' sums: [j, j, j] and [j] give the same S
    }
    const double S = block_sum_d(term, sh);
    if (tid != 0) return;
    const double m1 = stats[0], mh = stats[1], n = (double)N, bn = (double)Bn;
    scr[0] = (float)(-S / (2.0 * n * m1 * bn));
    scr[1] = (float)(mh * S / (n * m1 * m1 * bn));
    scr[2] = (float)(-mh / (2.0 * m1 * bn));
}

__global__ __launch_bounds__(RS_T) void resample_step_kernel(float* __restrict__ theta, float* __restrict__ buf, int N, int Bn, const float* __restrict__ scr, float lr, float momentum,
                                                             float* __restrict__ grad_out, int vth, int vbuf, int vg) {
    __shared__ float sl[RS_CHUNK];
    const int tid = threadIdx.x;
    const int64_t lo = (int64_t)blockIdx.x * RS_CHUNK;
    const int* own_j = reinterpret_cast<const int*>(scr + 4);
    const float* own_s = scr + 4 + Bn;
#pragma unroll
    for (int j = 0; j < 4; ++j) sl[4 * tid + j] = 0.f;
    __syncthreads();
    for (int b = tid; b < Bn; b += RS_T) {
        const int64_t r = (int64_t)own_j[b] - lo;
        if (own_j[b] >= 0 && r >= 0 && r < RS_CHUNK) sl[r] = own_s[b];              // one owner per index
    }
    __syncthreads();
    const float A = scr[0], Bc = scr[1], Cc = scr[2];
    if (lo + 4 * tid >= (int64_t)N) return;
    const int n = (int)lo + 4 * tid;
    float x[4], m[4], g[4];
    row_load4(theta, n, N, vth, 0.f, x);
    row_load4(buf, n, N, vbuf, 0.f, m);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float rs = 1.0f / sqrtf(rs_softplus(x[j]));
        g[j] = (fmaf(Cc * sl[4 * tid + j], rs, A * rs) + Bc) * rs_dsoftplus(x[j]);
        m[j] = fmaf(momentum, m[j], g[j]);
        x[j] = fmaf(-lr, m[j], x[j]);
    }
    row_store4(theta, n, N, vth, x);
    row_store4(buf, n, N, vbuf, m);
    if (grad_out) row_store4(grad_out, n, N, vg, g);
}

// ------------------------------------------------------------------------------------------------ host
static inline int rs_parts(int N) { const int g = (N + 4 * RS_T - 1) / (4 * RS_T); return g < 1 ? 1 : (g > RS_MAX_PARTS ? RS_MAX_PARTS : g); }

// what any of the three calls needs (they may share one buffer on one stream): the sum pass's partials | 2 floats per row | coefficients + owners
size_t k_resample_scratch_floats(int N, int B) {
    if (B <= 0) return 0;
    const size_t a = N > 0 ? 4 * (size_t)rs_parts(N) : 0, b = 4 + 2 * (size_t)B;
    return a > b ? a : b;
}

int k_resample_weights(const float* theta, int N, const int64_t* wid, int Bn, double* stats, float* weights, float* scratch, hipStream_t s) {
    RGQA_REQUIRE(theta != nullptr && stats != nullptr && scratch != nullptr, "resample_weights: null theta / stats / scratch pointer");
    RGQA_REQUIRE(N > 0 && Bn >= 0 && (Bn == 0 || (wid != nullptr && weights != nullptr)), "resample_weights: bad shape N=%d Bn=%d, or null wid / weights", N, Bn);
    RGQA_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 7) == 0, "resample_weights: stats must be 8-byte aligned");
    const int G = rs_parts(N);
    hipLaunchKernelGGL(resample_sum_kernel, dim3(G), dim3(RS_T), 0, s, theta, N, vec16_ok(theta, 0), scratch);
    RGQA_LAUNCH_CHECK("resample_sum_kernel");
    hipLaunchKernelGGL(resample_weights_kernel, dim3(1), dim3(RS_T), 0, s, (const float*)scratch, G, theta, N, wid, Bn, stats, weights);
    RGQA_LAUNCH_CHECK("resample_weights_kernel");
    return RGQA_OK;
}

int k_resample_loss(const float* logits, int ld, const float* target, int ldt, int B, int n_pos, int NA, int NAp, const float* weights, float grad_scale, float* loss3,
                    float* dlogits, int ldd, float* row_loss, float* scratch, hipStream_t s) {
    RGQA_REQUIRE(logits != nullptr && target != nullptr && weights != nullptr, "resample_loss: null logits / target / weights pointer");
    RGQA_REQUIRE(B > 1 && n_pos >= 1 && n_pos < B && NA > 0 && NAp >= NA && ld >= NA && ldt >= NA, "resample_loss: bad shape B=%d n_pos=%d NA=%d NAp=%d ld=%d ld_target=%d", B, n_pos, NA,
                 NAp, ld, ldt);
    RGQA_REQUIRE(dlogits == nullptr || ldd >= NAp, "resample_loss: ldd %d < NAp %d", ldd, NAp);
    RGQA_REQUIRE(loss3 == nullptr || scratch != nullptr, "resample_loss: the loss needs rgqa_resample_scratch_floats(N, B) floats of scratch");
    ResampleLossArgs a;
    a.z = logits; a.ld = ld; a.t = target; a.ldt = ldt; a.weights = weights;
    a.B = B; a.n_pos = n_pos; a.NA = NA; a.NAp = NAp; a.gscale = grad_scale;
    a.dz = dlogits; a.ldd = ldd; a.row_loss = row_loss; a.rows = loss3 ? scratch : nullptr;
    a.vz = vec16_ok(logits, ld); a.vt = vec16_ok(target, ldt); a.vd = vec16_ok(dlogits, ldd);
    hipLaunchKernelGGL(resample_loss_kernel, dim3(B), dim3(RS_T), 0, s, a);
    RGQA_LAUNCH_CHECK("resample_loss_kernel");
    if (loss3) {
        hipLaunchKernelGGL(resample_loss_fold_kernel, dim3(1), dim3(RS_T), 0, s, (const float*)scratch, weights, B, n_pos, loss3);
        RGQA_LAUNCH_CHECK("resample_loss_fold_kernel");
    }
    return RGQA_OK;
}

int k_resample_step(float* theta, float* buf, int N, const int64_t* wid, const float* row_loss, int Bn, const double* stats, float lr, float momentum, float* grad_out,
                    float* scratch, hipStream_t s) {
    RGQA_REQUIRE(theta != nullptr && buf != nullptr && wid != nullptr && row_loss != nullptr && stats != nullptr && scratch != nullptr, "resample_step: null pointer");
    RGQA_REQUIRE(N > 0 && Bn > 0, "resample_step: bad shape N=%d Bn=%d", N, Bn);
    RGQA_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 7) == 0, "resample_step: stats must be 8-byte aligned");
    hipLaunchKernelGGL(resample_owner_kernel, dim3(1), dim3(RS_T), 0, s, (const float*)theta, N, wid, row_loss, Bn, stats, scratch);
    RGQA_LAUNCH_CHECK("resample_owner_kernel");
    const int G = (int)(((int64_t)N + RS_CHUNK - 1) / RS_CHUNK);
    hipLaunchKernelGGL(resample_step_kernel, dim3(G), dim3(RS_T), 0, s, theta, buf, N, Bn, (const float*)scratch, lr, momentum, grad_out, vec16_ok(theta, 0), vec16_ok(buf, 0),
                       vec16_ok(grad_out, 0));
    RGQA_LAUNCH_CHECK("resample_step_kernel");
    return RGQA_OK;
}
