// The loss head of the reference's confidence-branch trainer (tasks/gqa_branched.py:126-143, :147, :209-210), from the UQ column of the target to dlogits
// and dconf, fused:
//   id_inds = target[:, -1] == 0;  target = target[:, :-1]                                                            :126-127
//   --mce_loss: _, tgt = target.max(1); loss_ce = CrossEntropyLoss(ignore_index=-1)(logit[id_inds], tgt[id_inds]) * NA   :133-134
//   default:    loss_ce = BCEWithLogitsLoss()(logit[id_inds], target[id_inds]) * NA                                      :136-137
//   conf = sigmoid(conf).squeeze(); loss_conf = binary_cross_entropy(conf, id_inds.float()); loss = loss_ce + loss_conf  :138-142
//   _, label = logit.max(1)  :147 ;  score1 = sigmoid(logit).max(1)[0]  :209
// With n_id answerable rows:  BCE: dz = (sigmoid(z) - t) / n_id on the answerable rows      MCE: dz = (NA / n_id)(softmax(z) - onehot) on them
//                             dz = +0 on the unanswerable rows and on the padded columns;   dconf_b = (sigmoid(c_b) - id_b) / B
// Laid out like energy_loss.hip: the rows meet only in n_id, which the B flags alone fix - every workgroup counts it itself and finishes its row in ONE
// launch; a second one-workgroup launch folds the row shares in a fixed order.  No float atomics: results repeat bit for bit.
//
// Arithmetic.  The element formulas of the BCE form are loss.hip's (rowops.h bce_term / bce_sigmoid); row sums are carried in f64 and travel to the fold
// as (hi, lo) float pairs, as in energy_loss.hip.  The confidence term is one number per row and is formed in f64 in the stable (softplus) form
//   BCE(sigmoid(c), y) = max(c, 0) - c y + log1p(exp(-|c|)),   capped at 100 as torch's log clamp at -100 caps it.
// torch's own f32 path saturates sigmoid(c) to exactly 1 (c >~ 17) or to a denormal / 0 (c <~ -88) first and then clamps the log: its loss term of a
// confidently WRONG row then jumps to 100 where this form keeps growing as |c|, and its gradient sigmoid(c) - y is what this kernel gives as well.
#include "kernels.h"

#define BL_T 256

struct BranchedLossArgs {
    const float* z; int ld;
    const float* c;                 // conf logits [B]
    const float* t; int ldt;        // target_with_uq [B, NA + 1]: column NA is the UQ flag
    int B, NA, NAp, mce;
    float gscale;
    float* dz; int ldd;
    float* dconf; float* conf; int64_t* label; float* score1;
    float* rows;                    // [B][4]: answer-loss share hi, lo | confidence term hi, lo  (null: no loss asked for)
    int vz, vt, vd;                 // 16-byte accesses allowed for z / t / dz
};

__global__ __launch_bounds__(BL_T) void branched_loss_kernel(BranchedLossArgs a) {
    __shared__ double sd[2][4];
    __shared__ float sv[2][4];
    __shared__ int si[3][4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.x;
    const float* z = a.z + (size_t)b * a.ld;
    const float* t = a.t + (size_t)b * a.ldt;
    // ---- the count of the unanswerable rows (every workgroup for itself: B flags)
    int n_out = 0;
    for (int r = tid; r < a.B; r += BL_T) n_out += a.t[(size_t)r * a.ldt + a.NA] != 0.f ? 1 : 0;
    n_out = wave_sum_i(n_out);
    if (lane == 0) si[0][w] = n_out;
    const bool uq = t[a.NA] != 0.f;

    // ---- first sweep: the row's share of the answer loss, the first maximum of the logit row (label, score1), MCE: the first maximum of the target row
    double acc = 0.0;
    float zm = -INFINITY; int zi = 0x7fffffff;
    float tv = -INFINITY; int ti = 0x7fffffff;
    for (int n = 4 * tid; n < a.NA; n += 4 * BL_T) {
        float x[4], y[4];
        row_load4(z, n, a.NA, a.vz, 0.f, x);
        row_load4(t, n, a.NA, a.vt, 0.f, y);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (n + j < a.NA) {
                if (!a.mce) acc += (double)bce_term(x[j], y[j]);
                if (x[j] > zm) { zm = x[j]; zi = n + j; }          // ascending n per thread: the first maximum stays
                if (y[j] > tv) { tv = y[j]; ti = n + j; }
            }
        }
    }
    acc = wave_sum_d(acc);
    wave_first_max(zm, zi);
    wave_first_max(tv, ti);
    if (lane == 0) { sd[0][w] = acc; sv[0][w] = zm; si[1][w] = zi; sv[1][w] = tv; si[2][w] = ti; }
    __syncthreads();
    zm = sv[0][0]; zi = si[1][0]; tv = sv[1][0]; ti = si[2][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) { first_max(zm, zi, sv[0][k], si[1][k]); first_max(tv, ti, sv[1][k], si[2][k]); }
    n_out = (si[0][0] + si[0][1]) + (si[0][2] + si[0][3]);
    const int n_id = a.B - n_out;
    double share = (sd[0][0] + sd[0][1]) + (sd[0][2] + sd[0][3]);
    const int label = zi < a.NA ? zi : 0;             // (a row of NaN logits names no column: column 0)
    const int tgt = ti < a.NA ? ti : 0;
    float inv_s = 0.f;
    if (a.mce && !uq) {
        double se = 0.0;
        for (int n = 4 * tid; n < a.NA; n += 4 * BL_T) {
            float x[4];
            row_load4(z, n, a.NA, a.vz, 0.f, x);
#pragma unroll
            for (int j = 0; j < 4; ++j) if (n + j < a.NA) se += (double)expf(x[j] - zm);
        }
        se = wave_sum_d(se);
        if (lane == 0) sd[1][w] = se;
        __syncthreads();
        se = (sd[1][0] + sd[1][1]) + (sd[1][2] + sd[1][3]);
        share = ((double)zm + log(se)) - (double)z[tgt];        // cross entropy at the first maximum of the target row
        inv_s = (float)(1.0 / se);
    }
    // ---- the confidence term and the per-row outputs
    if (tid == 0) {
        const float c = a.c[b];
        const float sg = 1.0f / (1.0f + expf(-c));
        const float idf = uq ? 0.f : 1.f;
        if (a.conf) a.conf[b] = sg;
        if (a.dconf) a.dconf[b] = (sg - idf) * (1.0f / (float)a.B) * a.gscale;
        if (a.label) a.label[b] = label;
        if (a.score1) a.score1[b] = 1.0f / (1.0f + expf(-zm));
        if (a.rows) {
            const double cd = (double)c;
            const double term = fmin(fmax(cd, 0.0) - cd * (double)idf + log1p(exp(-fabs(cd))), 100.0);
            split_store(a.rows + 4 * (size_t)b, uq ? 0.0 : share);
            split_store(a.rows + 4 * (size_t)b + 2, term);
        }
    }
    if (a.dz == nullptr) return;
    // ---- dlogits: the second sweep over the row; unanswerable rows and the columns NA .. NAp get exact (positive) zeros
    float* d = a.dz + (size_t)b * a.ldd;
    const float inv_n = 1.0f / (float)n_id, ce_scale = (float)a.NA * inv_n;
    for (int n = 4 * tid; n < a.NAp; n += 4 * BL_T) {
        float x[4], y[4], g[4];
        if (!uq) {
            row_load4(z, n, a.NA, a.vz, 0.f, x);
            if (!a.mce) row_load4(t, n, a.NA, a.vt, 0.f, y);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = 0.f;
            if (!uq && n + j < a.NA) {
                if (!a.mce) v = (bce_sigmoid(x[j]) - y[j]) * inv_n * a.gscale;
                else v = (expf(x[j] - zm) * inv_s - (n + j == tgt ? 1.0f : 0.0f)) * ce_scale * a.gscale;
            }
            g[j] = v;
        }
        row_store4(d, n, a.NAp, a.vd, g);
    }
}

// loss[1] = loss_ce, loss[2] = loss_conf, loss[0] = their sum: the B row shares added in a fixed order, in f64.  The mean over an empty answerable subset
// is 0 / 0 = NaN, as torch's is.
__global__ __launch_bounds__(BL_T) void branched_loss_fold_kernel(const float* __restrict__ rows, const float* __restrict__ t, int ldt, int B, int NA, int mce,
                                                                  float* __restrict__ loss) {
    __shared__ double sd[2][4];
    __shared__ int si[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double ce = 0.0, cf = 0.0;
    int n_out = 0;
    for (int b = tid; b < B; b += BL_T) {
        const float* r = rows + 4 * (size_t)b;
        if (t[(size_t)b * ldt + NA] != 0.f) ++n_out; else ce += (double)r[0] + (double)r[1];
        cf += (double)r[2] + (double)r[3];
    }
    ce = wave_sum_d(ce); cf = wave_sum_d(cf); n_out = wave_sum_i(n_out);
    if (lane == 0) { sd[0][w] = ce; sd[1][w] = cf; si[w] = n_out; }
    __syncthreads();
    if (tid != 0) return;
    ce = (sd[0][0] + sd[0][1]) + (sd[0][2] + sd[0][3]);
    cf = (sd[1][0] + sd[1][1]) + (sd[1][2] + sd[1][3]);
    n_out = (si[0] + si[1]) + (si[2] + si[3]);
    ce = (mce ? (double)NA * ce : ce) / (double)(B - n_out);
    cf = cf / (double)B;
    loss[0] = (float)(ce + cf); loss[1] = (float)ce; loss[2] = (float)cf;
}

size_t k_branched_loss_scratch_floats(int B) { return B > 0 ? 4 * (size_t)B : 0; }

int k_branched_loss(const float* logits, int ld, const float* conf_logit, const float* target_with_uq, int ldt, int B, int NA, int NAp, int mce, float grad_scale,
                    float* loss3, float* dlogits, int ldd, float* dconf, float* conf, int64_t* label, float* score1, float* scratch, hipStream_t s) {
    RGQA_REQUIRE(logits != nullptr && conf_logit != nullptr && target_with_uq != nullptr, "branched_loss: null logits / conf_logit / target pointer");
    RGQA_REQUIRE(B > 0 && NA > 0 && NAp >= NA && ld >= NA && ldt >= NA + 1, "branched_loss: bad shape B=%d NA=%d NAp=%d ld=%d ld_target=%d (the target carries the UQ column)",
                 B, NA, NAp, ld, ldt);
    RGQA_REQUIRE(dlogits == nullptr || ldd >= NAp, "branched_loss: ldd %d < NAp %d", ldd, NAp);
    RGQA_REQUIRE(loss3 == nullptr || scratch != nullptr, "branched_loss: the loss needs rgqa_op_branched_loss_scratch_floats(B) floats of scratch");
    BranchedLossArgs a;
    a.z = logits; a.ld = ld; a.c = conf_logit; a.t = target_with_uq; a.ldt = ldt;
    a.B = B; a.NA = NA; a.NAp = NAp; a.mce = mce ? 1 : 0; a.gscale = grad_scale;
    a.dz = dlogits; a.ldd = ldd; a.dconf = dconf; a.conf = conf; a.label = label; a.score1 = score1; a.rows = loss3 ? scratch : nullptr;
    a.vz = vec16_ok(logits, ld); a.vt = vec16_ok(target_with_uq, ldt); a.vd = vec16_ok(dlogits, ldd);
    hipLaunchKernelGGL(branched_loss_kernel, dim3(B), dim3(BL_T), 0, s, a);
    RGQA_LAUNCH_CHECK("branched_loss_kernel");
    if (loss3) {
        hipLaunchKernelGGL(branched_loss_fold_kernel, dim3(1), dim3(BL_T), 0, s, scratch, target_with_uq, ldt, B, NA, a.mce, loss3);
        RGQA_LAUNCH_CHECK("branched_loss_fold_kernel");
    }
    return RGQA_OK;
}
