// The loss head of the reference's energy fine-tuning (tasks/gqa_energy.py:117-145), from the UQ column of the target to dlogits, fused:
//   id_inds = target[:, -1] == 0;  target = target[:, :-1]                                                           :122-123
//   --mceLoss: _, tgt = target.max(1); loss = CrossEntropyLoss(ignore_index=-1)(logit, tgt) * NA; E_f = logsumexp(logit, 1)   :128-131
//   default:   loss = BCEWithLogitsLoss()(logit, target) * NA;  E_f = log(1 + exp(logit)).sum(1)                      :133-135
//   loss += 0.1 * (relu(-E_f[id_inds] - m_in)**2).mean() + 0.1 * (relu(m_out + E_f[~id_inds])**2).mean()              :137-138
//   _, label = sigmoid(logit).max(1); score = E_f                                                                     :144-145
// With c_b = -2 w relu(-E_b - m_in) / n_in (ID rows) or +2 w relu(m_out + E_b) / n_out (OOD rows):
//   BCE: dz = ((sigmoid(z) - t) / B + c_b sigmoid(z)) grad_scale          MCE: dz = ((NA / B)(softmax(z) - onehot) + c_b softmax(z)) grad_scale
// The rows meet only in the counts n_in / n_out, which the B flags alone fix: every workgroup counts them itself and finishes its row in ONE launch
// (the 7-KiB row is re-read from cache for the gradient sweep); a second one-workgroup launch folds the row shares of the loss in a fixed order.
// No float atomics anywhere: results repeat bit for bit.
//
// Arithmetic.  The element formulas of the BCE form are loss.hip's (rowops.h bce_term / bce_sigmoid): with c_b an exact zero - weight 0, or a row
// whose hinge is inactive - a row of dlogits has the bits bce_kernel gives.  The softplus is score.hip's naive one, as the reference writes it (+inf
// above logit 88.7 like torch's; nothing is promised there).  Row sums (loss share, energy, softmax denominator) are carried in f64 and the row shares
// travel to the fold as (hi, lo) float pairs: 1842 f32 terms summed in f32 would lose 3-4 bits of a loss that a trainer compares between runs to 7
// digits, and an f64 add costs nothing in a kernel this far from any limit.
//
// Element -> thread mapping.  Thread t owns the column quads 4 (t + 256 i) .. + 3.  A quad is ONE 16-byte access where base and pitch of the operand
// allow (the engines' logits and dlogits: pitch NAp, a multiple of 64) and four 4-byte accesses where they do not (a target of NA + 1 columns: rows
// start on odd words); the mapping - and with it every sum's order - is the same in both forms, so a result does not depend on the operands' alignment
// (rowops.h row_load4 / row_store4, with the fixed-order reductions).
#include "kernels.h"

#define EL_T 256

struct EnergyLossArgs {
    const float* z; int ld;
    const float* t; int ldt;
    const float* flag; int ldf;
    int B, NA, NAp, mce;
    float weight, m_in, m_out, gscale;
    float* dz; int ldd;
    float* energy; int64_t* label;
    float* rows;                    // [B][4]: loss share hi, lo | hinge^2 hi, lo  (null: no loss asked for)
    int vz, vt, vd;                 // 16-byte accesses allowed for z / t / dz
};

__global__ __launch_bounds__(EL_T) void energy_loss_kernel(EnergyLossArgs a) {
    __shared__ double sd[3][4];
    __shared__ float sv[3][4];
    __shared__ int si[4][4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.x;
    const float* z = a.z + (size_t)b * a.ld;
    const float* t = a.t + (size_t)b * a.ldt;
    // ---- the counts of the two subsets (every workgroup for itself: B flags)
    int n_out = 0;
    for (int r = tid; r < a.B; r += EL_T) n_out += a.flag[(size_t)r * a.ldf] != 0.f ? 1 : 0;
    n_out = wave_sum_i(n_out);
    if (lane == 0) si[0][w] = n_out;
    const bool ood = a.flag[(size_t)b * a.ldf] != 0.f;

    double share = 0.0, E = 0.0;       // the row's part of the base loss (before the 1 / B, and the NA of the MCE form), its energy
    float zmax = 0.f, inv_s = 0.f;     // MCE: the softmax of the row is expf(z - zmax) * inv_s
    int tgt = 0;
    float best = -1.0f; int besti = 0x7fffffff;      // label: sigmoid values are >= 0
    if (!a.mce) {
        double acc = 0.0, en = 0.0;
        for (int n = 4 * tid; n < a.NA; n += 4 * EL_T) {
            float x[4], y[4];
            row_load4(z, n, a.NA, a.vz, 0.f, x);
            row_load4(t, n, a.NA, a.vt, 0.f, y);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (n + j < a.NA) {
                    acc += (double)bce_term(x[j], y[j]);
                    en += (double)softplus_naive(x[j]);
                    const float sg = 1.0f / (1.0f + expf(-x[j]));     // score_rows_kernel's expression at temperature 1: the same label
                    if (sg > best) { best = sg; besti = n + j; }      // ascending n per thread: the first maximum stays
                }
            }
        }
        acc = wave_sum_d(acc); en = wave_sum_d(en);
        wave_first_max(best, besti);
        if (lane == 0) { sd[0][w] = acc; sd[1][w] = en; sv[0][w] = best; si[1][w] = besti; }
        __syncthreads();
        share = (sd[0][0] + sd[0][1]) + (sd[0][2] + sd[0][3]);
        E = (sd[1][0] + sd[1][1]) + (sd[1][2] + sd[1][3]);
    } else {
        float zm = -INFINITY, tv = -INFINITY; int ti = 0x7fffffff;
        for (int n = 4 * tid; n < a.NA; n += 4 * EL_T) {
            float x[4], y[4];
            row_load4(z, n, a.NA, a.vz, 0.f, x);
            row_load4(t, n, a.NA, a.vt, 0.f, y);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (n + j < a.NA) {
                    zm = fmaxf(zm, x[j]);
                    if (y[j] > tv) { tv = y[j]; ti = n + j; }
                    const float sg = 1.0f / (1.0f + expf(-x[j]));
                    if (sg > best) { best = sg; besti = n + j; }
                }
            }
        }
        zm = wave_max(zm);
        wave_first_max(tv, ti);
        wave_first_max(best, besti);
        if (lane == 0) { sv[1][w] = zm; sv[2][w] = tv; si[2][w] = ti; sv[0][w] = best; si[1][w] = besti; }
        __syncthreads();
        zmax = fmaxf(fmaxf(sv[1][0], sv[1][1]), fmaxf(sv[1][2], sv[1][3]));
        tv = sv[2][0]; ti = si[2][0];
#pragma unroll
        for (int k = 1; k < 4; ++k) first_max(tv, ti, sv[2][k], si[2][k]);
        tgt = ti < a.NA ? ti : 0;                     // (a row of NaN targets names no column: column 0, in bounds)
        double se = 0.0;
        for (int n = 4 * tid; n < a.NA; n += 4 * EL_T) {
            float x[4];
            row_load4(z, n, a.NA, a.vz, 0.f, x);
#pragma unroll
            for (int j = 0; j < 4; ++j) if (n + j < a.NA) se += (double)expf(x[j] - zmax);
        }
        se = wave_sum_d(se);
        if (lane == 0) sd[2][w] = se;
        __syncthreads();
        se = (sd[2][0] + sd[2][1]) + (sd[2][2] + sd[2][3]);
        E = (double)zmax + log(se);                   // logsumexp(logit, 1)
        share = E - (double)z[tgt];                   // cross entropy at the first maximum of the target row
        inv_s = (float)(1.0 / se);
    }
    best = sv[0][0]; besti = si[1][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) first_max(best, besti, sv[0][k], si[1][k]);
    n_out = (si[0][0] + si[0][1]) + (si[0][2] + si[0][3]);
    const int n_in = a.B - n_out;
    // ---- the row's hinge and its coefficient: an inactive hinge gives an EXACT zero
    const double h = ood ? fmax((double)a.m_out + E, 0.0) : fmax(-E - (double)a.m_in, 0.0);
    const float cb = ood ? (float)(2.0 * (double)a.weight * h / (double)n_out) : (float)(-2.0 * (double)a.weight * h / (double)n_in);
    if (tid == 0) {
        if (a.energy) a.energy[b] = (float)E;
        if (a.label) a.label[b] = besti;
        if (a.rows) { split_store(a.rows + 4 * (size_t)b, share); split_store(a.rows + 4 * (size_t)b + 2, h * h); }
    }
    if (a.dz == nullptr) return;
    // ---- dlogits: the second sweep over the row; columns NA .. NAp get exact zeros (they feed K-padded GEMMs)
    float* d = a.dz + (size_t)b * a.ldd;
    const float inv_b = 1.0f / (float)a.B, ce_scale = (float)a.NA * inv_b;
    for (int n = 4 * tid; n < a.NAp; n += 4 * EL_T) {
        float x[4], y[4], g[4];
        row_load4(z, n, a.NA, a.vz, 0.f, x);
        if (!a.mce) row_load4(t, n, a.NA, a.vt, 0.f, y);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = 0.f;
            if (n + j < a.NA) {
                if (!a.mce) {
                    const float sg = bce_sigmoid(x[j]);
                    v = fmaf(cb, sg, (sg - y[j]) * inv_b) * a.gscale;          // cb == 0: (sg - y) * inv_b * gscale, bce_kernel's value
                } else {
                    const float p = expf(x[j] - zmax) * inv_s;
                    v = fmaf(cb, p, (p - (n + j == tgt ? 1.0f : 0.0f)) * ce_scale) * a.gscale;
                }
            }
            g[j] = v;
        }
        row_store4(d, n, a.NAp, a.vd, g);
    }
}

// loss[0] = base + regulariser, loss[1] = base, loss[2] = regulariser: the B row shares added in a fixed order, in f64.  The mean over an empty
// subset is 0 / 0 = NaN, as torch's is.
__global__ __launch_bounds__(EL_T) void energy_loss_fold_kernel(const float* __restrict__ rows, const float* __restrict__ flag, int ldf, int B, int NA, int mce, float weight,
                                                                float* __restrict__ loss) {
    __shared__ double sd[3][4];
    __shared__ int si[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double base = 0.0, hin = 0.0, hout = 0.0;
    int n_out = 0;
    for (int b = tid; b < B; b += EL_T) {
        const float* r = rows + 4 * (size_t)b;
        base += (double)r[0] + (double)r[1];
        const double h2 = (double)r[2] + (double)r[3];
        if (flag[(size_t)b * ldf] != 0.f) { hout += h2; ++n_out; } else hin += h2;
    }
    base = wave_sum_d(base); hin = wave_sum_d(hin); hout = wave_sum_d(hout); n_out = wave_sum_i(n_out);
    if (lane == 0) { sd[0][w] = base; sd[1][w] = hin; sd[2][w] = hout; si[w] = n_out; }
    __syncthreads();
    if (tid != 0) return;
    base = (sd[0][0] + sd[0][1]) + (sd[0][2] + sd[0][3]);
    hin = (sd[1][0] + sd[1][1]) + (sd[1][2] + sd[1][3]);
    hout = (sd[2][0] + sd[2][1]) + (sd[2][2] + sd[2][3]);
    n_out = (si[0] + si[1]) + (si[2] + si[3]);
    base = (mce ? (double)NA * base : base) / (double)B;
    const double reg = (double)weight * (hin / (double)(B - n_out)) + (double)weight * (hout / (double)n_out);
    loss[0] = (float)(base + reg); loss[1] = (float)base; loss[2] = (float)reg;
}

size_t k_energy_loss_scratch_floats(int B) { return B > 0 ? 4 * (size_t)B : 0; }

int k_energy_loss(const float* logits, int ld, const float* target, int ldt, const float* ood_flag, int ldf, int B, int NA, int NAp, const EnergyLossCfg& c, float grad_scale,
                  float* loss3, float* dlogits, int ldd, float* energy, int64_t* label, float* scratch, hipStream_t s) {
    RGQA_REQUIRE(logits != nullptr && target != nullptr && ood_flag != nullptr, "energy_loss: null logits / target / flag pointer");
    RGQA_REQUIRE(B > 0 && NA > 0 && NAp >= NA && ld >= NA && ldt >= NA && ldf >= 1, "energy_loss: bad shape B=%d NA=%d NAp=%d ld=%d ld_target=%d ld_flag=%d", B, NA, NAp, ld, ldt, ldf);
    RGQA_REQUIRE(dlogits == nullptr || ldd >= NAp, "energy_loss: ldd %d < NAp %d", ldd, NAp);
    RGQA_REQUIRE(c.weight >= 0.f, "energy_loss: the regulariser's weight must not be negative");
    RGQA_REQUIRE(loss3 == nullptr || scratch != nullptr, "energy_loss: the loss needs rgqa_op_energy_loss_scratch_floats(B) floats of scratch");
    EnergyLossArgs a;
    a.z = logits; a.ld = ld; a.t = target; a.ldt = ldt; a.flag = ood_flag; a.ldf = ldf;
    a.B = B; a.NA = NA; a.NAp = NAp; a.mce = c.mce ? 1 : 0;
    a.weight = c.weight; a.m_in = c.m_in; a.m_out = c.m_out; a.gscale = grad_scale;
    a.dz = dlogits; a.ldd = ldd; a.energy = energy; a.label = label; a.rows = loss3 ? scratch : nullptr;
    a.vz = vec16_ok(logits, ld); a.vt = vec16_ok(target, ldt); a.vd = vec16_ok(dlogits, ldd);
    hipLaunchKernelGGL(energy_loss_kernel, dim3(B), dim3(EL_T), 0, s, a);
    RGQA_LAUNCH_CHECK("energy_loss_kernel");
    if (loss3) {
        hipLaunchKernelGGL(energy_loss_fold_kernel, dim3(1), dim3(EL_T), 0, s, scratch, ood_flag, ldf, B, NA, a.mce, c.weight, loss3);
        RGQA_LAUNCH_CHECK("energy_loss_fold_kernel");
    }
    return RGQA_OK;
}
