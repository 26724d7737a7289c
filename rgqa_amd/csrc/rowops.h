// The row primitives of the "one workgroup (256 threads, four waves) per logits row" units: energy_loss.hip, branched_loss.hip, resample.hip.
// They carry the two promises those units make: every reduction has a FIXED order (xor butterflies inside a wave, (w0 + w1) + (w2 + w3) across the
// waves - no atomics), and thread t owns the same elements whether a quad moves by one 16-byte access or by four 4-byte ones, so a result repeats
// bit for bit and does not depend on the operands' alignment.
// The text uses only __device__ / __forceinline__, __shfl_xor(v, o, 64), __syncthreads, threadIdx, load4 / store4 (common.h), __expf and <math.h>:
// tests/host_emu/kernels.h includes this very file, so the host emulation runs the shipped formulas.  Included by kernels.h.
#pragma once

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// (value, index): the larger value wins, among equal values the lower index - the first maximum, whatever the order the candidates meet in
__device__ __forceinline__ void first_max(float& v, int& i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
__device__ __forceinline__ void wave_first_max(float& v, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        first_max(v, i, ov, oi);
    }
}
// elements n .. n + 3 of a row (n % 4 == 0); elements >= lim read as `fill` and are never touched in memory.  vec: 16-byte accesses allowed (vec16_ok)
__device__ __forceinline__ void row_load4(const float* row, int n, int lim, int vec, float fill, float v[4]) {
    if (vec && n + 3 < lim) { load4(row + n, v); return; }
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = n + j < lim ? row[n + j] : fill;
}
__device__ __forceinline__ void row_store4(float* row, int n, int lim, int vec, const float v[4]) {
    if (vec && n + 3 < lim) { store4(row + n, v); return; }
#pragma unroll
    for (int j = 0; j < 4; ++j) if (n + j < lim) row[n + j] = v[j];
}
// a double as a (hi, lo) float pair: hi + lo in f64 gives it back to 48 bits
__device__ __forceinline__ void split_store(float* p, double v) {
    const float hi = (float)v;
    p[0] = hi; p[1] = (float)(v - (double)hi);        // (inf / NaN: lo = NaN, and hi + lo is NaN / inf again in the fold - nothing is promised there)
}
// the four wave sums of a workgroup, added in a fixed order (every thread gets the result)
__device__ __forceinline__ double block_sum_d(double v, double* sh /* [4] */) {
    v = wave_sum_d(v);
    __syncthreads();                                   // (sh may still be read from a previous use)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// The element formulas of the BCE head, shared by bce_kernel (loss.hip) and the loss heads above: a row of the energy loss whose regulariser
// coefficient is an exact zero gets the dlogits bits of bce_kernel.
__device__ __forceinline__ float bce_term(float x, float y) { return fmaxf(x, 0.f) - x * y + log1pf(__expf(-fabsf(x))); }
__device__ __forceinline__ float bce_sigmoid(float x) { return 1.f / (1.f + __expf(-x)); }
// log(1 + exp(x)) as the reference writes it (tasks/gqa_energy.py:135,185): +inf above x = 88.7, as torch's (score.hip, energy_loss.hip)
__device__ __forceinline__ float softplus_naive(float x) { return logf(1.0f + expf(x)); }

// host: may the quads of an operand (base p, row pitch ld elements) move by 16-byte accesses?
static inline int vec16_ok(const float* p, int ld) { return p != nullptr && (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld & 3) == 0; }
