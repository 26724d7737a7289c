// MFMA attention core for gfx950, head size 64, Lq, Lk <= 64: the one source of the bf16 kernels (attn_mfma.hip) and of the split-f32 ones (attn_x3.hip).
// Reference semantics: BertAttention.forward, lxrt/modeling.py:326-346.
//
// One 64-lane wave (= one workgroup) per (sample, head).  Scores are produced TRANSPOSED,
//   S^T[key][query] = K Q^T   via v_mfma_f32_16x16x32_bf16(a = K fragment, b = Q fragment)
// so that each lane owns ONE query column and 4 keys per 16-key tile: the softmax reduction is lane-local plus
// two xor-shuffles (lane groups 16/32), and the probability tile is, without any data movement, the B operand of
//   ctx^T[d][query] = V^T P^T
// whose A operand (V transposed) comes from a row-major LDS image of V through ds_read_b64_tr_b16.
// K and Q fragments are loaded straight from HBM/L2 (16 B per lane and plane).  Nothing of size [Lq,Lk] ever leaves registers.
//
// Backward recomputes P from the saved log-sum-exp, in both orientations (lane = query for dQ; lane = key for
// dK / dV), so every gradient is again a chain of MFMAs fed from accumulators: 5 products as in flash-style
// backward, no atomics, each output element written exactly once.
//
// Everything is a template on an operand policy P, which says only what differs between the two precisions:
//   P::elem    element type of the tensors (bf16_t | sf32)
//   P::PLANES  bf16 planes an operand consists of: 1 = the bf16 value; 2 = (hi, lo) of a split-f32 value (common.h).  A 32-dim contraction step of a row
//              is PLANES consecutive 64-byte pieces in memory ([32 hi | 32 lo] for split f32), and every LDS image is PLANES consecutive bf16 images
//   P::split   one f32 value -> its PLANES bf16 parts, leading part first: the pack step of accumulators into fragments and output pieces
//   P::mma     c += A B on fragments of PLANES parts, in the unit's fixed MFMA order
//   P::NAME, P::LD_MULT, P::OUT_LD_MULT, P::ALIGN, P::OUT_ALIGN   message prefix and constants of the operand check
// A unit defines its policy and names its four kernels with ATTN_CORE_UNIT (end of this file).
#pragma once
#include "kernels.h"

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
#define ROWB 144  // LDS row pitch in bytes for a [rows][64] bf16 image (128 + 16: spreads 8 consecutive rows over banks)
#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)

template <int PL> struct frag8 { bf16x8 p[PL]; };      // an MFMA operand fragment: 8 values per lane, leading part first
template <int PL> struct frag4 { bf16x4 p[PL]; };      // 4 consecutive output values of a lane, as they leave an accumulator tile

// Operand fragment of contraction step s (dims 32s .. 32s+31) of a head slice: `base` = element (row 0, dim 0) of the head (wave-uniform),
// off = the lane's byte offset attn_row_off(row, nrows, row pitch in bytes, 16 * g) (kernels.h: the clamp is there).
// Rows past the sample's length are read from its LAST valid row instead of being zero-filled under a branch (4 v_mov + an exec-mask
// branch per fragment: 8-9 % of these kernels' instructions): whatever such a row holds is finite and only ever multiplies a probability
// that is exactly 0 (masked key: exp(-inf); query row past Lq: forced to 0 in the backward kernels, never stored in the forward one).
template <class P>
__device__ __forceinline__ frag8<P::PLANES> ldfrag(const unsigned char* base, uint32_t off, int s) {
    const unsigned char* p = base + off + s * (64 * P::PLANES);
    frag8<P::PLANES> f;
#pragma unroll
    for (int i = 0; i < P::PLANES; ++i) f.p[i] = *reinterpret_cast<const bf16x8*>(p + 64 * i);
    return f;
}
template <class P>
__device__ __forceinline__ const unsigned char* head_base(const void* p, size_t row0, int ld, int h) {
    return reinterpret_cast<const unsigned char*>(reinterpret_cast<const typename P::elem*>(p) + row0 * ld + h * 64);
}
template <class P>
__device__ __forceinline__ unsigned char* head_base(void* p, size_t row0, int ld, int h) {
    return reinterpret_cast<unsigned char*>(reinterpret_cast<typename P::elem*>(p) + row0 * ld + h * 64);
}
// f32 accumulators -> operand parts: two quads to a fragment, one quad to an output piece
template <class P>
__device__ __forceinline__ frag8<P::PLANES> pack8(const f32x4& a, const f32x4& b) {
    frag8<P::PLANES> r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        bf16_t t[P::PLANES];
        P::split(a[i], t);
#pragma unroll
        for (int pl = 0; pl < P::PLANES; ++pl) r.p[pl][i] = t[pl];
        P::split(b[i], t);
#pragma unroll
        for (int pl = 0; pl < P::PLANES; ++pl) r.p[pl][4 + i] = t[pl];
    }
    return r;
}
template <class P>
__device__ __forceinline__ frag4<P::PLANES> pack4(const f32x4& o) {
    frag4<P::PLANES> r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        bf16_t t[P::PLANES];
        P::split(o[i], t);
#pragma unroll
        for (int pl = 0; pl < P::PLANES; ++pl) r.p[pl][i] = t[pl];
    }
    return r;
}
// a fragment / a quad into an LDS image: part pl at byte `off` of plane pl (planes are `plane` bytes apart)
template <int PL>
__device__ __forceinline__ void lds_put(unsigned char* img, int plane, int off, const frag8<PL>& f) {
#pragma unroll
    for (int pl = 0; pl < PL; ++pl) *reinterpret_cast<bf16x8*>(img + pl * plane + off) = f.p[pl];
}
template <int PL>
__device__ __forceinline__ void lds_put(unsigned char* img, int plane, int off, const frag4<PL>& f) {
#pragma unroll
    for (int pl = 0; pl < PL; ++pl) *reinterpret_cast<bf16x4*>(img + pl * plane + off) = f.p[pl];
}
// transposed fragment: element jj = tile[ (jj<4 ? r0a : r0b) + 4*g + (jj&3) ][ c0 + (lane&15) ]
template <int PITCH>
__device__ __forceinline__ bf16x8 trfrag1(const unsigned char* tile, int r0a, int r0b, bool has_b, int c0, int lane) {
    const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
    const unsigned char* a1 = tile + (r0a + 4 * g + q) * PITCH + (c0 + 4 * p) * 2;
    bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)a1);
    bf16x4 hi = {0, 0, 0, 0};
    if (has_b) {
        const unsigned char* a2 = tile + (r0b + 4 * g + q) * PITCH + (c0 + 4 * p) * 2;
        hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)a2);
    }
    bf16x8 r;
    r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
    r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
    return r;
}
template <class P, int PITCH = ROWB>
__device__ __forceinline__ frag8<P::PLANES> trfrag(const unsigned char* img, int plane, int r0a, int r0b, bool has_b, int c0, int lane) {
    frag8<P::PLANES> f;
#pragma unroll
    for (int pl = 0; pl < P::PLANES; ++pl) f.p[pl] = trfrag1<PITCH>(img + pl * plane, r0a, r0b, has_b, c0, lane);
    return f;
}
// Output tile dt of a row, 16 bytes per lane and plane (kernels.h attn_pair16): an even dt parks its pieces in `ev`, the odd one completes the 32-dim step's
// PLANES 64-byte pieces at base + off (off = the row's byte offset + attn_pair_off(g)) and, when img is set, the 64 bytes of the row's bf16 image (= the leading
// parts) at img + ioff.  Every lane calls it; `valid` guards the stores only.
template <class P>
__device__ __forceinline__ void store16(unsigned char* base, unsigned char* img, bool valid, uint32_t off, uint32_t ioff, int dt, const f32x4& o, frag4<P::PLANES>& ev) {
    const frag4<P::PLANES> t = pack4<P>(o);
    if ((dt & 1) == 0) { ev = t; return; }
    bf16x8 t16[P::PLANES];
#pragma unroll
    for (int pl = 0; pl < P::PLANES; ++pl) t16[pl] = attn_pair16(ev.p[pl], t.p[pl]);
    if (valid) {
        unsigned char* p = base + (off + (dt >> 1) * (64 * P::PLANES));
#pragma unroll
        for (int pl = 0; pl < P::PLANES; ++pl) *reinterpret_cast<bf16x8*>(p + 64 * pl) = t16[pl];
        if (img) *reinterpret_cast<bf16x8*>(img + (ioff + (dt >> 1) * 64)) = t16[0];
    }
}

template <class P>
struct AttnCore {
    typedef frag8<P::PLANES> frag;
    typedef frag4<P::PLANES> quad;
    static constexpr uint32_t EB = sizeof(typename P::elem);      // bytes per element: row pitch = EB * row stride

    // ======================================================================== forward
    template <int NQT, int NKT>
    static constexpr int fwd_smem() { return P::PLANES * NKT * 16 * ROWB; }
    template <int NQT, int NKT>
    static __device__ __forceinline__ void fwd(const AttnArgs& a, const int blk, unsigned char* vs /* fwd_smem<NQT, NKT>() bytes */) {
        constexpr int VPL = NKT * 16 * ROWB;                       // one plane of the V image
        const int lane = threadIdx.x, fr = lane & 15, g = lane >> 4;
        const int b = blk / a.nh, h = blk % a.nh;
        ATTN_SAMPLE_ROWS(a, b)      // q0, k0: first row of this sample; Lq, Lk: its valid row counts (<= a.Lq, a.Lk)
        const unsigned char* Q = head_base<P>(a.q, q0, a.ldq, h);
        const unsigned char* K = head_base<P>(a.k, k0, a.ldk, h);
        const unsigned char* V = head_base<P>(a.v, k0, a.ldv, h);
        const uint32_t pk = EB * (uint32_t)a.ldk, pv = EB * (uint32_t)a.ldv, pq = EB * (uint32_t)a.ldq;      // row pitches in bytes
        // one global-load phase: Q, K, V fragments and the mask requested back to back; the V image for the transposed reads is
        // written from the V registers
        frag qf[NQT][2], kf[NKT][2], vf[NKT][2];
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            const uint32_t ko = attn_row_off(kt * 16 + fr, Lk, pk, 16 * g), vo = attn_row_off(kt * 16 + fr, Lk, pv, 16 * g);
#pragma unroll
            for (int s = 0; s < 2; ++s) { kf[kt][s] = ldfrag<P>(K, ko, s); vf[kt][s] = ldfrag<P>(V, vo, s); }
        }
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt) {
            const uint32_t qo = attn_row_off(qt * 16 + fr, Lq, pq, 16 * g);
#pragma unroll
            for (int s = 0; s < 2; ++s) qf[qt][s] = ldfrag<P>(Q, qo, s);
        }
        f32x4 acc[NKT][NQT];
        float mk[NKT][4];
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = kt * 16 + 4 * g + r;
                mk[kt][r] = key < Lk ? (a.mask ? a.mask[(size_t)b * a.Lk + key] : 0.f) : -INFINITY;
            }
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int s = 0; s < 2; ++s) lds_put(vs, VPL, (kt * 16 + fr) * ROWB + s * 64 + g * 16, vf[kt][s]);
        __syncthreads();
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt) {
                f32x4 c = {0.f, 0.f, 0.f, 0.f};
                c = P::mma(kf[kt][0], qf[qt][0], c);
                c = P::mma(kf[kt][1], qf[qt][1], c);
                acc[kt][qt] = c;
            }
        DropCfg dc = a.drop; dc.seed_hi ^= a.drop_site;
        // dropout index ((b nh + h) a.Lq + q) a.Lk + key, mod 2^32 as before: the wave's part once (scalar), the lane's fr a.Lk + 4 g once
        const uint32_t idx_w = (uint32_t)((b * a.nh + h) * a.Lq) * (uint32_t)a.Lk, idx_l = __umul24(fr, a.Lk) + 4 * g;
        float* lse_w = a.lse ? a.lse + ((size_t)b * a.nh + h) * a.Lq : nullptr;
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt) {
            const int q = qt * 16 + fr;
            const uint32_t idx_q = idx_w + idx_l + (uint32_t)(qt * 16) * (uint32_t)a.Lk;
            float m = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) { float s = acc[kt][qt][r] * a.scale + mk[kt][r]; acc[kt][qt][r] = s; m = fmaxf(m, s); }
            m = fmaxf(m, __shfl_xor(m, 16, 64));
            m = fmaxf(m, __shfl_xor(m, 32, 64));
            float sum = 0.f;
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) { float p = __expf(acc[kt][qt][r] - m); acc[kt][qt][r] = p; sum += p; }
            sum += __shfl_xor(sum, 16, 64);
            sum += __shfl_xor(sum, 32, 64);
            const float inv = 1.f / sum;
            if (g == 0 && q < Lq && lse_w) lse_w[q] = m + __logf(sum);
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) {
                // four consecutive keys of one query row: with an even row length the index is even and one hash serves two elements
                const uint32_t idx = idx_q + kt * 16;
                float v[4] = {acc[kt][qt][0] * inv, acc[kt][qt][1] * inv, acc[kt][qt][2] * inv, acc[kt][qt][3] * inv};
                if ((a.Lk & 1) == 0) drop_apply_vec<4>(dc, idx, v);
                else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = drop_apply(dc, idx + (uint32_t)r, v[r]);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[kt][qt][r] = v[r];
            }
        }
        // ctx^T[d][q] = sum_key V^T[d][key] P^T[key][q]
        unsigned char* O = head_base<P>(a.out, q0, a.ldo, h);
        // bf16x3_fwd precision: the bf16 image of a split-f32 output that the bf16 backward reads (a bf16 output is its own image)
        unsigned char* Ob = P::PLANES > 1 && a.out_b ? reinterpret_cast<unsigned char*>(reinterpret_cast<bf16_t*>(a.out_b) + q0 * a.ldo + h * 64) : nullptr;
        const uint32_t po = EB * (uint32_t)a.ldo, g16 = attn_pair_off(g);
        quad ev[NQT];      // the even dim tile's pieces, held until the odd one completes the 16-byte stores (kernels.h attn_pair16)
        constexpr int NKS = (NKT + 1) / 2;
        const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
        frag pb[NKS][NQT];
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt)
                pb[ks][qt] = pack8<P>(acc[2 * ks][qt], (2 * ks + 1 < NKT) ? acc[(2 * ks + 1 < NKT) ? 2 * ks + 1 : 0][qt] : zero4);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            frag va[NKS];
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) va[ks] = trfrag<P>(vs, VPL, 2 * ks * 16, (2 * ks + 1) * 16, 2 * ks + 1 < NKT, dt * 16, lane);
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt) {
                f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) o = P::mma(va[ks], pb[ks][qt], o);
                const int q = qt * 16 + fr;
                store16<P>(O, Ob, q < Lq, __umul24(q, po) + g16, __umul24(q, 2 * (uint32_t)a.ldo) + g16, dt, o, ev[qt]);
            }
        }
    }

    // ======================================================================== backward, probabilities computed once
    // Query-major pass: P recomputed from the saved log-sum-exp, dP = dO V^T, dS = P (dP - delta) scale, dQ = dS K.  The key-major pass does not
    // recompute S, the softmax, the dropout draws and dP: the query-major pass parks dS[q][key] and Pd[q][key] = dropout(P) (exactly the values it
    // feeds its own dQ MFMAs / the values the key-major pass would recompute) in row-major LDS images, and the key-major pass fetches them as MFMA B
    // operands with the transposed reads it already uses for Q^T and dO^T: dK = dS^T Q, dV = Pd^T dO.  dS takes the K image's place once every dQ
    // is done (held packed in registers until then); the Pd image is the only LDS beyond the operands' (pitch NKT * 32 + 16 bytes).
    // (docs/MEASUREMENTS.md 4.9: these kernels' waves wait rather than fill the issue pipe - a 14 % shorter stream for most language waves moved
    // nothing, 16-byte instead of 8-byte output stores (kernels.h attn_pair16) took 10-17 % off every launch.)
    template <int NQT, int NKT>
    static constexpr int bwd_smem() {
        return P::PLANES * ((NKT * 16 * ROWB > NQT * 16 * (NKT * 32 + 16) ? NKT * 16 * ROWB : NQT * 16 * (NKT * 32 + 16)) + 2 * NQT * 16 * ROWB + NQT * 16 * (NKT * 32 + 16));
    }
    template <int NQT, int NKT>
    static __device__ __forceinline__ void bwd(const AttnArgs& a, const int blk, unsigned char* smem /* bwd_smem<NQT, NKT>() bytes */) {
        constexpr int P2 = NKT * 32 + 16;                  // pitch of the [query][key] images
        // one plane of each image; an image is its PLANES planes, consecutively
        constexpr int KPL = NKT * 16 * ROWB > NQT * 16 * P2 ? NKT * 16 * ROWB : NQT * 16 * P2, QPL = NQT * 16 * ROWB, DPL = NQT * 16 * P2;
        unsigned char* ks_ = smem;                                   // K image; after the query-major pass: dS[q][key]
        unsigned char* qs_ = ks_ + P::PLANES * KPL;
        unsigned char* os_ = qs_ + P::PLANES * QPL;
        unsigned char* pd_ = os_ + P::PLANES * QPL;                  // Pd[q][key] = dropout(P)
        const int lane = threadIdx.x, fr = lane & 15, g = lane >> 4;
        const int b = blk / a.nh, h = blk % a.nh;
        ATTN_SAMPLE_ROWS(a, b)
        const unsigned char* Q = head_base<P>(a.q, q0, a.ldq, h);
        const unsigned char* K = head_base<P>(a.k, k0, a.ldk, h);
        const unsigned char* V = head_base<P>(a.v, k0, a.ldv, h);
        const unsigned char* dO = head_base<P>(a.dout, q0, a.lddo, h);
        const float* lse = a.lse + ((size_t)b * a.nh + h) * a.Lq;
        const uint32_t pk = EB * (uint32_t)a.ldk, pv = EB * (uint32_t)a.ldv, pq = EB * (uint32_t)a.ldq, pdo = EB * (uint32_t)a.lddo;      // row pitches in bytes
        // ONE global-load phase: every operand fragment (both passes use the same 16-B-per-lane row pieces), the log-sum-exp and
        // the key mask are requested back to back; the three LDS images the transposed reads need are then written from those
        // registers.  (The first version re-read K/Q/dO from global for the images and again per pass: ~6 dependent L2/HBM
        // round trips on a 1-wave block.)
        frag kf[NKT][2], vf[NKT][2], qf[NQT][2], of[NQT][2];
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            const uint32_t ko = attn_row_off(kt * 16 + fr, Lk, pk, 16 * g), vo = attn_row_off(kt * 16 + fr, Lk, pv, 16 * g);
#pragma unroll
            for (int s = 0; s < 2; ++s) { kf[kt][s] = ldfrag<P>(K, ko, s); vf[kt][s] = ldfrag<P>(V, vo, s); }
        }
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt) {
            const uint32_t qo = attn_row_off(qt * 16 + fr, Lq, pq, 16 * g), oo = attn_row_off(qt * 16 + fr, Lq, pdo, 16 * g);
#pragma unroll
            for (int s = 0; s < 2; ++s) { qf[qt][s] = ldfrag<P>(Q, qo, s); of[qt][s] = ldfrag<P>(dO, oo, s); }
        }
        float lse_t[NQT], mk[NKT][4];
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt) lse_t[qt] = qt * 16 + fr < Lq ? lse[qt * 16 + fr] : 0.f;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = kt * 16 + 4 * g + r;
                mk[kt][r] = key < Lk ? (a.mask ? a.mask[(size_t)b * a.Lk + key] : 0.f) : -INFINITY;
            }
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int s = 0; s < 2; ++s) lds_put(ks_, KPL, (kt * 16 + fr) * ROWB + s * 64 + g * 16, kf[kt][s]);
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                lds_put(qs_, QPL, (qt * 16 + fr) * ROWB + s * 64 + g * 16, qf[qt][s]);
                lds_put(os_, QPL, (qt * 16 + fr) * ROWB + s * 64 + g * 16, of[qt][s]);
            }
        __syncthreads();
        DropCfg dc = a.drop; dc.seed_hi ^= a.drop_site;
        const uint32_t idx0 = (uint32_t)((b * a.nh + h) * a.Lq) * (uint32_t)a.Lk + __umul24(fr, a.Lk) + 4 * g;      // + the lane's fr a.Lk + 4 g
        const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
        constexpr int NKS = (NKT + 1) / 2, NQS = (NQT + 1) / 2;

        // ---------------- pass T: lane = query, registers = keys  ->  dQ; Pd -> pd_, dS held packed
        quad dsh[NQT][NKT];
        {
            unsigned char* dQ = head_base<P>(a.dq, q0, a.lddq, h);
            const uint32_t pdq = EB * (uint32_t)a.lddq, g16 = attn_pair_off(g);
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt) {
                const int q = qt * 16 + fr;
                const uint32_t idx_q = idx0 + (uint32_t)(qt * 16) * (uint32_t)a.Lk;
                const float lq = lse_t[qt];
                f32x4 pp[NKT], dpp[NKT];
                float delta = 0.f;
#pragma unroll
                for (int kt = 0; kt < NKT; ++kt) {
                    f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, dp4 = {0.f, 0.f, 0.f, 0.f};
                    s4 = P::mma(kf[kt][0], qf[qt][0], s4); s4 = P::mma(kf[kt][1], qf[qt][1], s4);
                    dp4 = P::mma(vf[kt][0], of[qt][0], dp4); dp4 = P::mma(vf[kt][1], of[qt][1], dp4);
                    float keep4[4] = {1.f, 1.f, 1.f, 1.f};
                    {
                        const uint32_t idx = idx_q + kt * 16;
                        if ((a.Lk & 1) == 0) drop_apply_vec<4>(dc, idx, keep4);
                        else {
#pragma unroll
                            for (int r = 0; r < 4; ++r) keep4[r] = drop_apply(dc, idx + (uint32_t)r, 1.0f);
                        }
                    }
                    f32x4 pd4;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float p = q < Lq ? __expf(s4[r] * a.scale + mk[kt][r] - lq) : 0.f;
                        const float keep = keep4[r];
                        const float dp = dp4[r] * keep;
                        delta += p * dp;
                        s4[r] = p; dp4[r] = dp;
                        pd4[r] = p * keep;               // Pd
                    }
                    pp[kt] = s4; dpp[kt] = dp4;
                    lds_put(pd_, DPL, q * P2 + 8 * g + kt * 32, pack4<P>(pd4));      // keys kt*16 + 4g .. +3 of query row q
                }
                delta += __shfl_xor(delta, 16, 64);
                delta += __shfl_xor(delta, 32, 64);
#pragma unroll
                for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) pp[kt][r] = pp[kt][r] * (dpp[kt][r] - delta) * a.scale;   // dS^T
                    dsh[qt][kt] = pack4<P>(pp[kt]);
                }
                // dQ^T[d][q] = sum_key K^T[d][key] dS^T[key][q]
                frag db[NKS];
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) db[ks] = pack8<P>(pp[2 * ks], (2 * ks + 1 < NKT) ? pp[(2 * ks + 1 < NKT) ? 2 * ks + 1 : 0] : zero4);
                quad evq;      // the even dim tile's pieces (kernels.h attn_pair16)
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < NKS; ++ks) {
                        const frag ka = trfrag<P>(ks_, KPL, 2 * ks * 16, (2 * ks + 1) * 16, 2 * ks + 1 < NKT, dt * 16, lane);
                        o = P::mma(ka, db[ks], o);
                    }
                    store16<P>(dQ, nullptr, q < Lq, __umul24(q, pdq) + g16, 0, dt, o, evq);
                }
            }
        }
        __syncthreads();   // every dQ product has read the K image
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) lds_put(ks_, KPL, (qt * 16 + fr) * P2 + kt * 32 + 8 * g, dsh[qt][kt]);
        __syncthreads();
        // ---------------- pass N: lane = key  ->  dK, dV from the parked dS / Pd
        {
            unsigned char* dK = head_base<P>(a.dk, k0, a.lddk, h);
            unsigned char* dV = head_base<P>(a.dv, k0, a.lddv, h);
            const uint32_t pdk = EB * (uint32_t)a.lddk, pdv = EB * (uint32_t)a.lddv, g16 = attn_pair_off(g);
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) {
                const int key = kt * 16 + fr;
                frag dsb[NQS], pdb[NQS];
#pragma unroll
                for (int qs = 0; qs < NQS; ++qs) {
                    const bool two = 2 * qs + 1 < NQT;
                    dsb[qs] = trfrag<P, P2>(ks_, KPL, 2 * qs * 16, (2 * qs + 1) * 16, two, kt * 16, lane);     // element jj = dS[q(jj)][key]
                    pdb[qs] = trfrag<P, P2>(pd_, DPL, 2 * qs * 16, (2 * qs + 1) * 16, two, kt * 16, lane);
                }
                quad evk, evv;
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    f32x4 ok = {0.f, 0.f, 0.f, 0.f}, ov = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int qs = 0; qs < NQS; ++qs) {
                        const bool two = 2 * qs + 1 < NQT;
                        const frag qa = trfrag<P>(qs_, QPL, 2 * qs * 16, (2 * qs + 1) * 16, two, dt * 16, lane);
                        const frag oa = trfrag<P>(os_, QPL, 2 * qs * 16, (2 * qs + 1) * 16, two, dt * 16, lane);
                        ok = P::mma(qa, dsb[qs], ok);   // dK^T[d][key] = sum_q Q^T[d][q] dS[q][key]
                        ov = P::mma(oa, pdb[qs], ov);   // dV^T[d][key] = sum_q dO^T[d][q] Pd[q][key]
                    }
                    store16<P>(dK, nullptr, key < Lk, __umul24(key, pdk) + g16, 0, dt, ok, evk);
                    store16<P>(dV, nullptr, key < Lk, __umul24(key, pdv) + g16, 0, dt, ov, evv);
                }
            }
        }
    }
};

// ============================================================================ kernels
// What a unit's four __global__ functions run (ATTN_CORE_UNIT): one problem per launch, or TWO problems - the language and the vision side of a paired
// stage, or the two directions of a cross-attention stage - in one launch: blocks [0, n0) work on a0 with <Q0, K0> tiles, the rest on a1 with <Q1, K1>
// (block-uniform branch).  Per-sample tile counts: kernels.h ATTN_RUN_TRIMMED.
template <class P, int NQT, int NKT>
__device__ __forceinline__ void attn_fwd_kernel(const AttnArgs& a, const int trim) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[AttnCore<P>::template fwd_smem<NQT, NKT>()];
    ATTN_RUN_TRIMMED(AttnCore<P>::template fwd, NQT, NKT, a, blockIdx.x, smem, trim);
}
template <class P, int NQT, int NKT>
__device__ __forceinline__ void attn_bwd_kernel(const AttnArgs& a, const int trim) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[AttnCore<P>::template bwd_smem<NQT, NKT>()];
    ATTN_RUN_TRIMMED(AttnCore<P>::template bwd, NQT, NKT, a, blockIdx.x, smem, trim);
}
template <class P, int Q0, int K0, int Q1, int K1>
__device__ __forceinline__ void attn_fwd_pair_kernel(const AttnArgs& a0, const AttnArgs& a1, const int n0, const int trim) {
    constexpr int S0 = AttnCore<P>::template fwd_smem<Q0, K0>(), S1 = AttnCore<P>::template fwd_smem<Q1, K1>();
    __shared__ __attribute__((aligned(16))) unsigned char smem[S0 > S1 ? S0 : S1];
    if ((int)blockIdx.x < n0) ATTN_RUN_TRIMMED(AttnCore<P>::template fwd, Q0, K0, a0, blockIdx.x, smem, trim);
    else ATTN_RUN_TRIMMED(AttnCore<P>::template fwd, Q1, K1, a1, blockIdx.x - n0, smem, trim);
}
template <class P, int Q0, int K0, int Q1, int K1>
__device__ __forceinline__ void attn_bwd_pair_kernel(const AttnArgs& a0, const AttnArgs& a1, const int n0, const int trim) {
    constexpr int S0 = AttnCore<P>::template bwd_smem<Q0, K0>(), S1 = AttnCore<P>::template bwd_smem<Q1, K1>();
    __shared__ __attribute__((aligned(16))) unsigned char smem[S0 > S1 ? S0 : S1];
    if ((int)blockIdx.x < n0) ATTN_RUN_TRIMMED(AttnCore<P>::template bwd, Q0, K0, a0, blockIdx.x, smem, trim);
    else ATTN_RUN_TRIMMED(AttnCore<P>::template bwd, Q1, K1, a1, blockIdx.x - n0, smem, trim);
}

// ============================================================================ host side
// The unit that serves element type U: its policy P, its four kernels as templates on the tile counts, and their names (ATTN_CORE_UNIT)
template <typename U> struct AttnUnit;

template <class P>
static int attn_check(const AttnArgs& a, bool bwd) {
    RGQA_REQUIRE(a.dh == 64, "%s attention: head size must be 64 (got %d)", P::NAME, a.dh);
    RGQA_REQUIRE(a.B > 0 && a.nh > 0 && a.Lq > 0 && a.Lk > 0 && a.Lq <= 64 && a.Lk <= 64, "%s attention: Lq/Lk must be in 1..64 (got %d %d)", P::NAME, a.Lq, a.Lk);
    RGQA_REQUIRE(a.q && a.k && a.v && (a.ldq % P::LD_MULT) == 0 && (a.ldk % P::LD_MULT) == 0 && (a.ldv % P::LD_MULT) == 0,
                 "%s attention: null operand or row stride not a multiple of %d", P::NAME, P::LD_MULT);
    RGQA_REQUIRE(((uintptr_t)a.q % P::ALIGN) == 0 && ((uintptr_t)a.k % P::ALIGN) == 0 && ((uintptr_t)a.v % P::ALIGN) == 0, "%s attention: operands must be %d-byte aligned", P::NAME, P::ALIGN);
    // the kernels address a sample's rows with 32-bit lane offsets from a 64-bit wave base (kernels.h ATTN_MAX_LD)
    RGQA_REQUIRE(a.ldq > 0 && a.ldk > 0 && a.ldv > 0 && a.ldq < ATTN_MAX_LD && a.ldk < ATTN_MAX_LD && a.ldv < ATTN_MAX_LD, "%s attention: row stride out of range (1 .. %d)", P::NAME, ATTN_MAX_LD - 1);
    if (bwd) {
        RGQA_REQUIRE(a.dout && a.dq && a.dk && a.dv && a.lse, "%s attention bwd: null operand", P::NAME);
        RGQA_REQUIRE((a.lddo % P::LD_MULT) == 0 && (a.lddq % P::OUT_LD_MULT) == 0 && (a.lddk % P::OUT_LD_MULT) == 0 && (a.lddv % P::OUT_LD_MULT) == 0, "%s attention bwd: bad row strides", P::NAME);
        RGQA_REQUIRE(a.lddo > 0 && a.lddq > 0 && a.lddk > 0 && a.lddv > 0 && a.lddo < ATTN_MAX_LD && a.lddq < ATTN_MAX_LD && a.lddk < ATTN_MAX_LD && a.lddv < ATTN_MAX_LD,
                     "%s attention bwd: row stride out of range (1 .. %d)", P::NAME, ATTN_MAX_LD - 1);
        RGQA_REQUIRE(((uintptr_t)a.dout % P::OUT_ALIGN) == 0 && ((uintptr_t)a.dq % P::OUT_ALIGN) == 0 && ((uintptr_t)a.dk % P::OUT_ALIGN) == 0 && ((uintptr_t)a.dv % P::OUT_ALIGN) == 0,
                     "%s attention bwd: operands must be %d-byte aligned", P::NAME, P::OUT_ALIGN);
    } else {
        RGQA_REQUIRE(a.out && (a.ldo % P::OUT_LD_MULT) == 0 && ((uintptr_t)a.out % P::OUT_ALIGN) == 0, "%s attention: null output / bad stride", P::NAME);
        RGQA_REQUIRE(a.ldo > 0 && a.ldo < ATTN_MAX_LD, "%s attention: row stride out of range (1 .. %d)", P::NAME, ATTN_MAX_LD - 1);
    }
    return RGQA_OK;
}

#define DISPATCH_TILES(KERNEL, nqt, nkt)                                                                          \
    switch ((nqt) * 8 + (nkt)) {                                                                                  \
        case 1 * 8 + 1: hipLaunchKernelGGL((KERNEL<1, 1>), grid, dim3(64), 0, s, a, trim); break;                        \
        case 1 * 8 + 2: hipLaunchKernelGGL((KERNEL<1, 2>), grid, dim3(64), 0, s, a, trim); break;                        \
        case 1 * 8 + 3: hipLaunchKernelGGL((KERNEL<1, 3>), grid, dim3(64), 0, s, a, trim); break;                        \
        case 1 * 8 + 4: hipLaunchKernelGGL((KERNEL<1, 4>), grid, dim3(64), 0, s, a, trim); break;                        \
        case 2 * 8 + 1: hipLaunchKernelGGL((KERNEL<2, 1>), grid, dim3(64), 0, s, a, trim); break;                        \
        case 2 * 8 + 2: hipLaunchKernelGGL((KERNEL<2, 2>), grid, dim3(64), 0, s, a, trim); break;                        \
        case 2 * 8 + 3: hipLaunchKernelGGL((KERNEL<2, 3>), grid, dim3(64), 0, s, a, trim); break;                        \
        case 2 * 8 + 4: hipLaunchKernelGGL((KERNEL<2, 4>), grid, dim3(64), 0, s, a, trim); break;                        \
        case 3 * 8 + 1: hipLaunchKernelGGL((KERNEL<3, 1>), grid, dim3(64), 0, s, a, trim); break;                        \
        case 3 * 8 + 2: hipLaunchKernelGGL((KERNEL<3, 2>), grid, dim3(64), 0, s, a, trim); break;                        \
        case 3 * 8 + 3: hipLaunchKernelGGL((KERNEL<3, 3>), grid, dim3(64), 0, s, a, trim); break;                        \
        case 3 * 8 + 4: hipLaunchKernelGGL((KERNEL<3, 4>), grid, dim3(64), 0, s, a, trim); break;                        \
        case 4 * 8 + 1: hipLaunchKernelGGL((KERNEL<4, 1>), grid, dim3(64), 0, s, a, trim); break;                        \
        case 4 * 8 + 2: hipLaunchKernelGGL((KERNEL<4, 2>), grid, dim3(64), 0, s, a, trim); break;                        \
        case 4 * 8 + 3: hipLaunchKernelGGL((KERNEL<4, 3>), grid, dim3(64), 0, s, a, trim); break;                        \
        default: hipLaunchKernelGGL((KERNEL<4, 4>), grid, dim3(64), 0, s, a, trim); break;                               \
    }

// The two attention problems of a stage in ONE launch when their tile shapes are the GQA ones (questions of 17..32 tokens, 33..48 regions):
// self-attention <2,2> + <3,3>, cross-attention <2,3> + <3,2>; the heavier problem's blocks first.
static int pair_shape(const AttnArgs& a0, const AttnArgs& a1) {
    const int q0 = cdiv(a0.Lq, 16), k0 = cdiv(a0.Lk, 16), q1 = cdiv(a1.Lq, 16), k1 = cdiv(a1.Lk, 16);
    if (a0.nh != a1.nh || a0.dh != a1.dh) return 0;
    if (q0 == 3 && k0 == 3 && q1 == 2 && k1 == 2) return 1;
    if (q0 == 3 && k0 == 2 && q1 == 2 && k1 == 3) return 2;
    return 0;
}
template <typename U, bool BWD>
static int attn_launch(const AttnArgs& a, hipStream_t s) {
    typedef AttnUnit<U> K;
    int r = attn_check<typename K::P>(a, BWD);
    if (r) return r;
    const int nqt = cdiv(a.Lq, 16), nkt = cdiv(a.Lk, 16);
    dim3 grid(a.B * a.nh);
    const int trim = g_rgqa_attn_trim != 0 && (a.cu_q || a.cu_k);
    if (BWD) { DISPATCH_TILES(K::template bwd, nqt, nkt) }
    else { DISPATCH_TILES(K::template fwd, nqt, nkt) }
    RGQA_LAUNCH_CHECK(BWD ? K::bwd_name : K::fwd_name);
    return RGQA_OK;
}
// returns 1 when it launched, 0 when the caller should launch the two problems separately, < 0 on error
template <typename U, bool BWD>
static int attn_launch_pair(const AttnArgs& x, const AttnArgs& y, hipStream_t s) {
    typedef AttnUnit<U> K;
    const bool swap = x.Lq * x.Lk < y.Lq * y.Lk || (x.Lq * x.Lk == y.Lq * y.Lk && x.Lq < y.Lq);
    const AttnArgs& a0 = swap ? y : x; const AttnArgs& a1 = swap ? x : y;
    const int shape = pair_shape(a0, a1);
    if (shape == 0) return 0;
    int r = attn_check<typename K::P>(a0, BWD); if (r) return r;
    r = attn_check<typename K::P>(a1, BWD); if (r) return r;
    const int n0 = a0.B * a0.nh;
    dim3 grid(n0 + a1.B * a1.nh);
    const int trim = g_rgqa_attn_trim != 0 && (a0.cu_q || a0.cu_k || a1.cu_q || a1.cu_k);
    if (BWD) {
        if (shape == 1) hipLaunchKernelGGL((K::template bwd_pair<3, 3, 2, 2>), grid, dim3(64), 0, s, a0, a1, n0, trim);
        else hipLaunchKernelGGL((K::template bwd_pair<3, 2, 2, 3>), grid, dim3(64), 0, s, a0, a1, n0, trim);
    } else {
        if (shape == 1) hipLaunchKernelGGL((K::template fwd_pair<3, 3, 2, 2>), grid, dim3(64), 0, s, a0, a1, n0, trim);
        else hipLaunchKernelGGL((K::template fwd_pair<3, 2, 2, 3>), grid, dim3(64), 0, s, a0, a1, n0, trim);
    }
    RGQA_LAUNCH_CHECK(BWD ? K::bwd_pair_name : K::fwd_pair_name);
    return 1;
}
template <typename U> int k_attn_fwd_mfma(const AttnArgs& a, hipStream_t s) { return attn_launch<U, false>(a, s); }
template <typename U> int k_attn_bwd_mfma(const AttnArgs& a, hipStream_t s) { return attn_launch<U, true>(a, s); }
template <typename U> int k_attn_fwd_mfma_pair(const AttnArgs& a0, const AttnArgs& a1, hipStream_t s) { return attn_launch_pair<U, false>(a0, a1, s); }
template <typename U> int k_attn_bwd_mfma_pair(const AttnArgs& a0, const AttnArgs& a1, hipStream_t s) { return attn_launch_pair<U, true>(a0, a1, s); }

// A unit: the four kernels of policy POLICY under their profile-visible names (tools/ and profiles/ classify launches by them), the AttnUnit that
// hands them to the launchers above, and the launchers' instantiation for element type U.
#define ATTN_CORE_UNIT(U, POLICY, FWD, BWD, FWD_PAIR, BWD_PAIR)                                                                                      \
    template <int NQT, int NKT>                                                                                                                      \
    __global__ __launch_bounds__(64) void FWD(const AttnArgs a, const int trim) { attn_fwd_kernel<POLICY, NQT, NKT>(a, trim); }                      \
    template <int NQT, int NKT>                                                                                                                      \
    __global__ __launch_bounds__(64) void BWD(const AttnArgs a, const int trim) { attn_bwd_kernel<POLICY, NQT, NKT>(a, trim); }                      \
    template <int Q0, int K0, int Q1, int K1>                                                                                                        \
    __global__ __launch_bounds__(64) void FWD_PAIR(const AttnArgs a0, const AttnArgs a1, const int n0, const int trim) {                             \
        attn_fwd_pair_kernel<POLICY, Q0, K0, Q1, K1>(a0, a1, n0, trim);                                                                              \
    }                                                                                                                                                \
    template <int Q0, int K0, int Q1, int K1>                                                                                                        \
    __global__ __launch_bounds__(64) void BWD_PAIR(const AttnArgs a0, const AttnArgs a1, const int n0, const int trim) {                             \
        attn_bwd_pair_kernel<POLICY, Q0, K0, Q1, K1>(a0, a1, n0, trim);                                                                              \
    }                                                                                                                                                \
    template <> struct AttnUnit<U> {                                                                                                                 \
        typedef POLICY P;                                                                                                                            \
        template <int NQT, int NKT> static constexpr auto fwd = FWD<NQT, NKT>;                                                                       \
        template <int NQT, int NKT> static constexpr auto bwd = BWD<NQT, NKT>;                                                                       \
        template <int Q0, int K0, int Q1, int K1> static constexpr auto fwd_pair = FWD_PAIR<Q0, K0, Q1, K1>;                                         \
        template <int Q0, int K0, int Q1, int K1> static constexpr auto bwd_pair = BWD_PAIR<Q0, K0, Q1, K1>;                                         \
        static constexpr const char* fwd_name = #FWD; static constexpr const char* bwd_name = #BWD;                                                  \
        static constexpr const char* fwd_pair_name = #FWD_PAIR; static constexpr const char* bwd_pair_name = #BWD_PAIR;                              \
    };                                                                                                                                               \
    template int k_attn_fwd_mfma<U>(const AttnArgs&, hipStream_t);                                                                                   \
    template int k_attn_bwd_mfma<U>(const AttnArgs&, hipStream_t);                                                                                   \
    template int k_attn_fwd_mfma_pair<U>(const AttnArgs&, const AttnArgs&, hipStream_t);                                                             \
    template int k_attn_bwd_mfma_pair<U>(const AttnArgs&, const AttnArgs&, hipStream_t);
