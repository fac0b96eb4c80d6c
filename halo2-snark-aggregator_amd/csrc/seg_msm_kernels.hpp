// Segmented multi_exp: S independent MSMs over the disjoint, contiguous segments [seg_start[s], seg_start[s + 1]) of one
// point / scalar array, in one set of launches (h2agg_g1_msm_segmented; the 2N evaluation sides of h2agg_verify_proofs).
//
// The segments here are small and uneven (tens to a few hundred points: one side of evaluate_multiopen_proof), where the
// whole-array MSM's plan — windows sized for the total, a sort over every (MSM, window) — spends its time reducing buckets
// that hold one point or none.  Shape: one workgroup per (segment, window), one lane per bucket (C-bit unsigned digits,
// 2^C - 1 buckets); the workgroup counting-sorts its segment's digits in LDS, every lane adds its bucket's points (mixed
// additions, all lanes in step), weights its bucket by its digit (double-and-add over C bits), and the workgroup sums the
// weighted buckets; one wave per segment then does the Horner chain over the W window sums (k_msm_final_lp).
#pragma once
#include "batch_kernels.hpp"

namespace h2agg {

constexpr uint32_t SEG_MAX_LEN = 16384;   // longest segment the window kernel takes (16-bit indices in LDS); longer: msm_run

template <int C>
struct SegCfg {
    static constexpr int NB = 1 << C;               // digit values 0 .. NB - 1 (digit 0: no bucket)
    static constexpr int T = NB < 64 ? 64 : NB;      // lanes: one per bucket, at least one wave
};

// dynamic LDS of k_seg_window<C> for segments of at most maxlen points: the sort (counts, cursors, 16-bit indices), then the
// workgroup sum (XYZZ_WORDS words per lane) in the same bytes
template <int C>
inline size_t seg_window_lds(uint32_t maxlen) {
    const size_t sort = 4 * (size_t)(2 * SegCfg<C>::NB) + 2 * (size_t)maxlen + 4;
    const size_t red = 4 * (size_t)XYZZ_WORDS * SegCfg<C>::T;
    return sort > red ? sort : red;
}

// the C-bit digit of a canonical scalar (8 little-endian words) at bit `bit`
template <int C>
FP_INLINE uint32_t seg_digit(const uint8_t* scalar, uint32_t bit) {
    const uint32_t* k = reinterpret_cast<const uint32_t*>(scalar);
    const uint32_t wd = bit >> 5, sh = bit & 31;
    uint32_t v = k[wd] >> sh;
    if (sh + C > 32 && wd < 7) v |= k[wd + 1] << (32 - sh);
    return v & ((1u << C) - 1);
}

template <int T>
FP_INLINE void seg_lds_put(uint32_t* lds, int tid, const G1XYZZ& p) {
#pragma unroll
    for (int k = 0; k < NL; ++k) {
        lds[k * T + tid] = p.x.l[k];
        lds[(NL + k) * T + tid] = p.y.l[k];
        lds[(2 * NL + k) * T + tid] = p.zz.l[k];
        lds[(3 * NL + k) * T + tid] = p.zzz.l[k];
    }
}
template <int T>
FP_INLINE G1XYZZ seg_lds_get(const uint32_t* lds, int tid) {
    G1XYZZ p;
#pragma unroll
    for (int k = 0; k < NL; ++k) {
        p.x.l[k] = lds[k * T + tid];
        p.y.l[k] = lds[(NL + k) * T + tid];
        p.zz.l[k] = lds[(2 * NL + k) * T + tid];
        p.zzz.l[k] = lds[(3 * NL + k) * T + tid];
    }
    return p;
}

// grid (W, segments of this launch): wsum[(blockIdx.y * W + w)] = sum_b b * (sum of the points of segment first_seg +
// blockIdx.y whose digit w is b).  bases: Montgomery affine; scalars: canonical; seg_start: absolute offsets.
template <int C>
__global__ void __launch_bounds__(SegCfg<C>::T) k_seg_window(const uint8_t* __restrict__ bases,
                                                            const uint8_t* __restrict__ scalars,
                                                            const uint32_t* __restrict__ seg_start, uint32_t first_seg,
                                                            int W, uint8_t* __restrict__ wsum) {
    constexpr int NB = SegCfg<C>::NB, T = SegCfg<C>::T;
    extern __shared__ uint32_t seg_lds[];
    uint32_t* cnt = seg_lds;          // NB
    uint32_t* pos = seg_lds + NB;     // NB
    uint16_t* idx = reinterpret_cast<uint16_t*>(seg_lds + 2 * NB);
    const uint32_t w = blockIdx.x, s = first_seg + blockIdx.y;
    const uint32_t beg = seg_start[s], len = seg_start[s + 1] - beg;
    const int tid = threadIdx.x;
    const uint32_t bit = w * C;
    const uint8_t* sc = scalars + 32 * (size_t)beg;
    for (int b = tid; b < NB; b += T) cnt[b] = 0;
    __syncthreads();
    for (uint32_t i = tid; i < len; i += T) {
        const uint32_t d = seg_digit<C>(sc + 32 * (size_t)i, bit);
        if (d) atomicAdd(&cnt[d], 1u);
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (int b = 0; b < NB; ++b) {
            pos[b] = run;
            run += cnt[b];
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < len; i += T) {
        const uint32_t d = seg_digit<C>(sc + 32 * (size_t)i, bit);
        if (d) idx[atomicAdd(&pos[d], 1u)] = (uint16_t)i;
    }
    __syncthreads();
    // pos[b] is the end of bucket b now, pos[b] - cnt[b] its start
    G1XYZZ acc = G1XYZZ::identity();
    const uint8_t* bs = bases + 64 * (size_t)beg;
    if (tid > 0 && tid < NB) {
        const uint32_t e = pos[tid];
#pragma unroll 1
        for (uint32_t k = e - cnt[tid]; k < e; ++k) xyzz_add_affine(acc, affine_load(bs + 64 * (size_t)idx[k]));
    }
    // bucket b weighs b: double-and-add over the C bits of b
    G1XYZZ r = G1XYZZ::identity();
    if (tid > 0 && tid < NB && !acc.is_identity()) {
#pragma unroll 1
        for (int j = C - 1; j >= 0; --j) {
            r = xyzz_double(r);
            if ((tid >> j) & 1) r = xyzz_add(r, acc);
        }
    }
    __syncthreads();   // (the sort's bytes are free: the workgroup sum reuses them)
    seg_lds_put<T>(seg_lds, tid, r);
    __syncthreads();
#pragma unroll 1
    for (int h = T / 2; h >= 1; h >>= 1) {
        if (tid < h) {
            r = xyzz_add(r, seg_lds_get<T>(seg_lds, tid + h));
            seg_lds_put<T>(seg_lds, tid, r);
        }
        __syncthreads();
    }
    if (tid == 0) xyzz_store(wsum + XYZZ_BYTES * ((size_t)blockIdx.y * W + w), r);
}

// the evaluation sides' tail (evaluation.rs:198-200, verify.rs:730-731), S sides in one launch (one wave each):
// out[128 s] = (X, Y, ZZ, ZZZ) of  msm_jac[s] + the side's scalar-less points pns[pns_start[s] .. pns_start[s + 1]),
// canonical integers — the host divides, with one field inversion for every side (Montgomery's trick)
__global__ void __launch_bounds__(64) k_seg_tail(const uint8_t* __restrict__ msm_jac, const uint8_t* __restrict__ pns,
                                                 const uint32_t* __restrict__ pns_start, uint8_t* __restrict__ out,
                                                 uint32_t* flags) {
    if (threadIdx.x != 0) return;
    const uint32_t s = blockIdx.x;
    G1XYZZ acc = xyzz_from_jac(jac_load_canonical(msm_jac + 96 * (size_t)s));
    uint32_t bad = 0;
#pragma unroll 1
    for (uint32_t i = pns_start[s]; i < pns_start[s + 1]; ++i) xyzz_add_affine(acc, affine_load_canonical(pns + 64 * (size_t)i, bad));
    if (bad) atomicOr(flags, FLAG_NONCANONICAL);
    uint8_t* o = out + 128 * (size_t)s;
    fp_store<FqParams>(o, fp_from_mont<FqParams>(acc.x));
    fp_store<FqParams>(o + 32, fp_from_mont<FqParams>(acc.y));
    fp_store<FqParams>(o + 64, fp_from_mont<FqParams>(acc.zz));
    fp_store<FqParams>(o + 96, fp_from_mont<FqParams>(acc.zzz));
}

}  // namespace h2agg
