// Discrete Fourier transform over G1 for gfx950, and the scalars of a KZG setup: the device side of
//   ParamsKZG::setup / g_to_lagrange / downsize   (halo2_proofs poly/kzg/commitment.rs and arithmetic.rs; the crate is an
//                                                  unvendored git dependency of the reference: recalled)
// out[i] = sum_j w^(i*j) * in[j] over points: a radix-2 decimation-in-time transform.  The input is scattered to bit-reversed
// positions (k_g1_fft_load), then stage s = 1 .. k combines blocks of 2^(s-1) points with the butterfly
// (a, b) -> (a + t*b, a - t*b), t = w^(j * 2^(k-s)) for position j inside the block.  The scalar multiplication t*b is all
// the work (128 doublings and ~60 additions against the butterfly's two additions), so the stage kernel is the windowed
// ladder of scalar_mul_kernels.hpp — GLV halves, signed window-4 digits, 1P .. 8P in LDS, four lanes per point — with two
// changes an FFT allows:
//   * the digits of a twiddle are not decoded in the kernel: stage s has only 2^(s-1) twiddles, all of them powers of one
//     root, so their digit records are made once per (k, direction) and kept in the context (k_fft_twiddle_digits);
//   * a stage with >= FFT_UNIFORM_MIN butterflies per twiddle gives every workgroup butterflies of ONE twiddle: the record
//     index is wave-uniform, the digit words arrive through the scalar unit and the "digit is zero" / "which table entry"
//     decisions are the same for every lane.  Later stages read one record per group of four lanes.
// Butterflies whose twiddle is 1 (all of stage 1, position 0 of every block) multiply nothing.  The 1/n of the inverse
// transform is one more multiplication per point with ONE scalar for the whole array: it is done where the points are
// loaded (k_g1_fft_load), through the wave-uniform path.
// Stages are NOT fused through LDS: the multiplications are > 99 % of the work, k launches and one HBM round trip of
// 144 B / point per stage cost nothing next to them.
// Every addition goes through xyzz_add_par4 / xyzz_double_par4, which handle a == t*b (doubling), a == -t*b (identity)
// and identity operands explicitly.
#pragma once
#include "scalar_mul_kernels.hpp"

namespace h2agg {

// One scalar as the ladder reads it, 16 words: [0..4] magnitudes of the 33 window-4 digits of |k1| (4 bits each),
// [5..9] the same for |k2|, [10..11] bit j set: digit j of k1 subtracts (the half's sign already folded in),
// [12..13] the same for k2, [14..15] unused.
constexpr int FFT_REC_WORDS = 16;
constexpr uint32_t FFT_UNIFORM_MIN = 64;    // butterflies per twiddle from which a workgroup (32 butterflies) has one twiddle
constexpr unsigned FFT_MAX_K = 24;
constexpr int FRP_CHUNK = 16;               // consecutive exponents per thread of k_fr_affine_powers
constexpr int FRP_TABLE = 25;               // base^(2^j), j < 25: exponents below 2^25

// out[i] = A * base^i + B (canonical), i < n.  cst: base^(2^j) for j < FRP_TABLE, then A, then B, 32-byte canonical each.
// One thread per FRP_CHUNK consecutive exponents: base^(first) from the table, then one multiplication per element.
// The scalars of ParamsKZG::setup: s^i (A = 1, B = 0), and the denominators (s * w^-i - 1) / c of L_i(s).
__global__ void __launch_bounds__(BLOCK) k_fr_affine_powers(const uint8_t* __restrict__ cst, size_t n, uint8_t* __restrict__ out) {
    const size_t i0 = ((size_t)blockIdx.x * BLOCK + threadIdx.x) * FRP_CHUNK;
    if (i0 >= n) return;
    Fr cur = Fr::one();
#pragma unroll 1
    for (int j = 0; j < FRP_TABLE; ++j)
        if ((i0 >> j) & 1) cur = fp_mul<FrParams>(cur, fp_to_mont<FrParams>(fp_load<FrParams>(cst + 32 * j)));
    const Fr base = fp_to_mont<FrParams>(fp_load<FrParams>(cst));
    const Fr a = fp_load<FrParams>(cst + 32 * FRP_TABLE), b = fp_load<FrParams>(cst + 32 * (FRP_TABLE + 1));
#pragma unroll 1
    for (int e = 0; e < FRP_CHUNK && i0 + e < n; ++e) {
        const Fr v = fp_cond_sub<FrParams>(fp_mul<FrParams>(cur, a));   // (x R) * A / R = x * A
        fp_store<FrParams>(out + 32 * (i0 + e), fp_cond_sub<FrParams>(fp_add<FrParams>(v, b)));
        cur = fp_mul<FrParams>(cur, base);
    }
}

// canonical scalars -> ladder records (see FFT_REC_WORDS)
__global__ void __launch_bounds__(BLOCK) k_fft_twiddle_digits(const uint8_t* __restrict__ scalars, size_t n,
                                                              uint32_t* __restrict__ rec, uint32_t* flags) {
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * BLOCK) {
        const U256 s = u256_load(scalars + 32 * i);
        U256 d;
        if (!u256_is_canonical_fr(s) | !glv_decompose(s, d)) atomicOr(flags, FLAG_NONCANONICAL);
        const uint32_t m1[4] = {d.w[0], d.w[1], d.w[2], d.w[3] & 0x7fffffffu};
        const uint32_t m2[4] = {d.w[4], d.w[5], d.w[6], d.w[7] & 0x7fffffffu};
        const W4Digits d1 = w4_recode(m1), d2 = w4_recode(m2);
        const uint64_t all = ((uint64_t)1 << 33) - 1;
        const uint64_t n1 = d1.neg ^ ((d.w[3] >> 31) ? all : 0), n2 = d2.neg ^ ((d.w[7] >> 31) ? all : 0);
        uint4* o = reinterpret_cast<uint4*>(rec + FFT_REC_WORDS * i);
        o[0] = make_uint4(d1.mag[0], d1.mag[1], d1.mag[2], d1.mag[3]);
        o[1] = make_uint4(d1.mag[4], d2.mag[0], d2.mag[1], d2.mag[2]);
        o[2] = make_uint4(d2.mag[3], d2.mag[4], (uint32_t)n1, (uint32_t)(n1 >> 32));
        o[3] = make_uint4((uint32_t)n2, (uint32_t)(n2 >> 32), 0u, 0u);
    }
}

// (scalar of `rec`) * base, base replicated in the four lanes of a group; `tab` is the workgroup's table area.
// UNIFORM: every lane of the wave has the same `rec`.
template <bool UNIFORM>
FP_INLINE G1XYZZ fft_scalar_mul_par4(const G1XYZZ& base, const uint32_t* __restrict__ rec, uint32_t* tab) {
    if (base.is_identity()) return base;
    const int g = threadIdx.x >> 2;
    G1XYZZ t = base;
    if ((threadIdx.x & 3) == 0) sm_tab_put(tab, g, 0, t);
    t = xyzz_double_par4(t);
    if ((threadIdx.x & 3) == 0) sm_tab_put(tab, g, 1, t);
#pragma unroll 1
    for (int e = 2; e < SM_TABLE; ++e) {
        t = xyzz_add_par4(t, base);
        if ((threadIdx.x & 3) == 0) sm_tab_put(tab, g, e, t);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();     // the four lanes of a group are in one wave: the table is visible to them
    const Fq beta = fq_beta();
    uint32_t n1lo = rec[10], n1hi = rec[11], n2lo = rec[12], n2hi = rec[13];
    if (UNIFORM) {
        n1lo = __builtin_amdgcn_readfirstlane(n1lo);
        n1hi = __builtin_amdgcn_readfirstlane(n1hi);
        n2lo = __builtin_amdgcn_readfirstlane(n2lo);
        n2hi = __builtin_amdgcn_readfirstlane(n2hi);
    }
    const uint64_t neg1 = ((uint64_t)n1hi << 32) | n1lo, neg2 = ((uint64_t)n2hi << 32) | n2lo;
    G1XYZZ acc = G1XYZZ::identity();
#pragma unroll 1
    for (int j = 32; j >= 0; --j) {
        if (j != 32) {
#pragma unroll 1
            for (int k = 0; k < 4; ++k) acc = xyzz_double_par4(acc);
        }
        uint32_t a1 = (rec[j >> 3] >> (4 * (j & 7))) & 15u, a2 = (rec[5 + (j >> 3)] >> (4 * (j & 7))) & 15u;
        if (UNIFORM) {
            a1 = __builtin_amdgcn_readfirstlane(a1);
            a2 = __builtin_amdgcn_readfirstlane(a2);
        }
        if (a1) {
            G1XYZZ q = sm_tab_get(tab, g, (int)a1 - 1);
            if ((neg1 >> j) & 1u) q.y = fp_neg<4, FqParams>(q.y);
            acc = xyzz_add_par4(acc, q);
        }
        if (a2) {
            G1XYZZ q = sm_tab_get(tab, g, (int)a2 - 1);
            q.x = FQ_MUL(q.x, beta);                                  // phi: X -> beta * X  (8 * 1 / 169 + 1 -> [2])
            if ((neg2 >> j) & 1u) q.y = fp_neg<4, FqParams>(q.y);
            acc = xyzz_add_par4(acc, q);
        }
    }
    return acc;
}

// work[bitrev_k(i)] = scale * table[i], i < 2^k (XYZZ).  scale_rec == nullptr: no multiplication (the forward transform,
// and n = 1).  One group of four lanes per point; one round per workgroup.
__global__ void __launch_bounds__(SM_THREADS) k_g1_fft_load(const uint8_t* __restrict__ table, uint32_t k,
                                                            const uint32_t* __restrict__ scale_rec, uint8_t* __restrict__ work) {
    __shared__ uint32_t tab[SM_TABLE * XYZZ_WORDS * SM_GROUPS];
    const uint32_t n = 1u << k;
    const uint32_t i = blockIdx.x * SM_GROUPS + (threadIdx.x >> 2);
    const bool live = i < n;
    const uint32_t ii = live ? i : n - 1;
    G1XYZZ p = G1XYZZ::from_affine(affine_load(table + 64 * (size_t)ii));
    if (scale_rec) p = fft_scalar_mul_par4<true>(p, scale_rec, tab);
    const uint32_t dst = k ? __brev(ii) >> (32 - k) : 0u;
    if (live && (threadIdx.x & 3) == 0) xyzz_store(work + XYZZ_BYTES * (size_t)dst, p);
}

// Stage s (1 .. k) of the transform of 2^k points, in place.  Butterfly q < 2^(k-1): position j = q >> (k - s) inside its
// block, block q & (2^(k-s) - 1) — butterflies with the same twiddle are consecutive, so with 2^(k-s) >= FFT_UNIFORM_MIN a
// workgroup's 32 butterflies share one.  tw: records of w^t, t < 2^(K-1), for the K the context holds; tw_shift = K - k.
template <bool UNIFORM>
__global__ void __launch_bounds__(SM_THREADS) k_g1_fft_stage(uint8_t* __restrict__ work, uint32_t k, uint32_t s,
                                                             const uint32_t* __restrict__ tw, uint32_t tw_shift) {
    __shared__ uint32_t tab[SM_TABLE * XYZZ_WORDS * SM_GROUPS];
    const uint32_t half_n = 1u << (k - 1);
    const uint32_t q = blockIdx.x * SM_GROUPS + (threadIdx.x >> 2);
    const bool live = q < half_n;
    const uint32_t qq = live ? q : half_n - 1;
    const uint32_t sh = k - s;
    uint32_t j = qq >> sh;
    if (UNIFORM) j = __builtin_amdgcn_readfirstlane(j);
    const uint32_t blk = qq & ((1u << sh) - 1u);
    const size_t ia = ((size_t)blk << s) + j, ib = ia + ((size_t)1 << (s - 1));
    const G1XYZZ a = xyzz_load(work + XYZZ_BYTES * ia);
    G1XYZZ tb = xyzz_load(work + XYZZ_BYTES * ib);
    if (j) tb = fft_scalar_mul_par4<UNIFORM>(tb, tw + (size_t)FFT_REC_WORDS * ((size_t)(j << sh) << tw_shift), tab);
    const G1XYZZ lo = xyzz_add_par4(a, tb), hi = xyzz_add_par4(a, xyzz_neg(tb));
    if (live && (threadIdx.x & 3) == 0) {
        xyzz_store(work + XYZZ_BYTES * ia, lo);
        xyzz_store(work + XYZZ_BYTES * ib, hi);
    }
}

// XYZZ work array -> canonical Jacobian (what the batch-inversion kernel k_jac_to_mont_affine takes)
__global__ void __launch_bounds__(BLOCK) k_g1_fft_to_jac(const uint8_t* __restrict__ work, size_t n, uint8_t* __restrict__ out_jac) {
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * BLOCK)
        jac_store_canonical(out_jac + 96 * i, jac_from_xyzz(xyzz_load(work + XYZZ_BYTES * i)));
}

}  // namespace h2agg
