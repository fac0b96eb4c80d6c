// The Shplonk (BDFG20) multiopen prover over Fr for gfx950: the device side of poly/kzg/multiopen/shplonk/prover.rs of
// halo2_proofs (the crate is an unvendored git dependency of the reference: recalled, DESIGN.md section 2 — the yardstick is
// the definition in include/h2agg.h).  Two kernels on top of poly_kernels.hpp; host side: shplonk.inc.
//   wsum:  dst[j] = sum_m w_m p_m[j] - corr[j]        arbitrary weights, corr only below SHPLONK_MAX_SET coefficients
//   leaf:  h[j] (+)= sum_{z in S'} wz_z quot(N, z)[j]  the leaf level of the down-sweep for up to SHPLONK_CHAINS points at once
//
// Why the leaf kernel.  N vanishes on S, so N / Z_S = sum_{z in S} omega_z quot(N, z) with omega_z = 1 / prod_{z' != z}(z - z')
// (partial fractions of 1 / Z_S, times N; the remainders N(z) are 0).  |S| successive divisions read and write the array |S|
// times; here a workgroup reads its chunk of N ONCE (8 coefficients per thread, the geometry of fr_chunk.hpp), runs the
// down-sweep of k_fr_poly_chunk_divide once per point over the same registers, and adds wz_z q_z[j] into 8 accumulators
// that are stored once (wz_z = omega_z v^i: the set's power of v is folded in).  The carries into the chunk, one per point,
// come from the levels above, which are the existing kernels (they are n / T of the work).  A set with more points goes in
// rounds of SHPLONK_CHAINS, each adding into the same destination: the identity is a sum.
//
// Number forms, as poly_kernels.hpp: weights and powers of z arrive in Montgomery form, canonical (< 1 in units of r);
// coefficients and running values are plain residues.  fp_mul(aM, b) < a b / 169 + 1.
//   wsum  a coefficient x < 1 (a larger one raises FLAG_NONCANONICAL and the result is discarded): the product < 1.007 is
//         reduced by one fp_cond_sub to < 1 BEFORE it is added, and the sum acc + product < 2 by one more: acc < 1 after every
//         term, however long the list.  One product is summed per conditional subtraction.  -corr[j] is a canonical
//         residue from the host: acc + (-corr) < 2 -> one fp_cond_sub -> canonical.  Stored values are canonical.
//   leaf  per point the Horner chain is k_fr_poly_chunk_divide's: h < 1.07 (poly_kernels.hpp).  acc[e] starts at 0 and takes
//         fr_poly_step(wzM, h, acc[e]) = fp_cond_sub(wz h + acc[e]) < acc[e] + 0.007 (when acc[e] >= 1; < 1.007 otherwise) once
//         per point: after SHPLONK_CHAINS = 4 products, acc[e] < 1.03.  The store adds the old h[j] < 1 (canonical: ours):
//         < 2.03 -> fp_cond_sub -> < 1.03 -> fp_cond_sub -> canonical.  Without accumulation: < 1.03 -> one fp_cond_sub.
//
// Registers: 8 coefficients and 8 accumulators of 9 limbs live across the loop over the points (144 VGPRs), plus one chain's
// state; one wave per SIMD (256 threads per workgroup, as the other chunk kernels) has 512 to give: no scratch
// (tools/kernel_resources.py --check).  The loop over the points stays rolled; x[] and acc[] are only indexed by template
// constants inside it.
//
// These kernels serve synchronous entry points: the list of wsum and its weights live in a per-call device buffer that the
// call fills and keeps until it has synchronised (the by-value rule of poly_kernels.hpp is for queued calls); the leaf
// kernel's points and weights come by value all the same (they are few).
#pragma once
#include "poly_kernels.hpp"

namespace h2agg {

constexpr unsigned SHPLONK_CHAINS = 4;     // points per launch of the leaf kernel
constexpr unsigned SHPLONK_MAX_SET = 32;   // points per set, coefficients of a correction

struct FrWsumArgs {
    const uint8_t* polys;     // [rows][n]
    uint8_t* dst;             // [n]; not one of the rows named by idx
    const uint32_t* idx;      // nterms row indices (< rows: the host's)
    const uint32_t* w;        // nterms x 8 words: w_m R mod r, canonical
    const uint32_t* ncorr;    // SHPLONK_MAX_SET x 8 words: -corr[j] mod r, canonical, plain
    uint32_t* flags;
    uint32_t nterms;
    uint32_t n;
};

FP_INLINE Fr fr_load_words(const uint32_t* p) {
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = p[i];
    return fp_unpack<FrParams>(w);
}

// dst[j] = sum_m w_m polys[idx[m]][j] - corr[j].  j < n; idx[m] < rows and nterms >= 1 (checked by the host).
__global__ void __launch_bounds__(BLOCK) k_fr_poly_wsum(const FrWsumArgs a) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= a.n) return;
    Fr acc = Fr::zero();
#pragma unroll 1
    for (uint32_t m = 0; m < a.nterms; ++m) {
        const Fr x = fp_load<FrParams>(a.polys + 32 * ((size_t)a.idx[m] * a.n + j));
        if (!fp_is_canonical<FrParams>(x)) atomicOr(a.flags, FLAG_NONCANONICAL);
        const Fr p = fp_cond_sub<FrParams>(fp_mul<FrParams>(fr_load_words(a.w + 8 * m), x));
        acc = fp_cond_sub<FrParams>(fp_add<FrParams>(acc, p));
    }
    if (j < SHPLONK_MAX_SET) acc = fp_cond_sub<FrParams>(fp_add<FrParams>(acc, fr_load_words(a.ncorr + 8 * j)));
    fp_store<FrParams>(a.dst + 32 * (size_t)j, acc);
}

struct FrShplonkLeafArgs {
    FrPolyPoint pt[SHPLONK_CHAINS];   // the points of this round (level 0: b = z)
    uint32_t wz[SHPLONK_CHAINS][8];   // omega_z v^i, R mod r, canonical
    const uint8_t* src;      // N, [n]
    uint8_t* dst;            // h, [n]; not src
    const uint8_t* carry;    // the quotient of level 1, [query][chunks]; null when the array is one chunk (carry 0)
    uint32_t q0;             // the query (row of `carry`) of this round's first point
    uint32_t npts;           // 1 .. SHPLONK_CHAINS
    uint32_t n;
    uint32_t chunks;         // ceil(n / T) = the grid
    uint32_t t;
    uint32_t accumulate;     // 0: dst is written; 1: dst += the sum
};

//   acc[e] += wz h, h -> z h + x[e], for e = E .. 0  (the walk of fr_poly_emit, the store replaced by the weighted sum)
template <int E>
FP_INLINE void fr_shplonk_emit(const Fr& zM, const Fr& wzM, const Fr (&x)[FR_CHUNK_PER], Fr& h, Fr (&acc)[FR_CHUNK_PER]) {
    if constexpr (E >= 0) {
        acc[E] = fr_poly_step(wzM, h, acc[E]);
        if constexpr (E > 0) h = fr_poly_step(zM, h, x[E]);
        fr_shplonk_emit<E - 1>(zM, wzM, x, h, acc);
    }
}
//   the store: dst[i0 + e] for e = E .. 0, below n only
template <int E>
FP_INLINE void fr_shplonk_store(const Fr (&acc)[FR_CHUNK_PER], uint8_t* dst, uint32_t i0, uint32_t n, bool accumulate) {
    if constexpr (E >= 0) {
        if (i0 + E < n) {
            uint8_t* p = dst + 32 * (size_t)(i0 + E);
            Fr v = acc[E];
            if (accumulate) v = fp_cond_sub<FrParams>(fp_add<FrParams>(v, fp_load<FrParams>(p)));
            fp_store<FrParams>(p, fp_cond_sub<FrParams>(v));
        }
        fr_shplonk_store<E - 1>(acc, dst, i0, n, accumulate);
    }
}

// Indices: a thread reads src[i] and reads / writes dst[i] for i in [cT + 8 tid, cT + 8 tid + 8) with i < n only, every
// thread its own 8; carry[(q0 + s) * chunks + c] with s < npts and c < chunks (the level above has (q0 + npts) * chunks
// entries at least: the host's plan); LDS entries < T / 8 <= 256.  npts and t are uniform: every barrier is reached by the
// whole workgroup.
__global__ void __launch_bounds__(FR_CHUNK_THREADS) k_fr_shplonk_leaf(const FrShplonkLeafArgs a) {
    __shared__ uint32_t lds[NL * FR_CHUNK_THREADS];
    const auto [nthr, tid, c, i0] = fr_chunk(a.t, blockIdx.x);
    const bool active = tid < nthr;
    Fr x[FR_CHUNK_PER], acc[FR_CHUNK_PER];
#pragma unroll
    for (int e = 0; e < (int)FR_CHUNK_PER; ++e) {
        x[e] = Fr::zero();
        acc[e] = Fr::zero();
        if (active && i0 + e < a.n) x[e] = fp_load<FrParams>(a.src + 32 * (size_t)(i0 + e));   // canonical: ours (k_fr_poly_wsum)
    }
#pragma unroll 1
    for (uint32_t s = 0; s < a.npts; ++s) {
        const Fr zM = fp_unpack<FrParams>(a.pt[s].pw[0]);
        const Fr cin = a.carry ? fp_load<FrParams>(a.carry + 32 * ((size_t)(a.q0 + s) * a.chunks + c)) : Fr::zero();
        Fr sfx = x[FR_CHUNK_PER - 1];   // as k_fr_poly_chunk_divide: sum_e x[e] z^e, then the inclusive suffix sum over the threads
        fr_poly_fold<(int)FR_CHUNK_PER - 2>(zM, x, sfx);
        if (tid == nthr - 1) sfx = fr_poly_step(fp_unpack<FrParams>(a.pt[s].pw[FR_CHUNK_PER_LOG]), cin, sfx);
        fr_fft_lds_put(lds, tid, sfx);
        __syncthreads();
#pragma unroll 1
        for (uint32_t j = 0; j + FR_CHUNK_PER_LOG < a.t; ++j) {
            const uint32_t stride = 1u << j;
            const bool has = tid + stride < nthr;
            Fr o = Fr::zero();
            if (has) o = fr_fft_lds_get(lds, tid + stride);
            __syncthreads();
            if (has) {
                sfx = fr_poly_step(fp_unpack<FrParams>(a.pt[s].pw[j + FR_CHUNK_PER_LOG]), o, sfx);
                fr_fft_lds_put(lds, tid, sfx);
            }
            __syncthreads();
        }
        Fr h = cin;   // what is above this thread's coefficients: the next thread's inclusive sum, or the chunk's carry-in
        if (tid + 1 < nthr) h = fr_fft_lds_get(lds, tid + 1);
        __syncthreads();   // the next point's first put is behind every read of this one
        fr_shplonk_emit<(int)FR_CHUNK_PER - 1>(zM, fp_unpack<FrParams>(a.wz[s]), x, h, acc);
    }
    if (active) fr_shplonk_store<(int)FR_CHUNK_PER - 1>(acc, a.dst, i0, a.n, a.accumulate != 0);
}

}  // namespace h2agg
