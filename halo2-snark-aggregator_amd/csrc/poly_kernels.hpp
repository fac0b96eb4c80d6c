// KZG openings over Fr for gfx950: the device side of
//   eval_polynomial / kate_division (halo2_proofs arithmetic.rs) and the linear combination of the GWC multiopen prover
//   (poly/kzg/multiopen/gwc/prover.rs; the crate is an unvendored git dependency of the reference: recalled, DESIGN.md
//    section 2 — the yardstick is the definition in include/h2agg.h)
//   eval:    a(z) = sum_i a[i] z^i
//   divide:  q[j] = sum_{i > j} a[i] z^(i-j-1), j < n (q[n-1] = 0);  rem = a(z)
//   lincomb: c[j] = sum_m v^m p_m[j]
// n = 2^k coefficients, low degree first, canonical 32-byte little-endian in and out.
//
// Plan.  The array is cut into chunks of T = 2^t coefficients, one workgroup each, 8 consecutive coefficients per thread
// (the geometry of fr_chunk.hpp; the levels: fr_level_plan, fr_host.inc).
//   up-sweep   k_fr_poly_chunk_eval:    E[c] = sum_{i in chunk c} a[i] z^(i - cT).  E is a polynomial in z^T with ceil(n / T)
//              coefficients, so the same kernel evaluates it: 2^24 -> 2^13 -> 2^2 -> 1.  The top value is a(z).
//   down-sweep k_fr_poly_chunk_divide:  the carry into chunk c, sum_{i >= (c+1)T} a[i] z^(i - (c+1)T), is quot(E, z^T)[c]: the
//              levels are divided top down with the same kernel, each level's quotient the carries of the one below.
// A query is one (polynomial, point) pair; all queries of a call go through one launch per level (blockIdx.x = query *
// chunks + chunk).
//
// Number forms.  z^e (and v) arrive in Montgomery form, z^e R mod r, canonical; coefficients and running values are plain
// residues, so fp_mul(zM, h) = z h with no conversion anywhere.  Bounds, in units of r: zM < 1, a coefficient x < 1 (a
// non-canonical one, < 2^256 < 5.3, raises FLAG_NONCANONICAL and the result is discarded), a running value h < 1.1:
//   product  fp_mul(zM, h) < 1 * 1.1 / 169 + 1 < 1.007  (< 2r);
//   Horner   fp_cond_sub(product + x) < max(1, 1.007 + 1 - 1) = 1.007:  one conditional subtraction of r after the add;
//   tree / scan levels add two running values: fp_cond_sub(product + h) < h + 0.007, at most 9 times in a row (8 levels
//   and the carry fold) from 1.007: < 1.07.  The Horner that follows is back under 1.007 after its first step.
// Every stored value goes through one more fp_cond_sub: < 2 -> canonical.
//
// The powers z^(2^j) come from the host BY VALUE in the kernel arguments (FrPolyPoint, FR_POLY_POINTS points per launch): a
// device block that a host copy fills could be rewritten by a second queued call before the first one's launch has read
// it (fr_fft_kernels.hpp has the same rule).  A launch handles the queries whose point is one of its FR_POLY_POINTS; the
// workgroups of other queries return at once.  The host passes only points that a query names (poly_open.inc).
#pragma once
#include "fr_chunk.hpp"

namespace h2agg {

constexpr unsigned FR_POLY_POINTS = 8;       // points per launch (their power tables fill 2.8 KiB of kernel arguments)

struct FrPolyPoint {
    uint32_t pw[FR_CHUNK_LOG][8];   // (b^(2^j)) R mod r, canonical, j <= min(t, 10); b = z^(T^level)
};

struct FrPolyArgs {
    FrPolyPoint pt[FR_POLY_POINTS];   // the points pt0 .. pt0 + 7
    const uint8_t* src;     // level 0: the slab of polynomials; above: E of this level, [query][n]
    uint8_t* dst;           // eval: E of the next level, [query][chunks]; divide: the quotient, [query][n]
    const uint8_t* carry;   // divide: the quotient of the level above, [query][chunks]; null at the top (carry 0)
    const uint32_t* desc;   // {polynomial, point} per query; null: query q is polynomial q at point q
    uint32_t* flags;
    uint32_t n;             // coefficients per query at this level
    uint32_t chunks;        // ceil(n / T)
    uint32_t t;             // log2 T, FR_CHUNK_PER_LOG .. FR_CHUNK_LOG
    uint32_t pt0;
    uint32_t level0;        // src is the caller's slab: polynomials by desc, coefficients checked for < r
};

FP_INLINE Fr fr_poly_pw(const FrPolyArgs& a, uint32_t slot, uint32_t j) { return fp_unpack<FrParams>(a.pt[slot].pw[j]); }

// z h + x with one conditional subtraction;  zM < 1, h < 1.1:  x < 1 -> < 1.007,  x < X -> < X + 0.007  (file header)
FP_INLINE Fr fr_poly_step(const Fr& zM, const Fr& h, const Fr& x) {
    return fp_cond_sub<FrParams>(fp_add<FrParams>(fp_mul<FrParams>(zM, h), x));
}

// The two per-thread sweeps of the down-sweep over the coefficients x[0..8) held in registers.  Written as recursive templates:
// with the field product inlined a loop body is too large for the compiler to unroll on request, and a loop that stays
// rolled indexes x[] dynamically, which would put it into scratch memory.
//   fold: s -> (..(s z + x[E]) z + ..) z + x[0]
template <int E>
FP_INLINE void fr_poly_fold(const Fr& zM, const Fr (&x)[FR_CHUNK_PER], Fr& s) {
    if constexpr (E >= 0) {
        s = fr_poly_step(zM, s, x[E]);
        fr_poly_fold<E - 1>(zM, x, s);
    }
}
//   emit: q[i0 + e] = h, h -> z h + x[e], for e = E .. 0; stores only below n.  h < 1.1 -> one fp_cond_sub -> canonical
template <int E>
FP_INLINE void fr_poly_emit(const Fr& zM, const Fr (&x)[FR_CHUNK_PER], Fr& h, uint8_t* dst, uint32_t i0, uint32_t n) {
    if constexpr (E >= 0) {
        if (i0 + E < n) fp_store<FrParams>(dst + 32 * (size_t)(i0 + E), fp_cond_sub<FrParams>(h));
        if constexpr (E > 0) h = fr_poly_step(zM, h, x[E]);
        fr_poly_emit<E - 1>(zM, x, h, dst, i0, n);
    }
}

// query, chunk and point slot of this workgroup; false: the query's point is not in this launch
FP_INLINE bool fr_poly_locate(const FrPolyArgs& a, uint32_t& q, uint32_t& c, uint32_t& slot, const uint8_t*& src) {
    q = blockIdx.x / a.chunks;
    c = blockIdx.x - q * a.chunks;
    slot = (a.desc ? a.desc[2 * q + 1] : q) - a.pt0;
    const uint32_t poly = a.desc && a.level0 ? a.desc[2 * q] : q;
    src = a.src + 32 * (size_t)poly * a.n;
    return slot < FR_POLY_POINTS;
}

// Up-sweep.  Indices: a thread reads src[poly * n + i] for i in [cT + 8 tid, cT + 8 tid + 8) with i < n only (poly < the
// slab's polynomial count: checked by the host), LDS entries < T / 8 <= 256, and thread 0 stores dst[q * chunks + c].
__global__ void __launch_bounds__(FR_CHUNK_THREADS) k_fr_poly_chunk_eval(const FrPolyArgs a) {
    __shared__ uint32_t lds[NL * FR_CHUNK_THREADS];
    uint32_t q, chunk, slot;
    const uint8_t* src;
    if (!fr_poly_locate(a, q, chunk, slot, src)) return;   // uniform over the workgroup: in front of every barrier
    const auto [nthr, tid, c, i0] = fr_chunk(a.t, chunk);
    const Fr zM = fr_poly_pw(a, slot, 0);
    Fr h = Fr::zero();
    if (tid < nthr) {
#pragma unroll
        for (int e = FR_CHUNK_PER - 1; e >= 0; --e) {
            Fr x = Fr::zero();
            if (i0 + e < a.n) {
                x = fp_load<FrParams>(src + 32 * (size_t)(i0 + e));
                if (a.level0 && !fp_is_canonical<FrParams>(x)) atomicOr(a.flags, FLAG_NONCANONICAL);
            }
            h = e == (int)FR_CHUNK_PER - 1 ? x : fr_poly_step(zM, h, x);
        }
    }
    fr_fft_lds_put(lds, tid, h);
    __syncthreads();
    // tree: lo + z^(8 * 2^j) * hi; a level writes only entries it does not read from another thread
#pragma unroll 1
    for (uint32_t j = 0; j + FR_CHUNK_PER_LOG < a.t; ++j) {
        const uint32_t stride = 1u << j;
        if ((tid & (2u * stride - 1u)) == 0 && tid + stride < nthr) {
            h = fr_poly_step(fr_poly_pw(a, slot, j + FR_CHUNK_PER_LOG), fr_fft_lds_get(lds, tid + stride), h);
            fr_fft_lds_put(lds, tid, h);
        }
        __syncthreads();
    }
    if (tid == 0) fp_store<FrParams>(a.dst + 32 * ((size_t)q * a.chunks + c), fp_cond_sub<FrParams>(h));
}

// Down-sweep.  IN PLACE (dst == src) IS SAFE BECAUSE: a workgroup reads only its own chunk of src — every thread its own 8
// coefficients, all of them into registers before its first store — plus one element of `carry`, which is another buffer;
// and it stores only q[j] for j in its own chunk, every thread at the 8 indices it loaded.  No thread reads what another
// one writes, in this workgroup or any other.  Index bounds as in k_fr_poly_chunk_eval; stores have j < n.
__global__ void __launch_bounds__(FR_CHUNK_THREADS) k_fr_poly_chunk_divide(const FrPolyArgs a) {
    __shared__ uint32_t lds[NL * FR_CHUNK_THREADS];
    uint32_t q, chunk, slot;
    const uint8_t* src;
    if (!fr_poly_locate(a, q, chunk, slot, src)) return;
    const auto [nthr, tid, c, i0] = fr_chunk(a.t, chunk);
    const Fr zM = fr_poly_pw(a, slot, 0);
    const Fr cin = a.carry ? fp_load<FrParams>(a.carry + 32 * ((size_t)q * a.chunks + c)) : Fr::zero();   // canonical: ours
    const bool active = tid < nthr;
    Fr x[FR_CHUNK_PER];
#pragma unroll
    for (int e = 0; e < (int)FR_CHUNK_PER; ++e) {
        x[e] = Fr::zero();
        if (active && i0 + e < a.n) x[e] = fp_load<FrParams>(src + 32 * (size_t)(i0 + e));
    }
    Fr s = x[FR_CHUNK_PER - 1];   // sum_e x[e] z^e, then the inclusive suffix sum over the threads at and above this one
    fr_poly_fold<(int)FR_CHUNK_PER - 2>(zM, x, s);
    if (tid == nthr - 1) s = fr_poly_step(fr_poly_pw(a, slot, FR_CHUNK_PER_LOG), cin, s);   // + z^8 * carry-in
    fr_fft_lds_put(lds, tid, s);
    __syncthreads();
    // suffix scan: s[tid] += z^(8 * 2^j) * s[tid + 2^j]; read, barrier, write, barrier
#pragma unroll 1
    for (uint32_t j = 0; j + FR_CHUNK_PER_LOG < a.t; ++j) {
        const uint32_t stride = 1u << j;
        const bool has = tid + stride < nthr;
        Fr o = Fr::zero();
        if (has) o = fr_fft_lds_get(lds, tid + stride);
        __syncthreads();
        if (has) {
            s = fr_poly_step(fr_poly_pw(a, slot, j + FR_CHUNK_PER_LOG), o, s);
            fr_fft_lds_put(lds, tid, s);
        }
        __syncthreads();
    }
    if (tid >= nthr) return;   // (behind the last barrier)
    // what is above this thread's coefficients: the next thread's inclusive sum, or the chunk's carry-in
    Fr h = tid == nthr - 1 ? cin : fr_fft_lds_get(lds, tid + 1);
    uint8_t* dst = a.dst + 32 * (size_t)q * a.n;
    fr_poly_emit<(int)FR_CHUNK_PER - 1>(zM, x, h, dst, i0, a.n);
}

struct FrLincombArgs {
    uint32_t v[8];           // v R mod r, canonical
    const uint8_t* polys;    // [npoly][n]
    uint8_t* dst;            // [groups][n]
    const uint32_t* list;    // polynomial indices, group after group, each group's HIGHEST power of v first
    const uint32_t* goff;    // group g is list[goff[g] .. goff[g + 1]), never empty
    uint32_t* flags;
    uint32_t n;
};

// dst[g][j] = sum_m v^m p_m[j]: Horner in v.  j < n; list entries < npoly (checked by the host).
__global__ void __launch_bounds__(BLOCK) k_fr_poly_lincomb(const FrLincombArgs a) {
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x, g = blockIdx.y;
    if (j >= a.n) return;
    const Fr vM = fp_unpack<FrParams>(a.v);
    const uint32_t b = a.goff[g], e = a.goff[g + 1];
    Fr acc = Fr::zero();
#pragma unroll 1
    for (uint32_t m = b; m < e; ++m) {
        const Fr x = fp_load<FrParams>(a.polys + 32 * ((size_t)a.list[m] * a.n + j));
        if (!fp_is_canonical<FrParams>(x)) atomicOr(a.flags, FLAG_NONCANONICAL);
        acc = m == b ? x : fr_poly_step(vM, acc, x);
    }
    fp_store<FrParams>(a.dst + 32 * ((size_t)g * a.n + j), fp_cond_sub<FrParams>(acc));
}

}  // namespace h2agg
