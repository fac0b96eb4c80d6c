// Grand products over Fr for gfx950: the device side of
//   ff::BatchInvert, permutation::prover::commit, lookup::prover::commit_product
//   (halo2_proofs; the crate is an unvendored git dependency of the reference: recalled, DESIGN.md section 2 — the yardstick
//    is the definition in include/h2agg.h.  Which Z a verifier accepts is pinned: permutation.rs:70-133, lookup.rs:98-113)
//   invert:  out[i] = in[i]^-1, and 0 where in[i] = 0
//   scan:    out[0] = init, out[i + 1] = out[i] * num[i] * inv(den[i]), i < u  (inv(0) = 0)
//   terms:   the num / den columns of one permutation set, or of a lookup
// Canonical 32-byte little-endian in and out.
//
// Plan.  An array is cut into chunks of T = 2^t elements, one workgroup each, 8 consecutive elements per thread in registers
// (the geometry of fr_chunk.hpp; the levels: fr_level_plan, fr_host.inc).  The threads' products are
// combined by a binary tree in LDS: 2 * 256 slots, slot 1 the root, slots 2v and 2v + 1 the children of v, slot nthr + tid
// the leaf of thread tid.
//   up-sweep   k_fr_prod_chunk:   P[c] = the product of chunk c.  The same kernel runs on P, until ONE chunk is left.
//   down-sweep k_fr_prod_invert:  given the inverse of its product (from the level above; the one chunk at the top inverts
//              its own root: the ONE fp_inv of a call, on one lane), a chunk walks the tree down — the inverse of a child
//              is the inverse of the parent times the sibling — and every thread walks its 8 elements back: the inverse
//              of x[e] is (inverse of x[0..e]) * x[0..e-1].  Montgomery's trick on a tree: no inversion per element.
//              Zeros are replaced by 1 where they are loaded, in both sweeps (the down-sweep loads its elements again:
//              "remembered" costs no memory), and get 0.
//   down-sweep k_fr_prod_scan:    given the product of everything in front of its chunk (the level above's exclusive
//              prefix; `init` at the top), a chunk walks the tree down — left child: the parent's prefix, right child:
//              that times the left sibling — and every thread emits prefix, prefix * x[0], ...
// One launch for n <= T, three for n <= T^2 (up, down, down), five above.
//
// Number forms.  fp_mul(a, b) = a b / R.  Under that product the integers mod r form a group with unit R (Fr::one()) whose
// inverse of a is R^2 / a — what fp_inv computes (Montgomery in and out) — so the inversion sweeps take the canonical input
// AS IT IS and convert nothing per element: every value is the inverse, in that group, of a product of inputs, times the
// constant `top` the single root inverse is multiplied with.  top = 1 / R makes the outputs 1 / x (h2agg_fr_batch_invert);
// top = R leaves R^2 / x, which the scan wants: fp_mul(num, R^2 / den) = (num / den) R, the ratio in Montgomery form.
// (Without den: fp_mul(num, R^2).)  The scan multiplies Montgomery elements into a PLAIN running value — fp_mul(h, x R) =
// h x — so init, the carries between levels and the outputs are plain, the level products Montgomery.
// Bounds, in units of r: an input < 1 (a non-canonical one, < 2^256 < 5.3, raises FLAG_NONCANONICAL and the result is
// discarded); Fr::one(), R^2, top, init < 1; a product fp_mul(a, b) < a b / 169 + 1: of two values < 1.17 it is < 1.009,
// of a value < 1.17 and an input < 5.3 it is < 1.04, of two inputs < 1.17.  So every running value, tree slot and carry is
// < 1.17 (< 1.009 for canonical input), and every value stored to memory goes through fp_cond_sub (< 2 -> canonical):
// level buffers and outputs hold canonical integers only.
// Term kernels: a term v + b + gamma (v an input, b a product < 1.04, gamma < 1) is < 3.04 (< 7.4 non-canonical); the
// accumulator starts at R^m (R^2) < 1 and stays < 7.4 * 1.05 / 169 + 1 < 1.05; stored through fp_cond_sub.
//
// Batch.  k_fr_prod_chunk and k_fr_prod_scan take blockIdx.y as the column of a batch of running products (the lookups of a
// chunk): every array of the launch is a slab, column y at + y * its stride in bytes (fr_prod_column; the strides are 0 in a
// single call, whose grid has one row).  A level above the elements is [columns][chunks].  k_fr_lookup_terms takes blockIdx.y
// as the lookup in the same way.  Indices inside a column stay 32-bit.
//
// Per-call constants (top, init, beta, gamma, the delta powers) come BY VALUE in the kernel arguments: a device block that
// a host copy fills could be rewritten by a second queued call before the first one's launch has read it
// (fr_fft_kernels.hpp, poly_kernels.hpp).  The table of w^i is built by k_fr_powers on the same stream.
#pragma once
#include "fr_chunk.hpp"

namespace h2agg {

constexpr unsigned FR_PROD_MAX_COLUMNS = 16;
enum : uint32_t { FR_PROD_INVERT = 0, FR_PROD_SCAN = 1 };

struct FrProdArgs {
    uint32_t top[8];        // the top chunk of a down-sweep (carry == null): invert: `top`; scan: init.  canonical
    const uint8_t* src;     // level 0: the elements (invert: in; scan: num); above: this level's products
    const uint8_t* aux;     // scan, level 0: R^2 / den per element (ours, canonical); null: no den
    uint8_t* dst;           // up-sweep: the next level, [chunks]; down-sweep: [n]
    const uint8_t* carry;   // down-sweep: the level above after ITS down-sweep, [chunks]; null at the top
    uint32_t* flags;
    uint32_t n;             // elements at this level.  scan, level 0: u + 1 positions, element u reads as 1
    uint32_t t;             // log2 T, FR_CHUNK_PER_LOG .. FR_CHUNK_LOG
    uint32_t op;            // FR_PROD_INVERT / FR_PROD_SCAN
    uint32_t level0;
    uint32_t check;         // level 0: src is the caller's, elements are checked for < r
    size_t src_stride, aux_stride, dst_stride, carry_stride;   // bytes from column y to y + 1 of each array (file header, "Batch")
};

FP_INLINE FrProdArgs fr_prod_column(FrProdArgs a) {
    const size_t y = blockIdx.y;
    a.src += y * a.src_stride;
    if (a.aux) a.aux += y * a.aux_stride;
    a.dst += y * a.dst_stride;
    if (a.carry) a.carry += y * a.carry_stride;
    return a;
}

// Element i of this level in the form the sweep multiplies (file header); zero: an inversion's input that is 0.
// Reads src[i] (and aux[i]) for i < n only — scan, level 0: i < n - 1 = u.
FP_INLINE Fr fr_prod_element(const FrProdArgs& a, uint32_t i, bool& zero) {
    zero = false;
    const uint32_t have = a.level0 && a.op == FR_PROD_SCAN ? a.n - 1u : a.n;
    if (i >= have) return Fr::one();
    const Fr x = fp_load<FrParams>(a.src + 32 * (size_t)i);
    if (!a.level0) return x;
    if (a.check && !fp_is_canonical<FrParams>(x)) atomicOr(a.flags, FLAG_NONCANONICAL);
    if (a.op == FR_PROD_SCAN) return fp_mul<FrParams>(x, a.aux ? fp_load<FrParams>(a.aux + 32 * (size_t)i) : Fr::r2());
    zero = x.is_zero_int();
    return zero ? Fr::one() : x;
}

// The sweeps over the 8 elements a thread holds.  Recursive templates, as in poly_kernels.hpp: with the field product
// inlined a loop body is too large for the compiler to unroll on request, and a loop that stays rolled indexes the arrays
// dynamically, which would put them into scratch memory.
//   load: x[e] = element i0 + e (1 for an idle thread), zmask bit e = it was a zero
template <int E>
FP_INLINE void fr_prod_load(const FrProdArgs& a, bool active, uint32_t i0, Fr (&x)[FR_CHUNK_PER], uint32_t& zmask) {
    if constexpr (E < (int)FR_CHUNK_PER) {
        bool zero = false;
        x[E] = active ? fr_prod_element(a, i0 + E, zero) : Fr::one();
        if (zero) zmask |= 1u << E;
        fr_prod_load<E + 1>(a, active, i0, x, zmask);
    }
}
//   prefix: pre[e] = x[0] * .. * x[e], e < 7; returns through p the product of all 8
template <int E>
FP_INLINE void fr_prod_prefix(const Fr (&x)[FR_CHUNK_PER], Fr (&pre)[FR_CHUNK_PER - 1], Fr& p) {
    if constexpr (E < (int)FR_CHUNK_PER - 1) {
        pre[E] = E == 0 ? x[0] : fp_mul<FrParams>(pre[E > 0 ? E - 1 : 0], x[E]);
        fr_prod_prefix<E + 1>(x, pre, p);
    } else {
        p = fp_mul<FrParams>(pre[FR_CHUNK_PER - 2], x[FR_CHUNK_PER - 1]);
    }
}
//   fold: p = x[0] * .. * x[7]
template <int E>
FP_INLINE void fr_prod_fold(const Fr (&x)[FR_CHUNK_PER], Fr& p) {
    if constexpr (E < (int)FR_CHUNK_PER) {
        p = E == 0 ? x[0] : fp_mul<FrParams>(p, x[E]);
        fr_prod_fold<E + 1>(x, p);
    }
}
//   back: j = the inverse of x[0..E] -> out[i0 + E] = j * pre[E - 1], j -> j * x[E]; E = 7 .. 0; stores only below n
template <int E>
FP_INLINE void fr_prod_back(const Fr (&x)[FR_CHUNK_PER], const Fr (&pre)[FR_CHUNK_PER - 1], Fr& j, uint32_t zmask, uint8_t* dst,
                            uint32_t i0, uint32_t n) {
    if constexpr (E >= 0) {
        Fr o = j;
        if constexpr (E > 0) {
            o = fp_mul<FrParams>(j, pre[E - 1]);
            j = fp_mul<FrParams>(j, x[E]);
        }
        if (i0 + E < n) fp_store<FrParams>(dst + 32 * (size_t)(i0 + E), (zmask >> E) & 1u ? Fr::zero() : fp_cond_sub<FrParams>(o));
        fr_prod_back<E - 1>(x, pre, j, zmask, dst, i0, n);
    }
}
//   emit: out[i0 + E] = h, h -> h * x[E]; E = 0 .. 7; stores only below n
template <int E>
FP_INLINE void fr_prod_emit(const Fr (&x)[FR_CHUNK_PER], Fr& h, uint8_t* dst, uint32_t i0, uint32_t n) {
    if constexpr (E < (int)FR_CHUNK_PER) {
        if (i0 + E < n) fp_store<FrParams>(dst + 32 * (size_t)(i0 + E), fp_cond_sub<FrParams>(h));
        if constexpr (E + 1 < (int)FR_CHUNK_PER) h = fp_mul<FrParams>(h, x[E]);
        fr_prod_emit<E + 1>(x, h, dst, i0, n);
    }
}

// Leaves, then the tree: slot v = slot 2v * slot 2v + 1, v = nthr - 1 .. 1.  Slots < 2 nthr <= 512.  Ends behind a barrier.
FP_INLINE void fr_prod_tree_up(uint32_t* lds, uint32_t tid, uint32_t nthr, const Fr& p) {
    if (tid < nthr) fr_fft_lds_put(lds, nthr + tid, p);
    __syncthreads();
#pragma unroll 1
    for (uint32_t s = nthr >> 1; s >= 1; s >>= 1) {
        if (tid < s) fr_fft_lds_put(lds, s + tid, fp_mul<FrParams>(fr_fft_lds_get(lds, 2 * (s + tid)), fr_fft_lds_get(lds, 2 * (s + tid) + 1)));
        __syncthreads();
    }
}

// Up-sweep.  Indices: a thread reads element i for i in [cT + 8 tid, cT + 8 tid + 8) with i < n only, thread 0 stores dst[c],
// c < chunks = gridDim.x.
__global__ void __launch_bounds__(FR_CHUNK_THREADS) k_fr_prod_chunk(const FrProdArgs a0) {
    const FrProdArgs a = fr_prod_column(a0);
    __shared__ uint32_t lds[NL * 2 * FR_CHUNK_THREADS];
    const auto [nthr, tid, c, i0] = fr_chunk(a.t, blockIdx.x);
    Fr x[FR_CHUNK_PER];
    uint32_t zmask = 0;
    fr_prod_load<0>(a, tid < nthr, i0, x, zmask);
    Fr p;
    fr_prod_fold<0>(x, p);
    fr_prod_tree_up(lds, tid, nthr, p);
    if (tid == 0) fp_store<FrParams>(a.dst + 32 * (size_t)c, fp_cond_sub<FrParams>(fr_fft_lds_get(lds, 1)));
}

// Down-sweep of the inversion.  IN PLACE (dst == src) IS SAFE BECAUSE: a workgroup reads only its own chunk of src — every
// thread its own 8 elements, all of them into registers before its first store — plus one element of `carry`, which is
// another buffer; and it stores only at the 8 indices it loaded.  No thread reads what another one writes.
__global__ void __launch_bounds__(FR_CHUNK_THREADS) k_fr_prod_invert(const FrProdArgs a) {
    __shared__ uint32_t lds[NL * 2 * FR_CHUNK_THREADS];
    const auto [nthr, tid, c, i0] = fr_chunk(a.t, blockIdx.x);
    Fr x[FR_CHUNK_PER], pre[FR_CHUNK_PER - 1];
    uint32_t zmask = 0;
    fr_prod_load<0>(a, tid < nthr, i0, x, zmask);
    Fr p;
    fr_prod_prefix<0>(x, pre, p);
    fr_prod_tree_up(lds, tid, nthr, p);
    if (tid == 0) {
        Fr inv;
        if (a.carry) {
            inv = fp_load<FrParams>(a.carry + 32 * (size_t)c);   // canonical: ours
        } else {   // the top: the call's one inversion.  root (no zero factor: never 0) -> R^2 / root -> times top
            const Fr root = fp_from_mont<FrParams>(fr_fft_lds_get(lds, 1));
            Fr ri;
            [[clang::always_inline]] ri = fp_inv_int<FrParams>(root);   // inlined HERE: a call frame would be scratch memory
            inv = fp_mul<FrParams>(fp_to_mont<FrParams>(ri), fp_unpack<FrParams>(a.top));
        }
        fr_fft_lds_put(lds, 1, inv);
    }
    __syncthreads();
    // slot v holds the inverse of node v: the children get it times their sibling.  A step reads and writes only the two
    // child slots of its own node, and the node's slot, which the step before wrote (barrier).
#pragma unroll 1
    for (uint32_t s = 1; s < nthr; s <<= 1) {
        if (tid < s) {
            const uint32_t v = s + tid;
            const Fr inv = fr_fft_lds_get(lds, v), l = fr_fft_lds_get(lds, 2 * v), r = fr_fft_lds_get(lds, 2 * v + 1);
            fr_fft_lds_put(lds, 2 * v, fp_mul<FrParams>(inv, r));
            fr_fft_lds_put(lds, 2 * v + 1, fp_mul<FrParams>(inv, l));
        }
        __syncthreads();
    }
    if (tid >= nthr) return;   // (behind the last barrier)
    Fr j = fr_fft_lds_get(lds, nthr + tid);
    fr_prod_back<(int)FR_CHUNK_PER - 1>(x, pre, j, zmask, a.dst, i0, a.n);
}

// Down-sweep of the scan.  In place (dst == src, which h2agg_fr_grand_product_device allows for out and num) is safe for the
// reason given at k_fr_prod_invert; dst[n - 1] (level 0: out[u]) is stored by the thread that owns position n - 1, which
// loads nothing there.
__global__ void __launch_bounds__(FR_CHUNK_THREADS) k_fr_prod_scan(const FrProdArgs a0) {
    const FrProdArgs a = fr_prod_column(a0);
    __shared__ uint32_t lds[NL * 2 * FR_CHUNK_THREADS];
    const auto [nthr, tid, c, i0] = fr_chunk(a.t, blockIdx.x);
    Fr x[FR_CHUNK_PER];
    uint32_t zmask = 0;
    fr_prod_load<0>(a, tid < nthr, i0, x, zmask);
    Fr p;
    fr_prod_fold<0>(x, p);
    fr_prod_tree_up(lds, tid, nthr, p);
    if (tid == 0) fr_fft_lds_put(lds, 1, a.carry ? fp_load<FrParams>(a.carry + 32 * (size_t)c) : fp_unpack<FrParams>(a.top));
    __syncthreads();
    // slot v holds the (plain) product of everything in front of node v: the left child inherits it, the right child gets
    // it times the left sibling.  Same slot discipline as in k_fr_prod_invert.
#pragma unroll 1
    for (uint32_t s = 1; s < nthr; s <<= 1) {
        if (tid < s) {
            const uint32_t v = s + tid;
            const Fr h = fr_fft_lds_get(lds, v), l = fr_fft_lds_get(lds, 2 * v);
            fr_fft_lds_put(lds, 2 * v, h);
            fr_fft_lds_put(lds, 2 * v + 1, fp_mul<FrParams>(h, l));
        }
        __syncthreads();
    }
    if (tid >= nthr) return;   // (behind the last barrier)
    Fr h = fr_fft_lds_get(lds, nthr + tid);
    fr_prod_emit<0>(x, h, a.dst, i0, a.n);
}

struct FrPermArgs {
    uint32_t beta[8];                       // beta R mod r (Montgomery), canonical
    uint32_t gamma[8];                      // plain
    uint32_t rm[8];                         // R^m mod r: the accumulators' start, so that m products leave a plain value
    uint32_t bd[FR_PROD_MAX_COLUMNS][8];    // beta * delta_first * delta^j, plain
    const uint8_t* values;                  // [m][n]
    const uint8_t* sigmas;                  // [m][n]
    uint8_t* num;                           // [u]
    uint8_t* den;                           // [u]
    const uint8_t* w_lo;                    // Montgomery w^i, i < 2^wT   (fr_fft_table's pair)
    const uint8_t* w_hi;                    // Montgomery w^(i * 2^wT)
    uint32_t* flags;
    uint32_t n, u, m, wT;
};

// num[i] = prod_j (values[j][i] + beta dj w^i + gamma), den[i] = prod_j (values[j][i] + beta sigmas[j][i] + gamma), i < u < n:
// consecutive threads read consecutive rows of every column.  Table indices: i < n = 2^k, the table's size.
__global__ void __launch_bounds__(BLOCK) k_fr_perm_terms(const FrPermArgs a) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.u) return;
    const Fr wi = i ? fr_fft_table(a.w_lo, a.w_hi, a.wT, i) : Fr::one();   // w^i R, < 2
    const Fr betaM = fp_unpack<FrParams>(a.beta), gamma = fp_unpack<FrParams>(a.gamma);
    Fr num = fp_unpack<FrParams>(a.rm), den = num;
#pragma unroll 1
    for (uint32_t j = 0; j < a.m; ++j) {
        const Fr v = fp_load<FrParams>(a.values + 32 * ((size_t)j * a.n + i));
        const Fr s = fp_load<FrParams>(a.sigmas + 32 * ((size_t)j * a.n + i));
        if (!fp_is_canonical<FrParams>(v) || !fp_is_canonical<FrParams>(s)) atomicOr(a.flags, FLAG_NONCANONICAL);
        const Fr vg = fp_add<FrParams>(v, gamma);
        num = fp_mul<FrParams>(num, fp_add<FrParams>(vg, fp_mul<FrParams>(fp_unpack<FrParams>(a.bd[j]), wi)));
        den = fp_mul<FrParams>(den, fp_add<FrParams>(vg, fp_mul<FrParams>(betaM, s)));
    }
    fp_store<FrParams>(a.num + 32 * (size_t)i, fp_cond_sub<FrParams>(num));
    fp_store<FrParams>(a.den + 32 * (size_t)i, fp_cond_sub<FrParams>(den));
}

struct FrLookupArgs {
    uint32_t beta[8], gamma[8];   // plain, canonical
    const uint8_t* a;             // compressed input, table, and their permuted forms: [n] each, rows < u are read
    const uint8_t* s;
    const uint8_t* ap;
    const uint8_t* sp;
    uint8_t* num;                 // [u]
    uint8_t* den;                 // [u]
    uint32_t* flags;
    size_t col_stride;            // bytes between the lookups' columns of a, s, ap, sp; num and den are dense [lookups][u]
    uint32_t u;
};

// num[i] = (a[i] + beta)(s[i] + gamma), den[i] = (ap[i] + beta)(sp[i] + gamma), i < u; blockIdx.y = lookup
__global__ void __launch_bounds__(BLOCK) k_fr_lookup_terms(const FrLookupArgs a0) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a0.u) return;
    FrLookupArgs a = a0;
    {
        const size_t y = blockIdx.y, at = y * a.col_stride, dense = y * 32 * (size_t)a.u;
        a.a += at;
        a.s += at;
        a.ap += at;
        a.sp += at;
        a.num += dense;
        a.den += dense;
    }
    const Fr beta = fp_unpack<FrParams>(a.beta), gamma = fp_unpack<FrParams>(a.gamma);
    const Fr x = fp_load<FrParams>(a.a + 32 * (size_t)i), s = fp_load<FrParams>(a.s + 32 * (size_t)i);
    const Fr xp = fp_load<FrParams>(a.ap + 32 * (size_t)i), sp = fp_load<FrParams>(a.sp + 32 * (size_t)i);
    if (!fp_is_canonical<FrParams>(x) || !fp_is_canonical<FrParams>(s) || !fp_is_canonical<FrParams>(xp) || !fp_is_canonical<FrParams>(sp))
        atomicOr(a.flags, FLAG_NONCANONICAL);
    const Fr num = fp_mul<FrParams>(fp_mul<FrParams>(Fr::r2(), fp_add<FrParams>(x, beta)), fp_add<FrParams>(s, gamma));
    const Fr den = fp_mul<FrParams>(fp_mul<FrParams>(Fr::r2(), fp_add<FrParams>(xp, beta)), fp_add<FrParams>(sp, gamma));
    fp_store<FrParams>(a.num + 32 * (size_t)i, fp_cond_sub<FrParams>(num));
    fp_store<FrParams>(a.den + 32 * (size_t)i, fp_cond_sub<FrParams>(den));
}

}  // namespace h2agg
