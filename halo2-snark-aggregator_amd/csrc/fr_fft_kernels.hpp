// Discrete Fourier transform over Fr for gfx950: the device side of
//   best_fft / EvaluationDomain::{lagrange_to_coeff, coeff_to_lagrange, coeff_to_extended, extended_to_coeff}
//   (halo2_proofs arithmetic.rs / poly/domain.rs; the crate is an unvendored git dependency of the reference: recalled,
//    DESIGN.md section 2 — the yardstick is the definition in include/h2agg.h)
//   forward:  out[i] = sum_j (shift^j * in[j]) * w^(i*j)            inverse:  out[j] = shift^-j / n * sum_i in[i] * w^(-i*j)
// natural order in and out, n = 2^k, k <= FFT_MAX_K.
//
// Pass plan.  The k index bits are cut into P = ceil(k / L) digits, most significant first: P - 1 digits of L bits and a
// last one of k - (P - 1) L bits (L = FR_FFT_LOCAL = 10: two passes at k = 20, three at k = 24).  Pass p is a
// decimation-in-frequency step over digit p: for every value of the other bits, a 2^width-point transform over that digit,
// then the twiddle w^(i_p * 2^hb * jrest) — i_p the output digit, hb the bits above the digit, jrest the input bits below
// it.  That leaves the array in digit-reversed order; the LAST pass undoes it where it writes, so there is no bit-reversal
// launch: it reads tile digitrev(rho) and writes out[(i_P << (k - width)) | rho].  Passes in front of it work in place on
// the context's work array (Montgomery form, 32 B per element); the last one, which permutes, is out of place (work array
// -> out), so d_out == d_in is allowed.  A single pass (k <= L) is one workgroup that reads everything before it writes.
//
// One pass = one launch of k_fr_fft_pass.  A workgroup holds FR_FFT_TILE = 2048 elements in LDS as nine 29-bit limbs each
// (72 KiB: two workgroups per CU inside 160 KiB; the 9-dword stride keeps consecutive elements on different banks): C =
// 2048 >> width transforms side by side, over C CONSECUTIVE values of the low bits, so global accesses are runs of C
// elements (the last pass reads whole tiles and writes runs of C).  Inside the tile the 2^width-point transform is
// decimation-in-time: elements are stored to bit-reversed rows as they are loaded, then `width` radix-2 stages
// (a, b) -> (a + t b, a - t b) with a barrier between stages; rows come out in natural order.  Every stored value is < 2r
// (one conditional subtraction of 2r per butterfly output: without it the twiddle-1 path doubles its bound every stage).
// The first pass absorbs the conversion from canonical form and the inverse's 1/n (one product with a constant) and
// shift^j (one more, with the shift table's entry).  The last pass absorbs shift^-j and the conversion back.  Butterflies
// and inter-pass twiddles whose factor is 1 multiply nothing.
//
// Twiddles: no per-element pow.  w^e, e < 2^K, is lo[e & (2^T - 1)] * hi[e >> T] with two tables of <= 2^12 Montgomery
// entries per direction, built for the largest K seen and kept in the context (a smaller k shifts e left by K - k); a factor
// whose low or high part is 0 is one table entry and no product, which is every butterfly twiddle when K - L >= T.
// shift^j is the same pair of tables, built per call.  The tables come from k_fr_powers: k_fr_affine_powers' algorithm with
// the constants as kernel arguments — that kernel reads them from a device block which a host copy fills, and a second
// transform queued behind a first must not rewrite the block the first one's launch has not read yet.
//
// Batch.  A launch transforms m columns of 2^k elements, one pass of all of them: the tile index space of a pass is
// m * 2^(k - width), tile T being tile T & (2^(k - width) - 1) of column T >> (k - width).  Digit, jrest, twiddle exponent and
// the last pass's digit reversal act on the within-column tile; only the addresses know the column.  A workgroup's C tile
// columns run on across column boundaries: at k = 7 one workgroup holds 16 whole transforms, and the last workgroup of a
// launch may be partly empty.  The single transform is the batch of one.  The first pass reads its columns from a table of at
// most FR_FFT_SEGS segments (base pointer, first column), each a contiguous slab of stride 2^k — by value in the kernel
// arguments, for the reason above; the work array and the destination are contiguous slabs [m][2^k].  The shift table, the
// twiddle tables, cvt and the FLAG_NONCANONICAL report are shared by all columns of a launch.
#pragma once
#include "g1_fft_kernels.hpp"

namespace h2agg {

constexpr unsigned FR_FFT_LOCAL = 10;       // radix-2 stages fused per pass (default)
constexpr unsigned FR_FFT_TILE_LOG = 11;    // elements a workgroup holds in LDS: 2^11 * 36 B = 72 KiB
constexpr unsigned FR_FFT_TILE = 1u << FR_FFT_TILE_LOG;
constexpr int FR_FFT_THREADS = 512;
constexpr int FRW_TABLE = 13;               // base^(2^j), j < 13: the tables have at most 2^12 entries
constexpr int FR_FFT_SEGS = 9;              // source slabs of one batched launch (the quotient's nine kinds of polynomial)
constexpr unsigned FR_FFT_BATCH_WORK_LOG = 23;   // a batch's work array: at most 2^23 elements (256 MiB), or one column

struct FrPowersArgs {
    uint32_t pw[FRW_TABLE][8];   // base^(2^j), canonical
    uint32_t a[8];               // A, canonical
};

// out[i] = A * base^i as a canonical integer, i < n <= 2^FRW_TABLE.  (A = R: the Montgomery form of base^i.)
__global__ void __launch_bounds__(BLOCK) k_fr_powers(const FrPowersArgs args, uint32_t n, uint8_t* __restrict__ out) {
    const uint32_t i0 = (blockIdx.x * BLOCK + threadIdx.x) * FRP_CHUNK;
    if (i0 >= n) return;
    Fr cur = Fr::one();
#pragma unroll 1
    for (int j = 0; j < FRW_TABLE; ++j)
        if ((i0 >> j) & 1) cur = fp_mul<FrParams>(cur, fp_to_mont<FrParams>(fp_unpack<FrParams>(args.pw[j])));
    const Fr base = fp_to_mont<FrParams>(fp_unpack<FrParams>(args.pw[0]));
    const Fr a = fp_unpack<FrParams>(args.a);
#pragma unroll 1
    for (int e = 0; e < FRP_CHUNK && i0 + e < n; ++e) {
        fp_store<FrParams>(out + 32 * (size_t)(i0 + e), fp_cond_sub<FrParams>(fp_mul<FrParams>(cur, a)));   // (x R) * A / R
        cur = fp_mul<FrParams>(cur, base);
    }
}

struct FrFftPass {
    const uint8_t* seg_base[FR_FFT_SEGS];   // source slabs: columns seg_first[s] .. seg_first[s + 1] - 1 of the launch are the
    uint32_t seg_first[FR_FFT_SEGS];        // columns of slab s from its base on; seg_first[0] = 0, an unused entry ~0
    uint8_t* dst;                           // [m][2^k]
    uint32_t m;                             // columns of this launch; m * 2^(k - width) < 2^32
    const uint8_t* tw_lo;   // Montgomery w^i, i < 2^tw_T
    const uint8_t* tw_hi;   // Montgomery w^(i * 2^tw_T)
    const uint8_t* sh_lo;   // Montgomery shift^i (forward) / shift^-i (inverse), i < 2^sh_T; null without a shift
    const uint8_t* sh_hi;   // Montgomery shift^(+-i * 2^sh_T)
    uint32_t* flags;
    uint32_t k, width, lb, hb;   // bits of the array, of this pass's digit, below it, above it
    uint32_t local;              // L: width of the digits in front of the last one
    uint32_t digits;             // P - 1
    uint32_t tw_T, tw_up;        // split of the twiddle tables; K - k
    uint32_t sh_T;
    uint32_t first, last;
    uint32_t sh_first, sh_last;  // the shift table applies where this pass loads (forward) / stores (inverse)
    uint32_t cvt[NL];            // first pass: R^2 (forward), R^2 / n (inverse), as limbs
};

// a value < 4r -> < 2r
FP_INLINE Fr fr_fft_reduce2(const Fr& a) {
    int32_t x[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) x[i] = (int32_t)a.l[i] - (int32_t)km_limb<FrParams>(2, i);
    const Fr t = fp_normalize<FrParams>(x);
    const bool neg = (int32_t)t.l[8] < 0;
    Fr r;
#pragma unroll
    for (int i = 0; i < NL; ++i) r.l[i] = neg ? a.l[i] : t.l[i];
    return r;
}

// Montgomery base^e = lo[e & (2^T - 1)] * hi[e >> T], e != 0.  A zero half is the factor 1: no product.  Result < 2r.
FP_INLINE Fr fr_fft_table(const uint8_t* __restrict__ lo, const uint8_t* __restrict__ hi, uint32_t T, uint32_t e) {
    const uint32_t el = e & ((1u << T) - 1u), eh = e >> T;
    if (el == 0) return fp_load<FrParams>(hi + 32 * (size_t)eh);
    const Fr a = fp_load<FrParams>(lo + 32 * (size_t)el);
    if (eh == 0) return a;
    return fp_mul<FrParams>(a, fp_load<FrParams>(hi + 32 * (size_t)eh));
}

FP_INLINE Fr fr_fft_lds_get(const uint32_t* lds, uint32_t e) {
    Fr r;
#pragma unroll
    for (int i = 0; i < NL; ++i) r.l[i] = lds[NL * e + i];
    return r;
}
FP_INLINE void fr_fft_lds_put(uint32_t* lds, uint32_t e, const Fr& v) {
#pragma unroll
    for (int i = 0; i < NL; ++i) lds[NL * e + i] = v.l[i];
}

// One pass (see the file header).  Workgroup b holds tiles b * C .. b * C + C - 1 of the batch's m * 2^(k - width), C =
// FR_FFT_TILE >> width; element (row, column) of the tile set is at LDS index row * C + column.  Every global address is a
// column's base (column < m) plus 32 g, g < 2^k, and every LDS index < FR_FFT_TILE: rows < 2^width, columns < C, columns of
// tiles >= m * 2^(k - width) are skipped.
__global__ void __launch_bounds__(FR_FFT_THREADS) k_fr_fft_pass(const FrFftPass p) {
    __shared__ uint32_t lds[NL * FR_FFT_TILE];
    const uint32_t lgC = FR_FFT_TILE_LOG - p.width, C = 1u << lgC;
    const uint32_t ctb = p.k - p.width, ctmask = (1u << ctb) - 1u;   // tiles of one column: 2^ctb
    const uint32_t ntiles = p.m << ctb;
    const uint32_t tile0 = blockIdx.x * C;
    const uint32_t lbmask = (1u << p.lb) - 1u;

    // ---- load: digit value d of tile column c -> row bitrev(d)
#pragma unroll 1
    for (uint32_t idx = threadIdx.x; idx < FR_FFT_TILE; idx += FR_FFT_THREADS) {
        // the last pass reads whole tiles (digit fastest); the others runs of C columns (column fastest)
        const uint32_t c = p.last ? idx >> p.width : idx & (C - 1u);
        const uint32_t d = p.last ? idx & ((1u << p.width) - 1u) : idx >> lgC;
        if (tile0 + c >= ntiles) continue;
        const uint32_t col = (tile0 + c) >> ctb, t = (tile0 + c) & ctmask;
        uint32_t g;
        if (p.last) {
            uint32_t pi = 0, rho = t;
#pragma unroll 1
            for (uint32_t q = 0; q < p.digits; ++q) {
                pi = (pi << p.local) | (rho & ((1u << p.local) - 1u));
                rho >>= p.local;
            }
            g = (pi << p.width) | d;
        } else {
            g = ((t >> p.lb) << (p.width + p.lb)) | (d << p.lb) | (t & lbmask);
        }
        const uint8_t* base = p.seg_base[0];
        uint32_t at = col;
        if (p.seg_first[1] != ~0u) {   // (uniform: one slab — the work array, a single transform — looks nothing up)
#pragma unroll
            for (int sg = 1; sg < FR_FFT_SEGS; ++sg)
                if (col >= p.seg_first[sg]) {
                    base = p.seg_base[sg];
                    at = col - p.seg_first[sg];
                }
        }
        Fr x = fp_load<FrParams>(base + (((size_t)at << p.k) + g) * 32);
        if (p.first) {
            if (!fp_is_canonical<FrParams>(x)) atomicOr(p.flags, FLAG_NONCANONICAL);
            Fr cv;
#pragma unroll
            for (int i = 0; i < NL; ++i) cv.l[i] = p.cvt[i];
            x = fp_mul<FrParams>(x, cv);                                    // x < 2^256 < 5.3 r  ->  (x [/ n]) R, < 2r
            if (p.sh_first && g) x = fp_mul<FrParams>(x, fr_fft_table(p.sh_lo, p.sh_hi, p.sh_T, g));
        }
        const uint32_t row = p.width ? __brev(d) >> (32u - p.width) : 0u;
        fr_fft_lds_put(lds, (row << lgC) | c, x);
    }
    __syncthreads();

    // ---- `width` radix-2 decimation-in-time stages; butterfly u: column u & (C - 1), butterfly u >> lgC of its transform
#pragma unroll 1
    for (uint32_t s = 1; s <= p.width; ++s) {
        const uint32_t half = 1u << (s - 1u);
#pragma unroll 1
        for (uint32_t u = threadIdx.x; u < FR_FFT_TILE / 2; u += FR_FFT_THREADS) {
            const uint32_t c = u & (C - 1u), q = u >> lgC;
            if (tile0 + c >= ntiles) continue;
            const uint32_t pos = q & (half - 1u), blk = q >> (s - 1u);
            const uint32_t ra = (blk << s) | pos, ea = (ra << lgC) | c, eb = ((ra + half) << lgC) | c;
            const Fr a = fr_fft_lds_get(lds, ea);
            Fr b = fr_fft_lds_get(lds, eb);
            // w^(pos * 2^(k - s)) in units of the table's root
            if (pos) b = fp_mul<FrParams>(b, fr_fft_table(p.tw_lo, p.tw_hi, p.tw_T, pos << (p.k - s + p.tw_up)));
            fr_fft_lds_put(lds, ea, fr_fft_reduce2(fp_add<FrParams>(a, b)));          // a, b < 2r
            fr_fft_lds_put(lds, eb, fr_fft_reduce2(fp_sub<2, FrParams>(a, b)));
        }
        __syncthreads();
    }

    // ---- store (column fastest): row d is the output digit
#pragma unroll 1
    for (uint32_t idx = threadIdx.x; idx < FR_FFT_TILE; idx += FR_FFT_THREADS) {
        const uint32_t c = idx & (C - 1u), d = idx >> lgC;
        if (tile0 + c >= ntiles) continue;
        const uint32_t col = (tile0 + c) >> ctb, t = (tile0 + c) & ctmask;
        Fr v = fr_fft_lds_get(lds, idx);
        uint32_t g;
        if (p.last) {
            g = (d << (p.k - p.width)) | t;
            if (p.sh_last && g) v = fp_mul<FrParams>(v, fr_fft_table(p.sh_lo, p.sh_hi, p.sh_T, g));
            v = fp_from_mont<FrParams>(v);
        } else {
            const uint32_t jrest = t & lbmask;
            g = ((t >> p.lb) << (p.width + p.lb)) | (d << p.lb) | jrest;
            const uint32_t e = (d << p.hb) * jrest;   // < 2^k
            if (e) v = fp_mul<FrParams>(v, fr_fft_table(p.tw_lo, p.tw_hi, p.tw_T, e << p.tw_up));
        }
        fp_store<FrParams>(p.dst + (((size_t)col << p.k) + g) * 32, v);
    }
}

}  // namespace h2agg
