// The permutation half of keygen for gfx950: the sigma columns of a permutation given as a cell mapping — the device side of
//   permutation::keygen::Assembly::build_vk / build_pk  (halo2_proofs permutation/keygen.rs; the crate is an unvendored git
//    dependency of the reference: recalled, DESIGN.md section 2 — the yardstick is the definition in include/h2agg.h)
//   sigma[j][i] = delta^c * w^r  for {c, r} = mapping[j][i],  m columns of n = 2^k rows.
//
// One kernel, k_perm_sigma, over the m * n cells; memory-bound: 8 B read and 32 B written per cell, plus one bitmap atomic.
// Cell x = j * n + i reads its entry as one 8-byte load (consecutive lanes, consecutive entries) and stores 32 contiguous
// bytes, as the other Fr kernels store.  It is also the validity check of the mapping (include/h2agg.h):
//   - c < m and r < n are tested BEFORE any address is formed from them: an entry that fails raises FLAG_BAD_MAPPING and the
//     cell is skipped (nothing read or written through it);
//   - a cell with i >= usable must map to itself;
//   - bit c * n + r of a bitmap (one bit per cell, cleared in front of the launch) is set with atomicOr: a bit that was set
//     already is a second cell with the same target, so m * n entries that all pass are a bijection of the cells.
// The factors: w^r = lo[e & (2^T - 1)] * hi[e >> T] from the context's two-level twiddle tables through fr_fft_table (at most
// one product; the tables are built for the largest K seen, so e = r << (K - k)); delta^c from a table of m entries that
// k_fr_powers builds per call — with A = 1, i.e. as plain integers, not in Montgomery form: the Montgomery product
// (w^r R) * delta^c / R is then the canonical value itself, and the one product that combines the factors is also the
// conversion out.  A cell costs two products at most (r == 0 and a zero half of the exponent read an entry instead of
// forming the twiddle product; c == 0 multiplies by the entry 1, which is the conversion).  Cell indices, bit indices and
// slab offsets are 64-bit: m * n reaches 2^36.
#pragma once
#include "fr_fft_kernels.hpp"
#include "lookup_kernels.hpp"

namespace h2agg {

enum : uint32_t { FLAG_BAD_MAPPING = 16u };
static_assert((FLAG_BAD_MAPPING & (FLAG_NONCANONICAL | FLAG_DIV_ZERO | FLAG_BAD_POINT | FLAG_NOT_IN_TABLE)) == 0, "status bits must be disjoint");

constexpr unsigned PERM_MAX_COLUMNS = 4096;   // H2AGG_PERM_MAX_COLUMNS: the delta table is one k_fr_powers launch (<= 2^FRW_TABLE entries)
static_assert(PERM_MAX_COLUMNS <= (1u << FRW_TABLE), "k_fr_powers builds at most 2^FRW_TABLE entries");

struct PermSigmaArgs {
    const uint2* mapping;    // [m * n] {column, row}
    uint8_t* out;            // [m][n], canonical
    uint32_t* bitmap;        // ceil(m n / 32) words, zero
    uint32_t* flags;
    const uint8_t* tw_lo;    // Montgomery w_K^i, i < 2^tw_T
    const uint8_t* tw_hi;    // Montgomery w_K^(i * 2^tw_T)
    const uint8_t* delta;    // delta^c as a plain canonical integer, c < m
    uint64_t cells;          // m * n
    uint32_t m, k, usable;
    uint32_t tw_T, tw_up;    // split of the twiddle tables; K - k
};

// Every address is formed from a cell index x < cells (mapping, out), from c < m (delta), from e = r << tw_up < 2^K (the
// tables hold 2^tw_T + 2^(K - tw_T) entries), or from the bit index c * n + r < cells (bitmap).
__global__ void __launch_bounds__(BLOCK) k_perm_sigma(const PermSigmaArgs p) {
    const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
    const uint64_t nmask = ((uint64_t)1 << p.k) - 1u;
#pragma unroll 1
    for (uint64_t x = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; x < p.cells; x += stride) {
        const uint2 e = p.mapping[x];
        const uint32_t c = e.x, r = e.y;
        if (c >= p.m || r > nmask) {
            atomicOr(p.flags, FLAG_BAD_MAPPING);
            continue;
        }
        const uint64_t j = x >> p.k, i = x & nmask;
        if (i >= p.usable && (c != j || r != i)) atomicOr(p.flags, FLAG_BAD_MAPPING);
        const uint64_t bit = ((uint64_t)c << p.k) | r;
        const uint32_t mask = 1u << (bit & 31u);
        if (atomicOr(p.bitmap + (bit >> 5), mask) & mask) atomicOr(p.flags, FLAG_BAD_MAPPING);
        // (w^r R) * delta^c / R: the delta table holds plain integers, so the combining product is also the conversion out
        const Fr w = r ? fr_fft_table(p.tw_lo, p.tw_hi, p.tw_T, r << p.tw_up) : Fr::one();   // < 2r
        fp_store<FrParams>(p.out + 32 * x, fp_cond_sub<FrParams>(fp_mul<FrParams>(w, fp_load<FrParams>(p.delta + 32 * (size_t)c))));
    }
}

}  // namespace h2agg
