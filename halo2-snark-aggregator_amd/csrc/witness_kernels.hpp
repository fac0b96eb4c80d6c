// The witness check for gfx950: the device side of
//   h2agg_witness_check   which gate polynomial, permutation column or lookup a witness fails, and on which rows
//   (halo2_proofs' dev::MockProver::verify: the crate is an unvendored git dependency of the reference, recalled — DESIGN.md
//    section 2; the yardstick is the definition in include/h2agg.h.  The order of the constraints is pinned:
//    halo2-snark-aggregator-api/src/systems/halo2/params.rs:74-224.)
// Nothing here writes a value per (constraint, row).  Every check sets ONE BIT per (constraint, row) — a line of
// zwords = 2 ceil(n / 64) words per constraint, bit (i & 31) of word i >> 5 is row i — and the report kernels turn the lines
// into counts, first rows and the lowest failing rows.
//
// Flags.  A wave holds 64 consecutive rows and stores their bits as two words (qe_put_flag, quotient_kernels.hpp): no
// atomics, one writer per word, and every word of a line is written by every launch (a wave with a row below n stores both
// of its words; rows from n up vote 0), so the lines need no clearing.
//   gates         k_qe_eval<true> (quotient_kernels.hpp): the interpreter with the zero test as its ending, rows below u
//   permutation   k_wc_permutation: cell (g, i) against its image under the mapping, 32 bytes each, all n rows
//   lookups       k_wc_lookup: row i < u of the folded input by binary search in the sorted folded table rows [0, u)
//                 (the sort is lookup_kernels.hpp's; the folds are k_qe_eval<false> with fold = theta)
//
// Report.  Deterministic: no atomic decides an order or a count.  One wave per workgroup, lane l of workgroup b holds
// word 64 b + l of a line (32 rows), so a workgroup covers a tile of WC_TILE_ROWS = 2048 rows:
//   k_wc_tile_count   the tile's failing rows (popcount, wave sum) and its lowest one (wave minimum): sums / mins [line][tile]
//   k_wc_line         per line, one wave walks the tile sums in steps of 64: the exclusive prefix of every tile in place
//                     (wave scan, the sum carried from step to step), the total -> counts, the minimum -> first_rows
//   k_wc_place        a tile whose prefix is below max_rows: the exclusive wave scan of its lanes' popcounts on top of the
//                     prefix gives every failing row its rank; ranks below max_rows are stored — ascending rows, ascending
//                     ranks.  The rest of rows[] keeps the 0xFFFFFFFF the host's memset put there.
//   k_wc_total        the 64-bit sum of counts
// Nothing here multiplies but the interpreter.  No per-thread array: the 256-bit compares are unrolled over registers.
#pragma once
#include "lookup_kernels.hpp"
#include "quotient_kernels.hpp"

namespace h2agg {

constexpr int WC_WAVE = 64;                            // threads of a report workgroup: one wave
constexpr uint32_t WC_TILE_ROWS = 32u * WC_WAVE;       // rows a report workgroup covers
constexpr uint32_t WC_NONE = 0xFFFFFFFFu;              // "no row"

struct WcPermArgs {
    const uint8_t* advice;    // slab 0, 1, 2: [columns][n]
    const uint8_t* fixed;
    const uint8_t* instance;
    const uint32_t* cols;     // [P] pairs {slab, column of the slab}: where permutation column g lives (k_qe_put)
    const uint2* mapping;     // [P][n] pairs {column, row}
    uint32_t* zflags;         // [gridDim.y][zwords]: line y is permutation column g0 + y
    uint32_t* flags;
    uint32_t n, P, g0, zwords;
};

// the cell (column c < P, row r < n) of the permutation: cols[2c] is 0, 1 or 2 and cols[2c + 1] a column of that slab (the
// key's own check, h2agg_vk_create: every permutation column is a queried column of its kind)
FP_INLINE U256 wc_cell(const WcPermArgs& a, uint32_t c, uint32_t r) {
    const uint32_t s = a.cols[2u * c], col = a.cols[2u * c + 1u];
    const uint8_t* slab = s == 0 ? a.advice : s == 1 ? a.fixed : a.instance;
    return u256_load(slab + 32 * ((size_t)col * a.n + r));
}

// Cell (g, i), g = g0 + blockIdx.y < P, i < n: fails when its value differs from the value of its image {c', r'} =
// mapping[g][i].  Consecutive threads take consecutive rows of one column.  c' < P and r' < n are tested before any address
// is formed from them (the host has scanned the mapping already: this is the guard, FLAG_BAD_MAPPING, the cell does not
// fail); a cell that maps to itself reads nothing more.  Every cell is checked for < r.  Writes line blockIdx.y of zflags.
__global__ void __launch_bounds__(BLOCK) k_wc_permutation(const WcPermArgs a) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x, g = a.g0 + blockIdx.y;
    if (i >= a.n || g >= a.P) return;
    const U256 x = wc_cell(a, g, i);
    if (!u256_is_canonical_fr(x)) atomicOr(a.flags, FLAG_NONCANONICAL);
    const uint2 m = a.mapping[(size_t)g * a.n + i];
    bool fails = false;
    if (m.x >= a.P || m.y >= a.n) atomicOr(a.flags, FLAG_BAD_MAPPING);
    else if (m.x != g || m.y != i) fails = !lk_equal(x, wc_cell(a, m.x, m.y));
    qe_put_flag(fails, a.zflags + (size_t)blockIdx.y * a.zwords, i);
}

struct WcLookupArgs {
    const uint8_t* a;         // [n] the folded input expressions (canonical: k_qe_eval's output)
    const uint8_t* s_in;      // the sorted folded table rows [0, u): the three buffers of the sort and its plan
    const uint8_t* s_w0;
    const uint8_t* s_w1;
    const uint32_t* s_plan;
    uint32_t* zflags;         // [zwords]
    uint32_t n, u;
};

// Row i < u fails when a[i] is not among the u sorted keys: the first key >= a[i] (binary search: mid < hi <= u, so every key
// read is below u) is not equal to it.  Rows u .. n - 1 read nothing and vote 0.  The same predicate as k_lk_heads', per row.
__global__ void __launch_bounds__(BLOCK) k_wc_lookup(const WcLookupArgs p) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= p.n) return;
    bool fails = false;
    if (i < p.u) {
        const uint8_t* S = lk_state_buf(p.s_in, p.s_w0, p.s_w1, p.s_plan[LK_PASSES]);
        const U256 x = u256_load(p.a + 32 * (size_t)i);
        uint32_t lo = 0, hi = p.u;
#pragma unroll 1
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (lk_less(u256_load(S + 32 * (size_t)mid), x)) lo = mid + 1;
            else hi = mid;
        }
        fails = !(lo < p.u && lk_equal(u256_load(S + 32 * (size_t)lo), x));
    }
    qe_put_flag(fails, p.zflags, i);
}

struct WcReportArgs {
    const uint32_t* zflags;   // [lines][zwords]
    uint32_t* sums;           // [lines][tiles]: a tile's failing rows, then (k_wc_line) the failing rows of the tiles below it
    uint32_t* mins;           // [lines][tiles]: a tile's lowest failing row or WC_NONE
    uint32_t* counts;         // [C]   the call's report: line y is constraint c0 + y
    uint32_t* first_rows;     // [C]
    uint32_t* rows;           // [C][max_rows]
    uint32_t zwords, tiles;   // tiles = ceil(zwords / 64)
    uint32_t c0, lines, max_rows;
};

FP_INLINE uint32_t wc_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
FP_INLINE uint32_t wc_wave_min(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}
// inclusive prefix sum over the wave
FP_INLINE uint32_t wc_wave_incl_scan(uint32_t v) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(v, o, 64);
        if (lane >= (uint32_t)o) v += up;
    }
    return v;
}

// grid (tiles, lines).  Word w = 64 blockIdx.x + lane of line blockIdx.y, read only if w < zwords; a failing row 32 w + bit
// is < 32 zwords <= n + 63 < 2^25.  sums / mins index y tiles + x < lines tiles.
__global__ void __launch_bounds__(WC_WAVE) k_wc_tile_count(const WcReportArgs a) {
    const uint32_t w = blockIdx.x * WC_WAVE + threadIdx.x;
    const uint32_t v = w < a.zwords ? a.zflags[(size_t)blockIdx.y * a.zwords + w] : 0u;
    const uint32_t cnt = wc_wave_sum((uint32_t)__popc(v));
    const uint32_t mn = wc_wave_min(v ? 32u * w + (uint32_t)(__ffs((int)v) - 1) : WC_NONE);
    if (threadIdx.x == 0) {
        a.sums[(size_t)blockIdx.y * a.tiles + blockIdx.x] = cnt;
        a.mins[(size_t)blockIdx.y * a.tiles + blockIdx.x] = mn;
    }
}

// grid (lines).  One wave walks the tiles of line blockIdx.x in steps of 64: entry e = start + lane, touched only if
// e < tiles; a step's entries are all loaded before its first store.  counts / first_rows index c0 + blockIdx.x < C (the
// host launches lines = the constraints of the chunk that starts at c0).  A count is <= n <= 2^24: no overflow.
__global__ void __launch_bounds__(WC_WAVE) k_wc_line(const WcReportArgs a) {
    uint32_t* sums = a.sums + (size_t)blockIdx.x * a.tiles;
    const uint32_t* mins = a.mins + (size_t)blockIdx.x * a.tiles;
    uint32_t carry = 0, mn = WC_NONE;
#pragma unroll 1
    for (uint32_t start = 0; start < a.tiles; start += WC_WAVE) {
        const uint32_t e = start + threadIdx.x;
        const uint32_t v = e < a.tiles ? sums[e] : 0u;
        const uint32_t m = e < a.tiles ? mins[e] : WC_NONE;
        const uint32_t incl = wc_wave_incl_scan(v);
        if (e < a.tiles) sums[e] = carry + incl - v;
        carry += __shfl(incl, 63, 64);
        mn = m < mn ? m : mn;
    }
    mn = wc_wave_min(mn);
    if (threadIdx.x == 0) {
        a.counts[a.c0 + blockIdx.x] = carry;
        a.first_rows[a.c0 + blockIdx.x] = mn;
    }
}

// grid (tiles, lines); launched only with max_rows > 0.  base = the failing rows of the line below this tile (uniform: the
// whole workgroup leaves if none of its rows can rank below max_rows).  A lane's failing rows get the ranks base + (failing
// rows of lower lanes) + 0, 1, ..: stored while rank < max_rows, at rows[(c0 + y) max_rows + rank] — inside line c0 + y < C
// of the [C][max_rows] array.  Ranks are distinct, so every word has one writer.
__global__ void __launch_bounds__(WC_WAVE) k_wc_place(const WcReportArgs a) {
    const uint32_t base = a.sums[(size_t)blockIdx.y * a.tiles + blockIdx.x];
    if (base >= a.max_rows) return;
    const uint32_t w = blockIdx.x * WC_WAVE + threadIdx.x;
    uint32_t v = w < a.zwords ? a.zflags[(size_t)blockIdx.y * a.zwords + w] : 0u;
    const uint32_t cnt = (uint32_t)__popc(v);
    uint32_t rank = base + wc_wave_incl_scan(cnt) - cnt;
    uint32_t* line = a.rows + (size_t)(a.c0 + blockIdx.y) * a.max_rows;
#pragma unroll 1
    while (v && rank < a.max_rows) {
        line[rank++] = 32u * w + (uint32_t)(__ffs((int)v) - 1);
        v &= v - 1u;
    }
}

// One wave: total[0 .. 1] = the 64-bit sum of counts[0 .. C), low word first.  Index e < C.
__global__ void __launch_bounds__(WC_WAVE) k_wc_total(const uint32_t* __restrict__ counts, uint32_t C, uint32_t* __restrict__ total) {
    uint64_t s = 0;
    for (uint32_t e = threadIdx.x; e < C; e += WC_WAVE) s += counts[e];
    uint32_t lo = (uint32_t)s, hi = (uint32_t)(s >> 32);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t other = (uint64_t)__shfl_xor(lo, o, 64) | (uint64_t)__shfl_xor(hi, o, 64) << 32;
        s += other;
        lo = (uint32_t)s;
        hi = (uint32_t)(s >> 32);
    }
    if (threadIdx.x == 0) {
        total[0] = lo;
        total[1] = hi;
    }
}

}  // namespace h2agg
