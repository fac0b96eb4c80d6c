// The two kernels of the Fr column stores (csrc/columns.inc; include/h2agg.h "Fr column stores") for gfx950.  A store is a slab
// [m][n] of canonical 32-byte elements, n = 2^k, column j at byte 32 * n * j.  Both kernels are copy-bound and do nothing but
// move or look at bytes: no LDS, no scratch, every access 16 bytes wide (global_load_dwordx4 / global_store_dwordx4).
//
//   k_columns_move       dst[j][i] = src[j][(i + rotation) mod n]: 32 B read and 32 B written per element.  The unit is the
//     16-byte half of an element, one per lane, so a lane-PAIR moves an element and a wave's instruction covers 1 KiB of
//     contiguous destination (lane l at base + 16 l: the coalescing ideal).  A column is 2n units and the rotation 2 * rotation
//     units, reduced mod 2n on the host: the source unit of destination unit u is (u + shift) & (2n - 1).  The workgroup's part
//     of that sum — its first unit plus the shift — is uniform (one scalar add per workgroup); a lane adds its own index and
//     masks, because the wrap may fall inside a workgroup's span.  n is a power of two, so the mask is all the modulo there is.
//     A workgroup moves COLUMNS_MOVE_SPAN units of one column: COLUMNS_MOVE_UNROLL independent loads per lane are in flight
//     before the first store (16 KiB per workgroup instead of 4 KiB: fewer, longer workgroups for the same bytes).
//     grid = (ceil(2n / COLUMNS_MOVE_SPAN), columns).  Addresses: u <= mask < 2n inside column blockIdx.y < columns.
//
//   k_columns_canonical  raises FLAG_NONCANONICAL in the context's status word when an element is >= r: 32 B read per element,
//     nothing written but the flag.  One element per lane (two 16-byte loads: u256_load), the comparison the stage kernels
//     make on their inputs (u256_is_canonical_fr), a grid-stride loop over the elements the write covered.
#pragma once
#include "batch_kernels.hpp"

namespace h2agg {

constexpr unsigned COLUMNS_MOVE_UNROLL = 4;
constexpr unsigned COLUMNS_MOVE_SPAN = COLUMNS_MOVE_UNROLL * BLOCK;   // units of 16 bytes per workgroup

struct ColumnsMoveArgs {
    const uint4* src;      // column 0 of the source range
    uint4* dst;            // column 0 of the destination range
    uint32_t units_log;    // k + 1: a column is 2^units_log units
    uint32_t shift;        // (2 * rotation) mod 2^units_log
};

__global__ void __launch_bounds__(BLOCK) k_columns_move(const ColumnsMoveArgs a) {
    const uint32_t mask = (1u << a.units_log) - 1u;
    const uint32_t u0 = blockIdx.x * COLUMNS_MOVE_SPAN;   // uniform
    const uint32_t s0 = u0 + a.shift;                      // uniform: < 2^26 + 2^25
    const size_t col = (size_t)blockIdx.y << a.units_log;
    const uint4* src = a.src + col;
    uint4* dst = a.dst + col;
    // (four named values, not an array: a conditionally written private array is promoted to LDS)
    static_assert(COLUMNS_MOVE_UNROLL == 4, "the body below is written out for four units per lane");
    const uint32_t t0 = threadIdx.x, t1 = t0 + BLOCK, t2 = t0 + 2 * BLOCK, t3 = t0 + 3 * BLOCK;
    const bool p0 = u0 + t0 <= mask, p1 = u0 + t1 <= mask, p2 = u0 + t2 <= mask, p3 = u0 + t3 <= mask;
    uint4 v0 = {}, v1 = {}, v2 = {}, v3 = {};
    if (p0) v0 = src[(s0 + t0) & mask];
    if (p1) v1 = src[(s0 + t1) & mask];
    if (p2) v2 = src[(s0 + t2) & mask];
    if (p3) v3 = src[(s0 + t3) & mask];
    if (p0) dst[u0 + t0] = v0;
    if (p1) dst[u0 + t1] = v1;
    if (p2) dst[u0 + t2] = v2;
    if (p3) dst[u0 + t3] = v3;
}

__global__ void __launch_bounds__(BLOCK) k_columns_canonical(const uint8_t* __restrict__ cols, size_t n, uint32_t* flags) {
    uint32_t bad = 0;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * BLOCK)
        bad |= !u256_is_canonical_fr(u256_load(cols + 32 * i));
    if (bad) atomicOr(flags, FLAG_NONCANONICAL);
}

}  // namespace h2agg
