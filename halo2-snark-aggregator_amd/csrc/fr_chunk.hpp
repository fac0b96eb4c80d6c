// Chunk geometry of the Fr sweep kernels (poly_kernels.hpp: k_fr_poly_chunk_eval / _divide; prod_kernels.hpp: k_fr_prod_chunk /
// _invert / _scan).  An array is cut into chunks of T = 2^t elements (t = FR_CHUNK_LOG = 11 unless a debug key asks for
// less), one workgroup each: FR_CHUNK_THREADS = 256 threads x FR_CHUNK_PER = 8 consecutive elements in registers.  A smaller
// t leaves the threads from 2^(t - 3) on idle.  The host side of the same geometry is fr_level_plan (fr_host.inc).
#pragma once
#include "fr_fft_kernels.hpp"

namespace h2agg {

constexpr unsigned FR_CHUNK_LOG = 11;      // log2 of the elements per workgroup (default)
constexpr unsigned FR_CHUNK_PER_LOG = 3;   // log2 of the elements per thread
constexpr unsigned FR_CHUNK_PER = 1u << FR_CHUNK_PER_LOG;
constexpr int FR_CHUNK_THREADS = 1 << (FR_CHUNK_LOG - FR_CHUNK_PER_LOG);   // 256

// where a thread stands in chunk c of a level cut with t: threads tid < nthr hold the elements i0 .. i0 + 7
struct FrChunk {
    uint32_t nthr, tid, c, i0;
};

FP_INLINE FrChunk fr_chunk(uint32_t t, uint32_t c) {
    const uint32_t tid = threadIdx.x;
    return {1u << (t - FR_CHUNK_PER_LOG), tid, c, (c << t) + (tid << FR_CHUNK_PER_LOG)};
}

}  // namespace h2agg
