// The lookup argument's permutation for gfx950: the device side of
//   lookup::prover::permute_expression_pair (and the theta-compression in front of it, which is k_fr_poly_lincomb)
//   (halo2_proofs; the crate is an unvendored git dependency of the reference: recalled, DESIGN.md section 2 — the yardstick
//    is the definition in include/h2agg.h.  Which pair a verifier accepts is pinned: lookup.rs:98-113)
//   sort:   u canonical 256-bit keys in ascending order of their integer value, twice per call (a, s)
//   heads:  row i of sorted a is a head if i == 0 or A[i] != A[i - 1]; every head consumes the first occurrence of its value
//           in sorted s, or raises FLAG_NOT_IN_TABLE
//   fill:   ap = A; sp[i] = A[i] on a head, else the leftover of rank (non-heads - 1 - non-heads below i): the unconsumed
//           table rows in ascending order go to the non-head rows from the highest row down
// Keys are moved as they are, 32 bytes little-endian: nothing here multiplies, nothing is in Montgomery form.
//
// Sort plan.  Least-significant-digit radix sort over the 32 bytes of a key, lowest byte first; a pass orders by one byte
// and keeps the order of keys whose byte is equal (the order the earlier passes made), so after byte 31 the keys ascend.
//   k_lk_digit_hist   ONE read of the input: the histogram of every one of the 32 bytes, hist[32][256] (the histogram of a
//                     byte does not depend on the order of the keys).  Checks the keys for < r.  Grid-stride: `hist_lanes`
//                     threads of each of at most `hist grid cap` workgroups take a key per stride.
//   k_lk_plan         from hist: pass p is SKIPPED if one bin holds all u keys (the byte is the same in every key: the pass
//                     would move nothing), and which buffer every pass reads: the keys start in the caller's column (state
//                     0, never written), the first pass that moves writes work buffer 0 (state 1), the next one buffer 1
//                     (state 2), then 0 again.  plan[p] = skip | state << 1; plan[32] = the state behind the last pass.
//                     The decision stays on the device: every kernel of a pass reads plan[p] and returns if it is skipped.
//   per pass p, a workgroup takes a tile of T = 2^t keys, wave w of its four the S = T / 4 consecutive keys
//   [tile T + w S, + S) in rounds of 64 — so "wave-column" col = 4 tile + w covers the keys [col S, col S + S), in order:
//   k_lk_tile_hist    counts[d][col] = the keys of the column whose byte is d        (matrix [256][ncols], ncols = 4 tiles)
//   k_lk_scan_rows    row d: exclusive prefix over the columns, plus the bin's base sum_{e < d} hist[p][e]: counts[d][col]
//                     becomes the position of the column's first key with byte d.  One workgroup walks a row in steps of
//                     `step` entries and carries the sum from step to step.
//   k_lk_scatter      a wave walks its keys in order; in a round the lanes with the same byte find one another with 8
//                     ballots (peers), a lane's position is counts[d][col] + (keys with byte d in earlier rounds) + (peers
//                     in lower lanes); the lowest peer adds the peer count to the running offset behind a barrier.
// The offset arithmetic is restated in tests/lookup_permute_ref.py (radix_pass_py: same tile, column, bin and scan layout)
// and compared with sorted() by the CPU suite.  A position is < u because the counts of a pass are taken from the very keys
// the scatter then moves (same buffer, same columns) and sum to u; the scatter checks it all the same before it stores.
// The u32 prefix sums behind the sort (non-head rows, unconsumed table rows) are two-level: k_lk_block_reduce per tile,
// k_lk_scan_rows over the tile sums (one workgroup), k_lk_block_scan per tile.
//
// Geometry (LkGeom, chosen on the host from the tile, lookup.inc lk_geom).  At the default tile the scan takes 1024 entries
// per step and the byte histogram runs 256 threads in at most 1024 workgroups, so a second scan step needs more than 1024
// wave-columns (u > 2^19) or tiles (u > 2^21) and a second stride u > 2^18.  Under the debug key fr_sort_tile (t < 11) all three
// shrink with the tile — step = hist_lanes = T / 4, at most 2 workgroups — so that inputs of 65 .. 1024 rows walk the step loop
// of both scans and the stride loop several times (t = 4, u = 65: 5 steps over the count matrix, 2 over the tile sums, 9 strides).
//
// Batch.  A launch carries a second grid dimension.  The sort kernels take blockIdx.y as the SORT COLUMN c of a chunk of nb
// lookups: c < nb is the input column of lookup c, nb + c' the table column of lookup c'; every column has its own histograms,
// plan, count matrix and pair of work buffers, slabs addressed base + c * stride in size_t (lk_sort_column).  Indices inside a
// column stay the 32-bit values of one column (< u < 2^24).  Every kernel reads its own column's plan word, so in one launch a
// column that skips a pass returns beside a column that moves, and each column ends in its own buffer state plan[32].  The
// rank kernels take blockIdx.y as the LOOKUP b: marks and prefixes are dense [nb][u] / [nb][u + 1], tile sums [nb][tiles].
// A kernel that raises a status bit also ORs it into status[lookup] where the chunk has such words (null: a single call).
// A single call is the chunk of one lookup (gridDim.y = 2 for its two sorts, 1 for the rank step).
#pragma once
#include "poly_kernels.hpp"

namespace h2agg {

// the fourth device status bit (batch_kernels.hpp has the first three): a head of sorted a does not occur in s[0 .. u)
enum : uint32_t { FLAG_NOT_IN_TABLE = 8u };
static_assert((FLAG_NOT_IN_TABLE & (FLAG_NONCANONICAL | FLAG_DIV_ZERO | FLAG_BAD_POINT)) == 0, "status bits must be disjoint");

constexpr unsigned LK_TILE_LOG = 11;       // log2 of the keys per workgroup (default)
constexpr unsigned LK_TILE_LOG_MIN = 4;    // smallest the debug key fr_sort_tile takes: 16 keys, 4 per wave
constexpr int LK_THREADS = 256;            // four waves of 64
constexpr uint32_t LK_WAVES = 4, LK_BINS = 256, LK_PASSES = 32;
constexpr uint32_t LK_PLAN_WORDS = LK_PASSES + 1;
constexpr uint32_t LK_SCAN_STEP = 4u * LK_THREADS;   // entries of a row per step of k_lk_scan_rows (default)
constexpr uint32_t LK_HIST_GRID = 1024;              // most workgroups of k_lk_digit_hist (default)
static_assert(LK_THREADS == 64 * LK_WAVES && LK_THREADS == (int)LK_BINS, "one thread per bin, four waves of 64");

struct FrSortArgs {
    const uint8_t* in;       // [u] the callers' columns: state 0, read only.  Sort column c < nb: in + c in_stride;
    const uint8_t* in2;      //     c >= nb: in2 + (c - nb) in_stride
    uint8_t* w0;             // [u] work buffers: states 1 and 2; column c at + c key_stride
    uint8_t* w1;
    uint32_t* hist;          // [32][256] byte histograms of the keys (zeroed in front of k_lk_digit_hist); column c at + c 8192
    uint32_t* plan;          // [33] (file header); column c at + c 33
    uint32_t* counts;        // [256][ncols]; column c at + c 256 ncols
    uint32_t* flags;
    uint32_t* status;        // [nb] one word per lookup, or null
    size_t in_stride;        // bytes between the callers' columns
    size_t key_stride;       // bytes between the work buffers of two sort columns (>= 32 u)
    uint32_t nb;             // lookups of the chunk: gridDim.y <= 2 nb sort columns
    uint32_t u;              // keys, 1 .. 2^24 - 1
    uint32_t t;              // log2 T, LK_TILE_LOG_MIN .. LK_TILE_LOG
    uint32_t ncols;          // 4 * ceil(u / T)
    uint32_t pass;           // 0 .. 31
    uint32_t hist_lanes;     // threads of a workgroup of k_lk_digit_hist that take keys: 1 .. 256 (LkGeom)
};

FP_INLINE const uint8_t* lk_state_buf(const uint8_t* in, const uint8_t* w0, const uint8_t* w1, uint32_t state) {
    return state == 0 ? in : state == 1 ? w0 : w1;
}
// byte p of key i: one 4-byte load (no dynamically indexed register array).  i < u.
FP_INLINE uint32_t lk_digit(const uint8_t* keys, uint32_t i, uint32_t p) {
    return (reinterpret_cast<const uint32_t*>(keys)[8 * (size_t)i + (p >> 2)] >> (8 * (p & 3))) & 0xffu;
}
// The arguments of sort column blockIdx.y: every pointer moved to the column's own slab (file header, "Batch"); status moved to
// the word of the column's lookup.  c < 2 nb <= 2048, strides in size_t.
FP_INLINE FrSortArgs lk_sort_column(FrSortArgs a) {
    const uint32_t c = blockIdx.y, b = c < a.nb ? c : c - a.nb;
    a.in = (c < a.nb ? a.in : a.in2) + (size_t)b * a.in_stride;
    a.w0 += (size_t)c * a.key_stride;
    a.w1 += (size_t)c * a.key_stride;
    a.hist += (size_t)c * (LK_PASSES * LK_BINS);
    a.plan += (size_t)c * LK_PLAN_WORDS;
    a.counts += (size_t)c * LK_BINS * a.ncols;
    if (a.status) a.status += b;
    return a;
}
FP_INLINE void lk_raise(uint32_t* flags, uint32_t* status, uint32_t bit) {
    atomicOr(flags, bit);
    if (status) atomicOr(status, bit);
}
FP_INLINE void u256_store(void* p, const U256& v) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
    q[1] = make_uint4(v.w[4], v.w[5], v.w[6], v.w[7]);
}
FP_INLINE bool lk_less(const U256& a, const U256& b) {   // a < b as 256-bit integers
    bool lt = false, decided = false;
#pragma unroll
    for (int j = 7; j >= 0; --j) {
        if (!decided && a.w[j] != b.w[j]) {
            lt = a.w[j] < b.w[j];
            decided = true;
        }
    }
    return lt;
}
FP_INLINE bool lk_equal(const U256& a, const U256& b) {
    uint32_t d = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) d |= a.w[j] ^ b.w[j];
    return d == 0;
}

// Exclusive prefix of v over the 256 threads of a workgroup; total: the sum of all.  lds: LK_WAVES words.  Ends behind a
// barrier, so lds can be used again at once.
FP_INLINE uint32_t lk_block_excl_scan(uint32_t v, uint32_t* lds, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, 64);
        if (lane >= (uint32_t)o) incl += up;
    }
    if (lane == 63u) lds[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < LK_WAVES; ++w) {
        const uint32_t s = lds[w];
        if (w < wave) before += s;
        total += s;
    }
    __syncthreads();
    return before + incl - v;
}

// hist[p][d] += the keys in[0 .. u) whose byte p is d, for all 32 bytes.  Thread x < hist_lanes of workgroup b takes the keys
// b hist_lanes + x + j gridDim.x hist_lanes, j = 0, 1, .. (every key below u exactly once; i < u < 2^24 and the stride is at
// most 2^18: no overflow); the other threads only help with the LDS.  LDS and hist indices 256 p + d < 8192.  Reads in, adds to
// hist (zeroed by the host's memset on the same stream).
__global__ void __launch_bounds__(LK_THREADS) k_lk_digit_hist(const FrSortArgs a0) {
    const FrSortArgs a = lk_sort_column(a0);
    __shared__ uint32_t h[LK_PASSES * LK_BINS];
    for (uint32_t j = threadIdx.x; j < LK_PASSES * LK_BINS; j += LK_THREADS) h[j] = 0;
    __syncthreads();
    bool bad = false;
    const uint32_t stride = gridDim.x * a.hist_lanes;
    for (uint32_t i = threadIdx.x < a.hist_lanes ? blockIdx.x * a.hist_lanes + threadIdx.x : a.u; i < a.u; i += stride) {
        const U256 x = u256_load(a.in + 32 * (size_t)i);
        bad |= !u256_is_canonical_fr(x);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
#pragma unroll
            for (int b = 0; b < 4; ++b) atomicAdd(&h[(4 * j + b) * LK_BINS + ((x.w[j] >> (8 * b)) & 0xffu)], 1u);
        }
    }
    if (bad) lk_raise(a.flags, a.status, FLAG_NONCANONICAL);
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < LK_PASSES * LK_BINS; j += LK_THREADS) {
        const uint32_t v = h[j];
        if (v) atomicAdd(&a.hist[j], v);
    }
}

// One workgroup per sort column (grid 1 x columns).  Reads hist[32][256], writes plan[0 .. 32] (file header).
__global__ void __launch_bounds__(LK_THREADS) k_lk_plan(const FrSortArgs a0) {
    const FrSortArgs a = lk_sort_column(a0);
    uint32_t state = 0;
#pragma unroll 1
    for (uint32_t p = 0; p < LK_PASSES; ++p) {
        const int uniform = __syncthreads_or(a.hist[p * LK_BINS + threadIdx.x] == a.u);
        if (threadIdx.x == 0) a.plan[p] = (uniform ? 1u : 0u) | (state << 1);
        if (!uniform) state = state == 1 ? 2u : 1u;
    }
    if (threadIdx.x == 0) a.plan[LK_PASSES] = state;
}

// where a thread stands in a pass: wave-column col = 4 blockIdx.x + wave holds the keys [first, first + S), S = T / 4; round
// r gives lane l the key first + 64 r + l if 64 r + l < S and the key is < u.  rounds = ceil(S / 64) is the same for every
// thread, so the barriers inside the round loops are uniform.  first + 64 r + l < gridDim.x T + T <= 2^24 + 2^12: no overflow.
struct LkLane {
    uint32_t lane, wave, col, first, S, rounds;
};
FP_INLINE LkLane lk_lane(uint32_t t) {
    LkLane g;
    g.lane = threadIdx.x & 63u;
    g.wave = threadIdx.x >> 6;
    g.S = 1u << (t - 2);
    g.col = LK_WAVES * blockIdx.x + g.wave;
    g.first = g.col * g.S;
    g.rounds = g.S <= 64u ? 1u : g.S >> 6;
    return g;
}

// counts[d][col] for the four columns of this tile, all 256 d (zeros included: the matrix needs no clearing).
// Indices: keys < u; counts index d ncols + col < 256 ncols as col < 4 gridDim.x = ncols.  Reads the pass's source buffer.
__global__ void __launch_bounds__(LK_THREADS) k_lk_tile_hist(const FrSortArgs a0) {
    const FrSortArgs a = lk_sort_column(a0);
    const uint32_t pw = a.plan[a.pass];
    if (pw & 1u) return;
    const uint8_t* src = lk_state_buf(a.in, a.w0, a.w1, pw >> 1);
    __shared__ uint32_t cnt[LK_WAVES][LK_BINS];
    const LkLane g = lk_lane(a.t);
    for (uint32_t d = g.lane; d < LK_BINS; d += 64u) cnt[g.wave][d] = 0;
    __syncthreads();
#pragma unroll 1
    for (uint32_t r = 0; r < g.rounds; ++r) {
        const uint32_t j = 64u * r + g.lane, i = g.first + j;
        if (j < g.S && i < a.u) atomicAdd(&cnt[g.wave][lk_digit(src, i, a.pass)], 1u);
    }
    __syncthreads();
    for (uint32_t d = g.lane; d < LK_BINS; d += 64u) a.counts[(size_t)d * a.ncols + g.col] = cnt[g.wave][d];
}

// Row `blockIdx.x` of data[rows][ncols] -> its exclusive prefix sums plus a base, in place.  hist != null (the count matrix
// of a pass: 256 rows): base = sum_{e < row} hist[256 pass + e], and the launch returns if plan says the pass is skipped;
// hist == null: base 0 (the tile sums of a u32 prefix sum: one row).  A step covers the entries [start, start + step), step a
// multiple of 4 in 4 .. 1024: thread x < step / 4 holds the 4 consecutive entries from start + 4 x (the other threads hold
// zeros and store nothing), all loaded before the first store of the step; the sum of a step is carried into the next.
// Indices: entry e < ncols only, and inside the step.  With hist, blockIdx.y is the sort column: its matrix, histograms and plan
// are the column's slabs (FrSortArgs); without, the rows of the launch are the lookups' tile sums [gridDim.x][ncols].
__global__ void __launch_bounds__(LK_THREADS) k_lk_scan_rows(uint32_t* data, uint32_t ncols, const uint32_t* hist,
                                                              const uint32_t* plan, uint32_t pass, uint32_t step) {
    if (hist) {
        data += (size_t)blockIdx.y * LK_BINS * ncols;
        hist += (size_t)blockIdx.y * (LK_PASSES * LK_BINS);
        plan += (size_t)blockIdx.y * LK_PLAN_WORDS;
    }
    if (plan && (plan[pass] & 1u)) return;
    __shared__ uint32_t lds[LK_WAVES];
    uint32_t carry = 0, total;
    if (hist) {
        (void)lk_block_excl_scan(threadIdx.x < blockIdx.x ? hist[pass * LK_BINS + threadIdx.x] : 0u, lds, total);
        carry = total;
    }
    uint32_t* row = data + (size_t)blockIdx.x * ncols;
    const bool mine = 4u * threadIdx.x < step;
#pragma unroll 1
    for (uint32_t start = 0; start < ncols; start += step) {
        const uint32_t e = start + 4u * threadIdx.x;
        uint32_t v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = mine && e + q < ncols ? row[e + q] : 0u;
        uint32_t run = carry + lk_block_excl_scan(v[0] + v[1] + v[2] + v[3], lds, total);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (mine && e + q < ncols) row[e + q] = run;
            run += v[q];
        }
        carry += total;
    }
}

// Moves the keys of the pass.  Reads the source buffer and the scanned counts; writes the other work buffer: positions
// < u (file header), checked.  off[wave][d]: where the wave's next key with byte d goes.  A round: every lane reads its
// offset; barrier; the lowest lane of every group of peers advances the group's offset; barrier.
__global__ void __launch_bounds__(LK_THREADS) k_lk_scatter(const FrSortArgs a0) {
    const FrSortArgs a = lk_sort_column(a0);
    const uint32_t pw = a.plan[a.pass];
    if (pw & 1u) return;
    const uint32_t state = pw >> 1;
    const uint8_t* src = lk_state_buf(a.in, a.w0, a.w1, state);
    uint8_t* dst = state == 1 ? a.w1 : a.w0;
    __shared__ uint32_t off[LK_WAVES][LK_BINS];
    const LkLane g = lk_lane(a.t);
    for (uint32_t d = g.lane; d < LK_BINS; d += 64u) off[g.wave][d] = a.counts[(size_t)d * a.ncols + g.col];
    __syncthreads();
    const uint64_t below = ((uint64_t)1 << g.lane) - 1u;
#pragma unroll 1
    for (uint32_t r = 0; r < g.rounds; ++r) {
        const uint32_t j = 64u * r + g.lane, i = g.first + j;
        const bool act = j < g.S && i < a.u;
        U256 key = {};
        uint32_t d = 0;
        if (act) {
            key = u256_load(src + 32 * (size_t)i);
            d = lk_digit(src, i, a.pass);
        }
        uint64_t peers = __ballot(act);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const uint64_t m = __ballot(act && bit);
            peers &= bit ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & below);
        const uint32_t pos = act ? off[g.wave][d] + rank : 0u;
        __syncthreads();
        if (act && rank == 0) off[g.wave][d] = pos + (uint32_t)__popcll(peers);
        __syncthreads();
        if (act && pos < a.u) u256_store(dst + 32 * (size_t)pos, key);
    }
}

// sums[b] = the sum of src[bT .. bT + T) below n.  A thread adds 8 consecutive entries (threads >= T / 8 idle).
// Indices: src index < n; sums index blockIdx.x < gridDim.x = ceil(n / T).  blockIdx.y = lookup: src [.][n], sums [.][gridDim.x].
__global__ void __launch_bounds__(LK_THREADS) k_lk_block_reduce(const uint32_t* src, uint32_t* sums, uint32_t n, uint32_t t) {
    __shared__ uint32_t lds[LK_WAVES];
    src += (size_t)blockIdx.y * n;
    sums += (size_t)blockIdx.y * gridDim.x;
    const uint32_t i0 = (blockIdx.x << t) + 8u * threadIdx.x;
    uint32_t s = 0;
    if (8u * threadIdx.x < (1u << t)) {
#pragma unroll
        for (int e = 0; e < 8; ++e) s += i0 + e < n ? src[i0 + e] : 0u;
    }
    uint32_t total;
    (void)lk_block_excl_scan(s, lds, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// dst[i] = sum of src[0 .. i), i <= n: the tile's exclusive prefix on top of sums[b] (the scanned tile sums); the thread that
// holds entry n - 1 also stores dst[n], the total.  dst has n + 1 entries and is not src.  blockIdx.y = lookup: src [.][n],
// sums [.][gridDim.x], dst [.][n + 1].
__global__ void __launch_bounds__(LK_THREADS) k_lk_block_scan(const uint32_t* src, const uint32_t* sums, uint32_t* dst, uint32_t n,
                                                               uint32_t t) {
    __shared__ uint32_t lds[LK_WAVES];
    src += (size_t)blockIdx.y * n;
    sums += (size_t)blockIdx.y * gridDim.x;
    dst += (size_t)blockIdx.y * ((size_t)n + 1);
    const uint32_t i0 = (blockIdx.x << t) + 8u * threadIdx.x;
    const bool mine = 8u * threadIdx.x < (1u << t);
    uint32_t v[8], s = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        v[e] = mine && i0 + e < n ? src[i0 + e] : 0u;
        s += v[e];
    }
    uint32_t total;
    uint32_t run = sums[blockIdx.x] + lk_block_excl_scan(s, lds, total);
    if (!mine) return;   // (behind the last barrier)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if (i0 + e < n) dst[i0 + e] = run;
        run += v[e];
        if (i0 + e + 1 == n) dst[n] = run;
    }
}

struct FrLookupPermuteArgs {
    const uint8_t* a_in;     // the sorted columns: the three buffers of each sort and its plan (plan[32]: which one)
    const uint8_t* a_w0;
    const uint8_t* a_w1;
    const uint32_t* a_plan;
    const uint8_t* s_in;
    const uint8_t* s_w0;
    const uint8_t* s_w1;
    const uint32_t* s_plan;
    uint32_t* non_head;      // [u] 1 where row i of sorted a is not a head
    uint32_t* left;          // [u] 1 where row q of sorted s is not consumed (set to 1 in front of k_lk_heads)
    uint32_t* non_head_pre;  // [u + 1] exclusive prefix of non_head, [u] the total
    uint32_t* left_pre;      // [u + 1] the same of left
    uint32_t* left_idx;      // [u] left_idx[j] = the row of sorted s that is the j-th leftover
    uint8_t* ap;             // [u]
    uint8_t* sp;             // [u]
    uint32_t* flags;
    uint32_t* status;        // [lookups] or null
    size_t col_stride;       // bytes between the lookups' columns of a_in, s_in, ap, sp
    size_t key_stride;       // ... of a_w0, a_w1, s_w0, s_w1
    uint32_t u;
};

// The arguments of lookup blockIdx.y (file header, "Batch"): the callers' columns by col_stride, the work buffers by key_stride,
// the plans by 33 words, the marks by u words, the prefixes by u + 1.
FP_INLINE FrLookupPermuteArgs lk_permute_lookup(FrLookupPermuteArgs p) {
    const size_t b = blockIdx.y;
    p.a_in += b * p.col_stride;
    p.s_in += b * p.col_stride;
    p.ap += b * p.col_stride;
    p.sp += b * p.col_stride;
    p.a_w0 += b * p.key_stride;
    p.a_w1 += b * p.key_stride;
    p.s_w0 += b * p.key_stride;
    p.s_w1 += b * p.key_stride;
    p.a_plan += b * LK_PLAN_WORDS;
    p.s_plan += b * LK_PLAN_WORDS;
    p.non_head += b * p.u;
    p.left += b * p.u;
    p.left_idx += b * p.u;
    p.non_head_pre += b * ((size_t)p.u + 1);
    p.left_pre += b * ((size_t)p.u + 1);
    if (p.status) p.status += b;
    return p;
}

// Row i < u of sorted a: head or not; a head finds the first row of sorted s that is >= its value (binary search: lo, mid < u)
// and clears left[] there if the values are equal — different heads have different values, so different rows — or raises
// FLAG_NOT_IN_TABLE.  Reads both sorted columns; writes non_head[i], left[lo].
__global__ void __launch_bounds__(BLOCK) k_lk_heads(const FrLookupPermuteArgs p0) {
    const FrLookupPermuteArgs p = lk_permute_lookup(p0);
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= p.u) return;
    const uint8_t* A = lk_state_buf(p.a_in, p.a_w0, p.a_w1, p.a_plan[LK_PASSES]);
    const uint8_t* S = lk_state_buf(p.s_in, p.s_w0, p.s_w1, p.s_plan[LK_PASSES]);
    const U256 x = u256_load(A + 32 * (size_t)i);
    const bool head = i == 0 || !lk_equal(x, u256_load(A + 32 * (size_t)(i - 1)));
    p.non_head[i] = head ? 0u : 1u;
    if (!head) return;
    uint32_t lo = 0, hi = p.u;
#pragma unroll 1
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (lk_less(u256_load(S + 32 * (size_t)mid), x)) lo = mid + 1;
        else hi = mid;
    }
    if (lo < p.u && lk_equal(u256_load(S + 32 * (size_t)lo), x)) p.left[lo] = 0u;
    else lk_raise(p.flags, p.status, FLAG_NOT_IN_TABLE);
}

// left_idx[left_pre[q]] = q for every unconsumed row q < u of sorted s.  left_pre[q] < left_pre[u] <= u.
__global__ void __launch_bounds__(BLOCK) k_lk_leftovers(const FrLookupPermuteArgs p0) {
    const FrLookupPermuteArgs p = lk_permute_lookup(p0);
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= p.u) return;
    const uint32_t j = p.left_pre[q];
    if (p.left_pre[q + 1] != j && j < p.u) p.left_idx[j] = q;
}

// ap[i] = A[i]; sp[i] = A[i] on a head, else the leftover of rank j = non-heads - 1 - (non-heads below i).  j < leftovers
// whenever every head was found (then leftovers = non-heads); checked, as is the row read from left_idx, so a call that
// raised FLAG_NOT_IN_TABLE stays inside its buffers (its outputs are unspecified).  Writes only ap[i] and sp[i], i < u.
__global__ void __launch_bounds__(BLOCK) k_lk_fill(const FrLookupPermuteArgs p0) {
    const FrLookupPermuteArgs p = lk_permute_lookup(p0);
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= p.u) return;
    const uint8_t* A = lk_state_buf(p.a_in, p.a_w0, p.a_w1, p.a_plan[LK_PASSES]);
    const uint8_t* S = lk_state_buf(p.s_in, p.s_w0, p.s_w1, p.s_plan[LK_PASSES]);
    const U256 x = u256_load(A + 32 * (size_t)i);
    U256 y = x;
    const uint32_t below = p.non_head_pre[i];
    if (p.non_head_pre[i + 1] != below) {
        const uint32_t j = p.non_head_pre[p.u] - 1u - below;
        if (j < p.left_pre[p.u]) {
            const uint32_t q = p.left_idx[j];
            if (q < p.u) y = u256_load(S + 32 * (size_t)q);
        }
    }
    u256_store(p.ap + 32 * (size_t)i, x);
    u256_store(p.sp + 32 * (size_t)i, y);
}

// The descriptor k_fr_poly_lincomb reads for one group of m polynomials, first one under the highest power: list = 0 .. m - 1,
// then goff = {0, m}.  desc has m + 2 words.
__global__ void __launch_bounds__(BLOCK) k_lk_compress_desc(uint32_t* desc, uint32_t m) {
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < m + 2u; i += gridDim.x * BLOCK) desc[i] = i < m ? i : i == m ? 0u : m;
}

}  // namespace h2agg
