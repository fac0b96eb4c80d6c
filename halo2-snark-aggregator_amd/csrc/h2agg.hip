// libh2agg.so — context management and the C ABI declared in include/h2agg.h.
// Everything numeric runs in the HIP kernels of batch_kernels.hpp / msm_kernels.hpp; there is no CPU
// arithmetic path in this library (a context cannot be created without a HIP device).
#include "../../include/h2agg.h"

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <cassert>
#include <csignal>
#include <dlfcn.h>
#include <unistd.h>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <sched.h>
#include <sys/resource.h>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "scalar_mul_kernels.hpp"
#include "lp_kernels.hpp"
#include "seg_msm_kernels.hpp"
#include "g1_fft_kernels.hpp"
#include "fr_fft_kernels.hpp"
#include "poly_kernels.hpp"
#include "prod_kernels.hpp"
#include "lookup_kernels.hpp"
#include "quotient_kernels.hpp"
#include "keygen_kernels.hpp"
#include "pairing.hpp"
#if !defined(__HIP_DEVICE_COMPILE__) && defined(__x86_64__)
// the same pairing once more, compiled for BMI2 + ADX (csrc/pairing.hpp's header): taken when the CPU has both
#define H2AGG_PAIRING_ADX_BUILD 1
#define PAIRING_NS pairing_adx
#define PAIRING_ADX 1
#pragma clang attribute push(__attribute__((target("bmi2,adx"))), apply_to = function)
#include "pairing.hpp"
#pragma clang attribute pop
#undef PAIRING_NS
#undef PAIRING_ADX
#endif
#include "poseidon_host.hpp"
#include "poseidon_sponge_host.hpp"
#include "poseidon_ifma_host.hpp"
#include "poseidon_kernels.hpp"
#include "hash_transcript_host.hpp"
#include "hash_transcript_kernels.hpp"

using namespace h2agg;

namespace {

// Experiment switches (occupancy caps, kernel variants, priorities, fault injection ...) exist only in a library built with
// -DH2AGG_MEASURE_KNOBS (tools/ and profiles/ say which runs used one).  A shipped library reads the environment for
// nothing but what include/h2agg.h documents under "Environment": H2AGG_HOST_THREADS, H2AGG_TRANSCRIPT, H2AGG_HOST_SPONGE,
// H2AGG_NO_PLACE, H2AGG_TRACE, H2AGG_TRACE_PHASES.  Per-call test hooks go through h2agg_debug_configure.
#ifdef H2AGG_MEASURE_KNOBS
static inline const char* knob(const char* name) { return getenv(name); }
#else
static inline const char* knob(const char*) { return nullptr; }
#endif
// Events that only order streams of this device / time kernels on it: device-scope release.  (The default is a system-scope
// release — an L2 write-back at every record.)  H2AGG_EVENT_SCOPE=system (a measure knob) restores the default for A/B runs.
static const bool ev_scope_system = knob("H2AGG_EVENT_SCOPE") && !strcmp(knob("H2AGG_EVENT_SCOPE"), "system");
#define EV_SYNC_FLAGS (ev_scope_system ? hipEventDisableTiming : (hipEventDisableTiming | hipEventReleaseToDevice))
#define EV_TIME_FLAGS (ev_scope_system ? hipEventDefault : hipEventReleaseToDevice)

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

enum Stage {
    ST_PART_COUNT = 0, ST_PART_SCATTER, ST_BUCKET_SORT, ST_ORDER, ST_ACCUM, ST_ACCUM_BIG, ST_REDUCE, ST_WINDOW_SUM,
    ST_FINAL, ST_N
};
const char* const STAGE_NAMES[ST_N] = {"msm_part_count", "msm_part_scatter",   "msm_bucket_sort",
                                       "msm_order",      "msm_accumulate",     "msm_accumulate_big",
                                       "msm_reduce",     "msm_window_sum",     "msm_final"};

struct Table {
    uint8_t* d = nullptr;       // Montgomery affine, 64 B / point
    uint8_t* endo_x = nullptr;  // beta * x, 32 B / point (made on the first GLV MSM over this table)
    size_t n = 0;
    // the call that wrote the table stored no identity base (flags[1], batch_kernels.hpp): MSMs over it take the bucket
    // accumulation without the per-entry identity test.  false = not known: "may hold one" (msm_lean_variant)
    bool no_identity = false;
    // fixed-base levels (h2agg_bases_precompute): pre[(w * n + i) * 64] = 2^(pre_c * w) * P_i, w < pre_W
    uint8_t* pre = nullptr;
    int pre_c = 0, pre_W = 0;
    // comb of the first comb_n bases (k_comb_table_build with bases; made on the first small MSM over a table that has
    // fixed-base levels, i.e. one its owner declared constant): comb[((b * 32 + w) * 255 + d - 1) * 64] = d * 2^(8w) * P_b
    uint8_t* comb = nullptr;
    size_t comb_n = 0;
    std::vector<uint8_t*> comb_retired;   // smaller combs this one replaced: kernels in flight may still read them, so they
                                          // are freed where the table's other buffers are (behind a synchronisation)
    void free_combs() {
        if (comb) hipFree(comb);
        for (uint8_t* p : comb_retired) hipFree(p);
        comb = nullptr;
        comb_n = 0;
        comb_retired.clear();
    }
};
struct PreTable {   // what msm_run needs of it
    const uint8_t* d;
    size_t n_level;
    int c, W;
};

// ---- the plain data of msm_run (csrc/msm_run.inc has the functions; the context below keeps a deferred tail by value)
// Slices of ONE MSM that share a bucket set (an MSM is a sum over points: the slices' bucket sums just add up, so only
// the last slice needs the bucket reduction / window sums / Horner tail — one latency chain per MSM instead of one per
// slice).  CHAIN_FIRST / CHAIN_MID: sort + accumulation only, the tail slot does not rotate; CHAIN_LAST: accumulation
// on top of what the slot holds, then the tail.
enum { CHAIN_OFF = 0, CHAIN_FIRST = 1, CHAIN_MID = 2, CHAIN_LAST = 3 };

struct MsmCall {   // the argument of msm_run (described there)
    const uint8_t* d_bases = nullptr;
    const uint8_t* d_scalars = nullptr;
    size_t n_base = 0;
    uint8_t* d_out_jac = nullptr;
    uint32_t batch = 1;
    const uint8_t* d_endo_x = nullptr;
    const PreTable* pre = nullptr;
    uint32_t split = 0;
    bool no_identity = false;
    int chain = CHAIN_OFF;    // ignored with batch != 1 or fixed-base levels
    size_t chain_n = 0;       // the point count a chain's plan is made for (every slice the same plan)
    bool chain_glv = false;   // a chain's endomorphism split
};

enum class SortKind {
    SMALL,         // one launch (k_small_sort)
    FB_LEVELS,     // the (level, point) sort of fixed-base levels at c = 20 (fb_sort_kernels.hpp)
    DIGIT_MAJOR,   // 16- / 17-bit windows over one table, 2^16 .. 2^22 keys per window (k_dm_*)
    PACKED,        // two levels over packed (sub-bucket | index) items, level 2 staged in LDS
    PACKED_L1,     // ... level 1 staged as well (h2agg_msm_configure_sort stage_l1)
    TWO_ARRAY      // two levels, index and sub-bucket in arrays of their own (the index does not fit the packed item)
};
enum class TailKind {
    FB_GRIDS,   // fixed-base levels: one set of 2^19 buckets as 16 grids
    R2D7,       // two-dimensional reduction, 16-bit windows
    R2D8,       // ... 17-bit windows
    SEGMENTS    // segment sums + window sums
};

// Every decision of one call (msm_route): a function of the call and of the context's configuration alone.
struct MsmRoute {
    int refuse_code;           // != H2AGG_OK: the call is refused with refuse_msg, nothing else is valid
    const char* refuse_msg;
    uint32_t batch, split;     // MSMs in the set of launches (a split MSM: 2); the split point or 0
    int chain;                 // CHAIN_*
    size_t n_base, n, nent;    // bases; scalars; bucket insertions
    MsmPlan p;
    int Wd, W1;                // digit positions per scalar; windows (bucket sets) per MSM
    uint32_t WT;               // windows in total
    SortKind sort;
    SortPlan sp;
    DmPlan dp;
    bool dm17;                 // digit-major at c = 17
    uint32_t dm_nwin, fb_ntile;
    unsigned ntiles;
    int idx_bits;
    size_t tile_counts_bytes;
    bool glv_here, endo_here;  // this call decomposes its scalars / makes the beta * x column
    bool ordered;              // buckets are taken in the order of their lengths
    uint32_t lpb;              // lanes per bucket
    bool lean, lean_dual;
    int lean_var;
    bool big_possible;
    size_t max_slots, max_keys;
    TailKind tail;
    bool par4;
    uint32_t nseg_total;
    // streams: the accumulation leaves the context's stream; sort outputs alternate; the over-long-bucket kernels go in front
    // of the tail; the whole tail / its last chain leaves the accumulation's stream; the tail waits for the next call
    bool piped, altbuf, tail_big, tails_off_stream, final_off_stream, defer;
};

// The buffers of one call (msm_bind): sort slot sq, tail slot par, as they were when the call was made.
struct MsmWorkspace {
    int sq, par;
    bool meta_was_clean;
    uint32_t *meta, *pcount, *pstart, *pcursor, *bin_count, *bin_start, *bin_cursor, *big_count;
    uint32_t *hist, *offs, *order, *entries, *item_idx, *fb_long, *tile_counts;
    uint16_t* item_sub;
    uint32_t *big_list, *big_keys, *fix_list, *ticket;
    uint8_t *big_part, *acc_out, *buckets, *segsum, *wsum, *res_xyzz;
    const uint8_t *d_bases, *d_scalars, *d_endo_x;
    uint8_t* d_out_jac;
};

struct MsmTailJob {   // a tail that waits for the next call: everything msm_tail needs
    MsmRoute r;
    MsmWorkspace w;
    hipStream_t from;   // the accumulation's stream
};
static_assert(std::is_trivially_copyable<MsmTailJob>::value, "a deferred tail is kept and copied as plain data");

}  // namespace

constexpr int MSM_MAX_SLICES = 16;

struct h2agg_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    std::string desc;
    int cu_count = 0;

    // grow-only device workspace
    DevBuf in_a, in_b, in_c, out, tmp_bases;                      // host-buffer entry points
    DevBuf comb;                                                  // fixed-base comb table of the generator (k_comb_table_build)
    bool comb_ready = false;
    // transcript side (csrc/transcript.inc): Poseidon constants as device registers; staging of proofs / items; the
    // decompressed points, element streams and challenges of the last transcript batch
    DevBuf psd_spec, tr_in, tr_points, tr_elems, tr_chal;
    bool psd_ready = false;
    int cfg_transcript = 0;            // sponge backend: 0 = auto, 1 = device, 2 = host threads (h2agg_transcript_configure)
    std::vector<uint8_t> h_elems;      // element streams downloaded for the host backend
    // verifier pipeline (csrc/verifier.inc): instance values / commitments of a circuit's proofs, the aggregation transcript
    DevBuf inst_vals, inst_jac, inst_aff, agg_elems;
    DevBuf hist[2], offs[2], pmeta[2], order[2], entries[2];   // what the accumulation reads: one set per sort slot (overlap level 3)
    DevBuf big_list[2], big_keys[2], big_part[2];              // written by the accumulation, read by the over-long-bucket kernels
    DevBuf fix_list[2];                                        // buckets the lean accumulation left to the general formulas
    bool meta_clean[2] = {};                                   // pmeta[q] was zeroed behind its last use (tail stream)
    DevBuf item_idx, item_sub,
        glv_buf, parts, small, endo_buf, tile_counts, fb_long;  // MSM (bulk side: main stream only)
    uint32_t* d_flags = nullptr;      // in `small`: [0] status flags, [1] big_count
    uint8_t* d_res_xyzz = nullptr;    // in `small` + 1024 + 144 * slot of the LAST msm_run (see msm_run)
    uint8_t* d_res_jac = nullptr;     // in `small` + 256
    uint8_t* h_pinned = nullptr;      // 4 KiB pinned staging for small results / flags

    // schema-layer scratch (grow-only; the schema API is synchronous, one evaluation is in flight per context):
    // the Fr register file, the uploaded staging block, per-side MSM scalars / Montgomery bases, pinned staging
    DevBuf sch_regs, sch_in, sch_scalars[2], sch_bases[2], sch_endo;
    uint8_t* h_stage = nullptr;
    size_t h_stage_cap = 0;
    uint8_t* h_down = nullptr;        // page-locked landing block of the from-bytes call's downloads (csrc/verify_run.inc)
    size_t h_down_cap = 0;
    const void* sch_owner = nullptr;  // the schema whose tape sch_regs reflects
    struct AggPlanCache* agg_plans = nullptr;   // recorded aggregations kept for the next call of the same shape (csrc/verifier.inc)

    // host-buffer MSM: slices are copied on this stream while the previous slice is computed
    hipStream_t copy_stream = nullptr;
    hipStream_t spare_streams[4] = {};   // what place_streams() did not give a role (see there)
    // verifier pipeline: point decompression of a circuit's proofs runs here, beside the instance-column MSMs
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_aux = nullptr, ev_aux_go = nullptr;
    hipEvent_t ev_copy[MSM_MAX_SLICES] = {}, ev_copy_s[MSM_MAX_SLICES] = {}, ev_ready = nullptr;

    std::map<uint64_t, Table> tables;
    uint64_t next_handle = 1;

    // multi-GPU: this context's rank in an RCCL communicator (csrc/comm.inc); ncclComm_t kept opaque here
    void* comm = nullptr;
    int comm_rank = 0, comm_size = 0;

    // h2agg_debug_configure: test hooks read per call (chained host-buffer slices, comb route, plan cache)
    int dbg_pcie_slices = 0, dbg_pcie_glv = 0, dbg_pcie_chain = 1, dbg_comb_msm = 1, dbg_plan_cache = 1, dbg_small_sort = 1, dbg_eval_split = 1, dbg_pre_big = 0, dbg_lean_acc = 1, dbg_shard_fail = 0, dbg_shard_calls = 0, dbg_phases = 0, dbg_tape_lds = 1, dbg_prewake = 1;
    int dbg_lean_full = 0;                  // 1: every bucket accumulation takes the instantiation for any table / any plan
    uint32_t table_word = 0;                // flags[1] as the last finish() read it: the creating call stored an identity base
    int last_lean_variant = -1;             // VAR of the last lean accumulation launched (h2agg_debug_table_identity)
    int dbg_seg_chunk = 0, dbg_seg_c = 0;   // segmented multi_exp: points per set of launches (0 = automatic), window bits (0 = default)
    DevBuf seg_wsum, seg_dev, seg_out;      // segmented multi_exp: window sums, segment offsets, results (csrc/seg_msm.inc)
    // G1 FFT (csrc/params.inc): ladder records of w_K^t, t < 2^(K-1), per direction (0 forward, 1 inverse) for the largest K asked
    // for so far (a smaller k reads them with a stride), and of 1 / 2^k for k <= 24
    DevBuf fft_tw[2], fft_scale;
    int fft_tw_k[2] = {-1, -1};
    bool fft_scale_ready = false;
    // Fr FFT (csrc/fr_fft.inc): the two-level twiddle tables of w_K per direction for the largest K asked for so far, the
    // shift table of the last shifted call, the work array of a multi-pass transform
    DevBuf frfft_tw[2], frfft_shift, frfft_work;
    int frfft_tw_k[2] = {-1, -1};
    int dbg_fr_fft_local = 0;   // debug key fr_fft_local: radix-2 stages fused per pass (0 = FR_FFT_LOCAL)
    int dbg_fr_fft_batch_chunk = 0;   // debug key fr_fft_batch_chunk: columns per set of launches of a batched transform (0 = by the work array)
    // KZG openings (csrc/poly_open.inc): the chunk values of every level above the coefficients, the queries / group lists of
    // the call in progress, the combined polynomials (then their quotients) of a multiopen, its Jacobian commitments
    DevBuf poly_work, poly_desc, poly_slab, poly_jac;
    int dbg_fr_poly_chunk = 0;   // debug key fr_poly_chunk: log2 of the coefficients per workgroup (0 = FR_CHUNK_LOG)
    // grand products (csrc/prod.inc): the num and den columns of a permutation / lookup call (den: then R^2 / den, also for
    // h2agg_fr_grand_product), the chunk products of every level above the elements, the two-level table of w^i
    DevBuf prod_num, prod_den, prod_lvl, prod_tab;
    int dbg_fr_scan_chunk = 0;   // debug key fr_scan_chunk: log2 of the elements per workgroup (0 = FR_CHUNK_LOG)
    // lookup permutation (csrc/lookup.inc): the key buffers, rank columns, count matrix, histograms and plans of a call
    // (lk_layout), the descriptor of a compression
    DevBuf lk_work, lk_desc;
    int dbg_fr_sort_tile = 0;   // debug key fr_sort_tile: log2 of the keys per workgroup (0 = LK_TILE_LOG)
    // quotient polynomial (csrc/quotient.inc): a coset's value slab with the columns behind it and the extended evaluations
    // (qt_layout), the compiled programs and the permutation columns' places, the two-level table of w^i
    DevBuf qt_work, qt_prog, qt_tab;
    // keygen (csrc/keygen.inc): one bit per cell of a permutation's mapping, the table of delta^c, the Jacobian commitments of a
    // slab commit
    DevBuf kg_bitmap, kg_delta, kg_jac;
    int dbg_commit_chunk = 0;   // debug key commit_chunk: columns per set of MSM launches of h2agg_commit_columns (0 = by the work-memory budget)
    std::string last_phases;   // debug key phases: the last h2agg_verify_aggregation's wall-clock split (h2agg_last_phases)
    // tuning
    int cfg_c = 0, cfg_seg = 0, cfg_big = 0, cfg_sub_bits = 0, cfg_tile = 0;
    int cfg_glv = 0;   // 0 = auto, 1 = on, -1 = off
    int cfg_lpb = 0;   // lanes per bucket in the accumulate kernel: 0 = auto, 1 / 2 / 4 / 8 / 16
    bool cfg_no_stage = false, cfg_stage_l1 = false, staged_attr_set = false, cfg_no_dm = false, dm_attr_set = false, r2d_attr_set = false;

    // optional overlap of the serial tail (k_msm_final) of MSM k with the bulk of MSM k+1
    bool tail_overlap = false;
    int overlap_level = 2;  // 1: only the Horner tail on the second stream; 2: reduction + window sums + tail
    // TAIL_SLOTS tail streams used round-robin, each with its own buckets / segsum / wsum set: the latency-shaped
    // tails of consecutive MSMs overlap one another as well as the next MSMs' bulk (small MSMs are otherwise
    // bound by one tail chain: ~0.7 ms per MSM at 2^14 points against 0.5 ms of bulk).
    static constexpr int TAIL_SLOTS = 3;
    // what a tail reads: one independent allocation per slot, so MSMs with DIFFERENT plans (bucket counts, segment
    // counts, window counts) in flight on different slots can never alias one another, whatever their sizes
    DevBuf r2d_ticket[TAIL_SLOTS];
    DevBuf buckets[TAIL_SLOTS], segsum[TAIL_SLOTS], wsum[TAIL_SLOTS];
    hipStream_t tail_streams[TAIL_SLOTS] = {};
    hipEvent_t ev_bulk[TAIL_SLOTS] = {}, ev_tail[TAIL_SLOTS] = {};
    bool tail_pending[TAIL_SLOTS] = {};
    int parity = 0;   // slot of the next MSM
    // called by msm_run on the stream of the accumulation, behind the sort and in front of the first kernel that reads the
    // bases: the host-buffer MSM waits there for the slice's bases (the sort only needs the scalars, which cross PCIe first)
    std::function<int(hipStream_t)> bases_hook;
    // overlap level 3: the bucket accumulation of MSM k runs on its own stream, under the sort of MSM k+1 (which stays on the
    // context's stream, ordered after whatever the caller queued there).  The sort's outputs exist twice.
    // Deferred tail (overlap level >= 2): the tail of MSM k is launched from the NEXT MSM's call, behind that MSM's sort —
    // beside the sort it slows the sort's latency chains by 2x, beside the accumulation it only costs its own instructions.
    // Whoever needs the results first (join_tails) launches it at once.
    MsmTailJob deferred_job;      // valid while tail_deferred (flush_deferred_tail)
    bool tail_deferred = false;
    hipEvent_t ev_sortdone = nullptr;
    hipStream_t acc_stream = nullptr;
    hipEvent_t ev_sorted[2] = {}, ev_accdone[2] = {};
    bool accdone_pending[2] = {};
    int sort_par = 0;

    // profiling: a ring of per-call event sets, harvested lazily so that measuring does not serialise
    // back-to-back asynchronous MSMs
    static constexpr int PROF_RING = 32;
    struct ProfSlot {
        hipEvent_t ev[ST_N][2] = {};
        bool used[ST_N] = {};
        bool pending = false;
    };
    bool profiling = false;
    int prof_only = -1;   // >= 0: only this stage is bracketed (one event pair per MSM instead of nine)
    bool prof_events_created = false;
    ProfSlot prof[PROF_RING];
    int prof_cur = 0;
    double stage_ms[ST_N] = {};
    uint64_t stage_launches[ST_N] = {};
};

namespace {

int fail(h2agg_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

#define HIP_TRY(ctx, expr)                                                                              \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(ctx, H2AGG_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));         \
    } while (0)

int flush_deferred_tail(h2agg_ctx* c, bool behind_sort);

int ensure(h2agg_ctx* c, DevBuf& b, size_t bytes) {
    if (bytes <= b.cap) return H2AGG_OK;
    if (b.p) {
        // a grow-only buffer is replaced: nothing queued on ANY stream of the device may still refer to the old one
        // (nor anything not yet queued: a deferred tail goes out first)
        {
            const int rc_ = flush_deferred_tail(c, false);
            if (rc_ != H2AGG_OK) return rc_;
        }
        HIP_TRY(c, hipDeviceSynchronize());
        HIP_TRY(c, hipFree(b.p));
    }
    b.p = nullptr;
    b.cap = 0;
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) return fail(c, H2AGG_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    b.cap = want;
    return H2AGG_OK;
}

#define TRY(expr)                      \
    do {                               \
        int rc_ = (expr);              \
        if (rc_ != H2AGG_OK) return rc_; \
    } while (0)

int grid_for(const h2agg_ctx* c, size_t n) {
    size_t blocks = (n + BLOCK - 1) / BLOCK;
    size_t cap = (size_t)c->cu_count * 8;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

// d_flags: [0] status of the call in progress, [1] spare, [2] sticky status of earlier asynchronous calls.
// A synchronous entry point starts with clear_flags (which ROLLS [0] into [2], so a flag raised by a preceding
// h2agg_g1_msm_device_async / _batch_async is never lost) and ends with finish (which reports both).
int clear_flags(h2agg_ctx* c) {
    hipLaunchKernelGGL(k_flags_roll, dim3(1), dim3(1), 0, c->stream, c->d_flags);
    return H2AGG_OK;
}

int flags_to_status(h2agg_ctx* c, uint32_t f, bool earlier) {
    const char* pre = earlier ? "an earlier asynchronous call on this context: " : "";
    if (f & FLAG_DIV_ZERO)
        return fail(c, H2AGG_ERR_DIV_ZERO, std::string(pre) + "inversion of zero (reference: invert().unwrap() panics)");
    if (f & FLAG_NONCANONICAL) return fail(c, H2AGG_ERR_NONCANONICAL, std::string(pre) + "input integer >= modulus");
    if (f & FLAG_BAD_POINT) return fail(c, H2AGG_ERR_BAD_POINT, std::string(pre) + "invalid point encoding in proof");
    if (f & FLAG_NOT_IN_TABLE) return fail(c, H2AGG_ERR_NOT_IN_TABLE, std::string(pre) + "a lookup input does not occur in the table");
    if (f & FLAG_BAD_MAPPING)
        return fail(c, H2AGG_ERR_INVALID, std::string(pre) + "the permutation mapping is not valid (a repeated target, an unusable row that moves, an entry out of range)");
    return H2AGG_OK;
}

// synchronise and translate device status flags (this call's, then any left behind by earlier asynchronous calls)
// host_flags: FLAG_* bits raised by host-side halves of the call (the host sponge's canonicity check): merged into the
// call's device flags so that the order of precedence of the errors does not depend on where a check ran
int finish(h2agg_ctx* c, uint32_t host_flags = 0) {
    HIP_TRY(c, hipMemcpyAsync(c->h_pinned + 2048, c->d_flags, 12, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    uint32_t f[3];
    memcpy(f, c->h_pinned + 2048, 12);
    c->table_word = f[1];   // (the base-table word of the call that ends here: h2agg_bases_upload and its kin)
    f[0] |= host_flags;
    if (f[0] | f[2]) HIP_TRY(c, hipMemsetAsync(c->d_flags, 0, 12, c->stream));   // reported once, here
    if (f[0]) return flags_to_status(c, f[0], false);
    return flags_to_status(c, f[2], true);
}

struct StageTimer {
    h2agg_ctx* c;
    int st;
    hipStream_t s;
    StageTimer(h2agg_ctx* c_, int st_, hipStream_t s_ = nullptr) : c(c_), st(st_), s(s_ ? s_ : c_->stream) {
        if (c->profiling && (c->prof_only < 0 || c->prof_only == st)) {
            hipEventRecord(c->prof[c->prof_cur].ev[st][0], s);
        }
    }
    ~StageTimer() {
        if (c->profiling && (c->prof_only < 0 || c->prof_only == st)) {
            hipEventRecord(c->prof[c->prof_cur].ev[st][1], s);
            c->prof[c->prof_cur].used[st] = true;
        }
    }
};

// Debugging aid (H2AGG_BREADCRUMBS=1): the return addresses of the last C-ABI entries (every entry point binds its context
// first) and the sizes of the last MSMs, dumped when the process aborts — the HSA runtime abort()s on a GPU memory fault, long
// after the host call that queued the faulting kernel has returned.  Resolve the addresses against libh2agg.so (they are
// printed relative to its load address).
struct Crumbs {
    static constexpr int N = 48;
    std::atomic<uint32_t> at{0};
    uintptr_t addr[N] = {};
    uint64_t note[N] = {};
    bool on = false;
};
Crumbs g_crumbs;
void crumbs_dump(int) {
    Dl_info info;
    uintptr_t base = 0;
    if (dladdr((void*)&crumbs_dump, &info)) base = (uintptr_t)info.dli_fbase;
    const uint32_t end = g_crumbs.at.load();
    fprintf(stderr, "[h2agg breadcrumbs pid %d] last entries, oldest first (addresses relative to libh2agg.so):\n", (int)getpid());
    for (uint32_t k = end > Crumbs::N ? end - Crumbs::N : 0; k < end; ++k)
        fprintf(stderr, "  #%u  +0x%zx  note %llu\n", k, (size_t)(g_crumbs.addr[k % Crumbs::N] - base), (unsigned long long)g_crumbs.note[k % Crumbs::N]);
    fflush(stderr);
    signal(SIGABRT, SIG_DFL);
    abort();
}
inline void crumb(uintptr_t a, uint64_t note) {
    if (!g_crumbs.on) return;
    const uint32_t k = g_crumbs.at.fetch_add(1) % Crumbs::N;
    g_crumbs.addr[k] = a;
    g_crumbs.note[k] = note;
}
struct CrumbsInit {
    CrumbsInit() {
        if (knob("H2AGG_BREADCRUMBS")) {
            g_crumbs.on = true;
            signal(SIGABRT, crumbs_dump);
        }
    }
} g_crumbs_init;

// Debugging aid (H2AGG_CHAOS=<bits>, off by default): a one-lane kernel that just waits, put in front of work on a stream to
// shift the streams against one another — a missing event dependency then shows as a wrong result in the test suites instead of
// as a once-in-twenty-runs memory fault.  bit 0: in front of every tail; bit 1: in front of every accumulation; bit 2: in
// front of every sort; bit 3: in front of the auxiliary stream's transcript work (verifier.inc); bit 4: in front of every
// slice's copies of the host-buffer MSM.
__global__ void k_chaos_wait(uint32_t us) {
    const uint64_t t0 = wall_clock64();
    while (wall_clock64() - t0 < (uint64_t)us * 100u) __builtin_amdgcn_s_sleep(32);   // wall_clock64 ticks at 100 MHz
}
inline int chaos_bits() {
    static const int bits = knob("H2AGG_CHAOS") ? atoi(knob("H2AGG_CHAOS")) : 0;
    return bits;
}
inline void debug_sync(int bit) {   // H2AGG_SYNC_AT=<bits>: a device-wide wait at that point of msm_run (bisecting a race)
    static const int bits = knob("H2AGG_SYNC_AT") ? atoi(knob("H2AGG_SYNC_AT")) : 0;
    if (bits & bit) hipDeviceSynchronize();
}
inline void chaos_wait(int bit, hipStream_t s, uint32_t us = 300) {
    if (chaos_bits() & bit) hipLaunchKernelGGL(k_chaos_wait, dim3(1), dim3(1), 0, s, us);
}

// Which of the context's streams may run BESIDE the main stream?  HIP gives a stream its hardware queue when it is first used,
// round robin over GPU_MAX_HW_QUEUES (default 4) queues, so which streams share a queue depends on everything the process used
// before — and a tail stream on the main stream's queue puts its latency chains (0.5 ms kernels of one wave) IN FRONT of the next
// MSM's sort and accumulation: back-to-back 2^20-point MSMs then take 1.55-1.65 instead of 1.25 ms (profiles/r03_sweeps.txt
// section 18; a lazily made copy stream on that queue cost the host-buffer MSM 0.9 ms).  So the roles are handed out by
// measurement: every candidate is kept busy with a waiting kernel in turn while a tiny kernel goes to the main stream; the
// candidates that hold it up share its queue and get no role that matters.  ~4 ms per call; h2agg_create and h2agg_set_stream.
int place_streams(h2agg_ctx* c) {
    if (getenv("H2AGG_NO_PLACE")) return H2AGG_OK;
    constexpr int NP = h2agg_ctx::TAIL_SLOTS + 3 + 4;
    hipStream_t pool[NP];
    int np = 0;
    for (int k = 0; k < h2agg_ctx::TAIL_SLOTS; ++k) pool[np++] = c->tail_streams[k];
    pool[np++] = c->aux_stream;
    pool[np++] = c->copy_stream;
    for (int k = 0; k < 4; ++k) pool[np++] = c->spare_streams[k];
    pool[np++] = c->acc_stream;
    // first use (= queue assignment) in a fixed order: the main stream, then the candidates
    hipLaunchKernelGGL(k_chaos_wait, dim3(1), dim3(1), 0, c->stream, 1u);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < np; ++i) {
        hipLaunchKernelGGL(k_chaos_wait, dim3(1), dim3(1), 0, pool[i], 1u);
        HIP_TRY(c, hipStreamSynchronize(pool[i]));
    }
    bool blocks[NP];
    int nfree = 0;
    for (int i = 0; i < np; ++i) {
        int held = 0;   // (majority of three: one slow launch on a busy box must not cost a stream its role)
        for (int rep = 0; rep < 3; ++rep) {
            hipLaunchKernelGGL(k_chaos_wait, dim3(1), dim3(1), 0, pool[i], 250u);
            const auto t0 = std::chrono::steady_clock::now();
            hipLaunchKernelGGL(k_chaos_wait, dim3(1), dim3(1), 0, c->stream, 1u);
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            HIP_TRY(c, hipStreamSynchronize(pool[i]));
            held += us > 120.0;
            if (rep == 1 && (held == 0 || held == 2)) break;
        }
        blocks[i] = held >= 2;
        nfree += !blocks[i];
    }
    if (knob("H2AGG_TRACE_STREAMS")) {
        fprintf(stderr, "[h2agg] streams that hold the main stream up when busy:");
        for (int i = 0; i < np; ++i) fprintf(stderr, " %d%s", i, blocks[i] ? "*" : "");
        fprintf(stderr, "  (* = shares its queue)\n");
    }
    if (nfree < h2agg_ctx::TAIL_SLOTS + 2) return H2AGG_OK;   // (not enough to choose from: keep the creation order)
    hipStream_t ordered[NP];
    int no = 0;
    for (int i = 0; i < np; ++i)
        if (!blocks[i]) ordered[no++] = pool[i];
    for (int i = 0; i < np; ++i)
        if (blocks[i]) ordered[no++] = pool[i];
    int at = 0;
    for (int k = 0; k < h2agg_ctx::TAIL_SLOTS; ++k) c->tail_streams[k] = ordered[at++];
    c->aux_stream = ordered[at++];
    c->copy_stream = ordered[at++];
    c->acc_stream = ordered[at++];
    for (int k = 0; k < 4; ++k) c->spare_streams[k] = ordered[at++];
    return H2AGG_OK;
}

// harvest one ring slot (blocks until that call's events have completed)
void profile_harvest(h2agg_ctx* c, int slot) {
    h2agg_ctx::ProfSlot& ps = c->prof[slot];
    if (!ps.pending) return;
    for (int s = 0; s < ST_N; ++s) {
        if (!ps.used[s]) continue;
        float ms = 0.f;
        hipEventSynchronize(ps.ev[s][1]);
        if (hipEventElapsedTime(&ms, ps.ev[s][0], ps.ev[s][1]) == hipSuccess) {
            c->stage_ms[s] += ms;
            c->stage_launches[s] += 1;
        }
        ps.used[s] = false;
    }
    ps.pending = false;
}
void profile_begin_call(h2agg_ctx* c) {
    if (!c->profiling) return;
    profile_harvest(c, c->prof_cur);  // slot about to be reused
}
void profile_end_call(h2agg_ctx* c) {
    if (!c->profiling) return;
    c->prof[c->prof_cur].pending = true;
    c->prof_cur = (c->prof_cur + 1) % h2agg_ctx::PROF_RING;
}
void profile_harvest_all(h2agg_ctx* c) {
    for (int k = 0; k < h2agg_ctx::PROF_RING; ++k) profile_harvest(c, k);
}

#include "msm_run.inc"

int set_identity_jac(uint8_t out[96]) {
    memset(out, 0, 96);
    out[32] = 1;
    return 0;
}

int fetch_result_jac(h2agg_ctx* c, uint8_t out[96]) {
    TRY(join_tails(c));
    HIP_TRY(c, hipMemcpyAsync(c->h_pinned, c->d_res_jac, 96, hipMemcpyDeviceToHost, c->stream));
    TRY(finish(c));
    memcpy(out, c->h_pinned, 96);
    return H2AGG_OK;
}

int bind(h2agg_ctx* c) {
    crumb((uintptr_t)__builtin_return_address(0), 0);
    if (!c) return H2AGG_ERR_INVALID;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return fail(c, H2AGG_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    return H2AGG_OK;
}

}  // namespace

extern "C" {

int h2agg_create(int device_ordinal, h2agg_ctx** out) try {
    if (!out) return H2AGG_ERR_INVALID;
    *out = nullptr;
    int count = 0;
    if (device_ordinal < 0 || hipGetDeviceCount(&count) != hipSuccess || device_ordinal >= count)
        return H2AGG_ERR_HIP;  // no CPU mode: a HIP device is required
    if (hipSetDevice(device_ordinal) != hipSuccess) return H2AGG_ERR_HIP;
    h2agg_ctx* c = new h2agg_ctx();
    c->device = device_ordinal;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) != hipSuccess) {
        delete c;
        return H2AGG_ERR_HIP;
    }
    c->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    char buf[256];
    snprintf(buf, sizeof buf, "h2agg 0.1 %s cu=%d", prop.gcnArchName, c->cu_count);
    c->desc = buf;
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess ||
        hipHostMalloc((void**)&c->h_pinned, 4096) != hipSuccess || ensure(c, c->small, 4096) != H2AGG_OK) {
        h2agg_destroy(c);
        return H2AGG_ERR_HIP;
    }
    c->stream = c->own_stream;
    for (int k = 0; k < h2agg_ctx::TAIL_SLOTS; ++k) {
        // H2AGG_TAIL_PRIO (experiment): -1 = lowest, 1 = highest stream priority for the tail streams
        static const int tail_prio = knob("H2AGG_TAIL_PRIO") ? atoi(knob("H2AGG_TAIL_PRIO")) : 0;
        int pr_lo = 0, pr_hi = 0;
        hipDeviceGetStreamPriorityRange(&pr_lo, &pr_hi);   // lo = least (numerically greatest)
        if ((tail_prio ? hipStreamCreateWithPriority(&c->tail_streams[k], hipStreamNonBlocking, tail_prio < 0 ? pr_lo : pr_hi)
                       : hipStreamCreateWithFlags(&c->tail_streams[k], hipStreamNonBlocking)) != hipSuccess) {
            h2agg_destroy(c);
            return H2AGG_ERR_HIP;
        }
        hipEventCreateWithFlags(&c->ev_bulk[k], EV_SYNC_FLAGS);
        hipEventCreateWithFlags(&c->ev_tail[k], EV_SYNC_FLAGS);
    }
    int apr_lo = 0, apr_hi = 0;
    hipDeviceGetStreamPriorityRange(&apr_lo, &apr_hi);
    static const int acc_prio = knob("H2AGG_ACC_PRIO") ? atoi(knob("H2AGG_ACC_PRIO")) : 0;   // experiment: -1 lowest
    if ((acc_prio ? hipStreamCreateWithPriority(&c->acc_stream, hipStreamNonBlocking, acc_prio < 0 ? apr_lo : apr_hi)
                  : hipStreamCreateWithFlags(&c->acc_stream, hipStreamNonBlocking)) != hipSuccess) {
        h2agg_destroy(c);
        return H2AGG_ERR_HIP;
    }
    // The auxiliary and the copy stream are made HERE, in a fixed order behind the others, not at their first use: where the
    // runtime places a stream depends on how many streams the process has made before it (profiles/r03_sweeps.txt section 18:
    // back-to-back MSMs run at 1.25 or at 1.55 ms per step depending on the number of streams made between the main stream and
    // the tail streams), and a placement that changes with what else the process did first is not reproducible.
    if (hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess) {
        h2agg_destroy(c);
        return H2AGG_ERR_HIP;
    }
    for (int k = 0; k < 4; ++k)
        if (hipStreamCreateWithFlags(&c->spare_streams[k], hipStreamNonBlocking) != hipSuccess) {
            h2agg_destroy(c);
            return H2AGG_ERR_HIP;
        }
    hipEventCreateWithFlags(&c->ev_aux, hipEventDisableTiming);
    hipEventCreateWithFlags(&c->ev_aux_go, hipEventDisableTiming);
    for (int k = 0; k < MSM_MAX_SLICES; ++k) {
        hipEventCreateWithFlags(&c->ev_copy[k], hipEventDisableTiming);
        hipEventCreateWithFlags(&c->ev_copy_s[k], hipEventDisableTiming);
    }
    hipEventCreateWithFlags(&c->ev_ready, hipEventDisableTiming);
    hipEventCreateWithFlags(&c->ev_sortdone, EV_SYNC_FLAGS);
    for (int q = 0; q < 2; ++q) {
        hipEventCreateWithFlags(&c->ev_sorted[q], EV_SYNC_FLAGS);
        hipEventCreateWithFlags(&c->ev_accdone[q], EV_SYNC_FLAGS);
    }
    c->d_flags = (uint32_t*)c->small.p;
    c->d_res_xyzz = (uint8_t*)c->small.p + 1024;   // 144 B
    c->d_res_jac = (uint8_t*)c->small.p + 256;   // 96 B
    hipMemset(c->small.p, 0, 4096);
    if (place_streams(c) != H2AGG_OK) {
        h2agg_destroy(c);
        return H2AGG_ERR_HIP;
    }
    *out = c;
    return H2AGG_OK;
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

}  // extern "C"
namespace {
void comm_release(h2agg_ctx* c);   // csrc/comm.inc
void agg_plans_release(h2agg_ctx* c);   // csrc/verifier.inc
}
extern "C" {
void h2agg_destroy(h2agg_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    comm_release(c);
    agg_plans_release(c);
    flush_deferred_tail(c, false);
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->acc_stream) hipStreamSynchronize(c->acc_stream);
    for (int k = 0; k < h2agg_ctx::TAIL_SLOTS; ++k)
        if (c->tail_streams[k]) hipStreamSynchronize(c->tail_streams[k]);
    static_assert(h2agg_ctx::TAIL_SLOTS == 3, "the list below names every tail slot's buffers");
    DevBuf* bufs[] = {&c->in_a,  &c->in_b,     &c->in_c,     &c->out,   &c->tmp_bases, &c->comb, &c->psd_spec, &c->tr_in, &c->tr_points, &c->tr_elems, &c->tr_chal, &c->inst_vals, &c->inst_jac, &c->inst_aff, &c->agg_elems, &c->hist[0], &c->hist[1],
                      &c->offs[0], &c->offs[1], &c->pmeta[0], &c->pmeta[1], &c->item_idx, &c->item_sub, &c->order[0], &c->order[1], &c->entries[0], &c->entries[1],
                      &c->r2d_ticket[0], &c->r2d_ticket[1], &c->r2d_ticket[2], &c->buckets[0], &c->buckets[1], &c->buckets[2], &c->segsum[0], &c->segsum[1], &c->segsum[2],
                      &c->wsum[0], &c->wsum[1], &c->wsum[2], &c->big_list[0], &c->big_list[1], &c->big_keys[0], &c->big_keys[1], &c->big_part[0], &c->big_part[1], &c->fix_list[0], &c->fix_list[1], &c->glv_buf, &c->parts, &c->small, &c->endo_buf, &c->tile_counts, &c->fb_long,
                      &c->sch_regs, &c->sch_in, &c->sch_scalars[0], &c->sch_scalars[1], &c->sch_bases[0], &c->sch_bases[1], &c->sch_endo,
                      &c->seg_wsum, &c->seg_dev, &c->seg_out, &c->fft_tw[0], &c->fft_tw[1], &c->fft_scale,
                      &c->frfft_tw[0], &c->frfft_tw[1], &c->frfft_shift, &c->frfft_work,
                      &c->poly_work, &c->poly_desc, &c->poly_slab, &c->poly_jac,
                      &c->prod_num, &c->prod_den, &c->prod_lvl, &c->prod_tab, &c->lk_work, &c->lk_desc,
                      &c->qt_work, &c->qt_prog, &c->qt_tab, &c->kg_bitmap, &c->kg_delta, &c->kg_jac};
    for (DevBuf* b : bufs)
        if (b->p) hipFree(b->p);
    for (auto& kv : c->tables) {
        if (kv.second.d) hipFree(kv.second.d);
        if (kv.second.endo_x) hipFree(kv.second.endo_x);
        kv.second.free_combs();
        if (kv.second.pre) hipFree(kv.second.pre);
    }
    if (c->h_pinned) hipHostFree(c->h_pinned);
    if (c->h_stage) hipHostFree(c->h_stage);
    if (c->h_down) hipHostFree(c->h_down);
    if (c->copy_stream) {
        hipStreamSynchronize(c->copy_stream);
        for (int k = 0; k < MSM_MAX_SLICES; ++k) {
            if (c->ev_copy[k]) hipEventDestroy(c->ev_copy[k]);
            if (c->ev_copy_s[k]) hipEventDestroy(c->ev_copy_s[k]);
        }
        if (c->ev_ready) hipEventDestroy(c->ev_ready);
        hipStreamDestroy(c->copy_stream);
    }
    if (c->aux_stream) {
        hipStreamSynchronize(c->aux_stream);
        if (c->ev_aux) hipEventDestroy(c->ev_aux);
        if (c->ev_aux_go) hipEventDestroy(c->ev_aux_go);
        hipStreamDestroy(c->aux_stream);
    }
    for (int r = 0; r < h2agg_ctx::PROF_RING; ++r)
        for (int s = 0; s < ST_N; ++s)
            for (int k = 0; k < 2; ++k)
                if (c->prof[r].ev[s][k]) hipEventDestroy(c->prof[r].ev[s][k]);
    for (int k = 0; k < h2agg_ctx::TAIL_SLOTS; ++k) {
        if (c->ev_bulk[k]) hipEventDestroy(c->ev_bulk[k]);
        if (c->ev_tail[k]) hipEventDestroy(c->ev_tail[k]);
        if (c->tail_streams[k]) hipStreamDestroy(c->tail_streams[k]);
    }
    if (c->ev_sortdone) hipEventDestroy(c->ev_sortdone);
    for (int q = 0; q < 2; ++q) {
        if (c->ev_sorted[q]) hipEventDestroy(c->ev_sorted[q]);
        if (c->ev_accdone[q]) hipEventDestroy(c->ev_accdone[q]);
    }
    if (c->acc_stream) hipStreamDestroy(c->acc_stream);
    for (int k = 0; k < 4; ++k)
        if (c->spare_streams[k]) hipStreamDestroy(c->spare_streams[k]);
    if (c->own_stream) hipStreamDestroy(c->own_stream);
    delete c;
}

const char* h2agg_last_error(const h2agg_ctx* c) { return c ? c->err.c_str() : "null context"; }
const char* h2agg_describe(h2agg_ctx* c) { return c ? c->desc.c_str() : ""; }

int h2agg_set_stream(h2agg_ctx* c, void* hip_stream) try {
    TRY(bind(c));
    TRY(join_tails(c));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const hipStream_t was = c->stream;
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    if (c->stream != was) {   // another main stream, another queue: hand the roles out again
        // The probe launches kernels on the caller's stream and waits for them: not possible while that stream is being
        // captured into a graph — the roles then stay as they are (H2AGG_NO_PLACE skips the probe altogether).
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hip_stream && hipStreamIsCapturing(c->stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) return H2AGG_OK;
        (void)hipGetLastError();
        HIP_TRY(c, hipDeviceSynchronize());
        TRY(place_streams(c));
    }
    return H2AGG_OK;
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_synchronize(h2agg_ctx* c) try {
    TRY(bind(c));
    TRY(join_tails(c));
    // also the place where status flags raised by asynchronous calls surface (e.g. a scalar >= r handed to
    // h2agg_g1_msm_device_async -> H2AGG_ERR_NONCANONICAL here)
    TRY(clear_flags(c));
    return finish(c);
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

// ---------------------------------------------------------------- Fr
int h2agg_fr_batch_op(h2agg_ctx* c, int op, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out) try {
    TRY(bind(c));
    if (op < H2AGG_OP_ADD || op > H2AGG_OP_DIV) return fail(c, H2AGG_ERR_INVALID, "unknown field op");
    if (n == 0) return H2AGG_OK;
    const bool binary = op <= H2AGG_OP_MUL || op == H2AGG_OP_DIV;
    if (!a || !out || (binary && !b)) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_a, 32 * n));
    TRY(ensure(c, c->out, 32 * n));
    HIP_TRY(c, hipMemcpyAsync(c->in_a.p, a, 32 * n, hipMemcpyHostToDevice, c->stream));
    if (binary) {
        TRY(ensure(c, c->in_b, 32 * n));
        HIP_TRY(c, hipMemcpyAsync(c->in_b.p, b, 32 * n, hipMemcpyHostToDevice, c->stream));
    }
    TRY(clear_flags(c));
    hipLaunchKernelGGL(k_fr_batch_op, dim3(grid_for(c, n)), dim3(BLOCK), 0, c->stream, op, (const uint8_t*)c->in_a.p,
                       (const uint8_t*)c->in_b.p, n, (uint8_t*)c->out.p, c->d_flags);
    HIP_TRY(c, hipMemcpyAsync(out, c->out.p, 32 * n, hipMemcpyDeviceToHost, c->stream));
    return finish(c);
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_fr_batch_pow_constant(h2agg_ctx* c, const uint8_t* a, size_t n, uint64_t exponent, uint8_t* out) try {
    TRY(bind(c));
    if (exponent < 1) return fail(c, H2AGG_ERR_INVALID, "assert!(exponent >= 1) failed (arith/field.rs:89)");
    if (n == 0) return H2AGG_OK;
    if (!a || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_a, 32 * n));
    TRY(ensure(c, c->out, 32 * n));
    HIP_TRY(c, hipMemcpyAsync(c->in_a.p, a, 32 * n, hipMemcpyHostToDevice, c->stream));
    TRY(clear_flags(c));
    hipLaunchKernelGGL(k_fr_batch_pow, dim3(grid_for(c, n)), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->in_a.p, n,
                       exponent, (uint8_t*)c->out.p, c->d_flags);
    HIP_TRY(c, hipMemcpyAsync(out, c->out.p, 32 * n, hipMemcpyDeviceToHost, c->stream));
    return finish(c);
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_fr_mul_add_accumulate(h2agg_ctx* c, const uint8_t* v, size_t n, const uint8_t b[32], uint8_t out[32]) try {
    TRY(bind(c));
    if ((n && !v) || !b || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_a, 32 * n + 32));
    TRY(ensure(c, c->in_b, 32));
    TRY(ensure(c, c->out, 32));
    if (n) HIP_TRY(c, hipMemcpyAsync(c->in_a.p, v, 32 * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->in_b.p, b, 32, hipMemcpyHostToDevice, c->stream));
    TRY(clear_flags(c));
    hipLaunchKernelGGL(k_fr_horner, dim3(1), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->in_a.p, n,
                       (const uint8_t*)c->in_b.p, (uint8_t*)c->out.p, c->d_flags);
    HIP_TRY(c, hipMemcpyAsync(out, c->out.p, 32, hipMemcpyDeviceToHost, c->stream));
    return finish(c);
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_fr_sum_with_coeff_and_constant(h2agg_ctx* c, const uint8_t* x, const uint8_t* coeff, size_t n,
                                         const uint8_t b[32], uint8_t out[32]) try {
    TRY(bind(c));
    if ((n && (!x || !coeff)) || !b || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_a, 32 * n + 32));
    TRY(ensure(c, c->in_b, 32 * n + 32));
    TRY(ensure(c, c->in_c, 32));
    TRY(ensure(c, c->out, 32));
    if (n) {
        HIP_TRY(c, hipMemcpyAsync(c->in_a.p, x, 32 * n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->in_b.p, coeff, 32 * n, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(c->in_c.p, b, 32, hipMemcpyHostToDevice, c->stream));
    TRY(clear_flags(c));
    hipLaunchKernelGGL(k_fr_sum_coeff, dim3(1), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->in_a.p,
                       (const uint8_t*)c->in_b.p, n, (const uint8_t*)c->in_c.p, (uint8_t*)c->out.p, c->d_flags);
    HIP_TRY(c, hipMemcpyAsync(out, c->out.p, 32, hipMemcpyDeviceToHost, c->stream));
    return finish(c);
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

// ---------------------------------------------------------------- G1 batch
int h2agg_g1_batch_add(h2agg_ctx* c, const uint8_t* a, const uint8_t* b, size_t n, int subtract, uint8_t* out) try {
    TRY(bind(c));
    if (n == 0) return H2AGG_OK;
    if (!a || !b || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_a, 96 * n));
    TRY(ensure(c, c->in_b, 96 * n));
    TRY(ensure(c, c->out, 96 * n));
    HIP_TRY(c, hipMemcpyAsync(c->in_a.p, a, 96 * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->in_b.p, b, 96 * n, hipMemcpyHostToDevice, c->stream));
    TRY(clear_flags(c));
    hipLaunchKernelGGL(k_g1_batch_add, dim3(grid_for(c, n)), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->in_a.p,
                       (const uint8_t*)c->in_b.p, n, subtract, (uint8_t*)c->out.p, c->d_flags);
    HIP_TRY(c, hipMemcpyAsync(out, c->out.p, 96 * n, hipMemcpyDeviceToHost, c->stream));
    return finish(c);
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_g1_batch_scalar_mul(h2agg_ctx* c, const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t* out) try {
    TRY(bind(c));
    if (n == 0) return H2AGG_OK;
    if (!bases || !scalars || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_a, 64 * n));
    TRY(ensure(c, c->in_b, 32 * n));
    TRY(ensure(c, c->out, 96 * n));
    HIP_TRY(c, hipMemcpyAsync(c->in_a.p, bases, 64 * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->in_b.p, scalars, 32 * n, hipMemcpyHostToDevice, c->stream));
    TRY(clear_flags(c));
    // GLV + signed window-4 ladder, four lanes per point (csrc/scalar_mul_kernels.hpp); H2AGG_SCALAR_MUL=ladder selects the
    // round-1 bit-serial kernel for A/B measurements
    static const bool ladder = knob("H2AGG_SCALAR_MUL") && !strcmp(knob("H2AGG_SCALAR_MUL"), "ladder");
    if (ladder) {
        hipLaunchKernelGGL(k_g1_batch_scalar_mul, dim3(grid_for(c, n)), dim3(BLOCK), 0, c->stream,
                           (const uint8_t*)c->in_a.p, (const uint8_t*)c->in_b.p, n, (uint8_t*)c->out.p, c->d_flags);
    } else {
        size_t groups = (n + SM_GROUPS - 1) / SM_GROUPS;
        const size_t cap = (size_t)c->cu_count * 16;
        if (groups > cap) groups = cap;
        hipLaunchKernelGGL(k_g1_batch_scalar_mul_w4, dim3((unsigned)groups), dim3(SM_THREADS), 0, c->stream,
                           (const uint8_t*)c->in_a.p, (const uint8_t*)c->in_b.p, n, (uint8_t*)c->out.p, c->d_flags);
    }
    HIP_TRY(c, hipMemcpyAsync(out, c->out.p, 96 * n, hipMemcpyDeviceToHost, c->stream));
    return finish(c);
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_g1_batch_to_affine(h2agg_ctx* c, const uint8_t* in, size_t n, uint8_t* out) try {
    TRY(bind(c));
    if (n == 0) return H2AGG_OK;
    if (!in || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_a, 96 * n));
    TRY(ensure(c, c->out, 64 * n));
    HIP_TRY(c, hipMemcpyAsync(c->in_a.p, in, 96 * n, hipMemcpyHostToDevice, c->stream));
    TRY(clear_flags(c));
    hipLaunchKernelGGL(k_g1_batch_to_affine, dim3(grid_for(c, n)), dim3(BLOCK), 0, c->stream,
                       (const uint8_t*)c->in_a.p, n, (uint8_t*)c->out.p, c->d_flags);
    HIP_TRY(c, hipMemcpyAsync(out, c->out.p, 64 * n, hipMemcpyDeviceToHost, c->stream));
    return finish(c);
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_g1_batch_to_affine_device(h2agg_ctx* c, const uint8_t* d_in_jac, size_t n, uint8_t* out) try {
    TRY(bind(c));
    if (n == 0) return H2AGG_OK;
    if (!d_in_jac || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(join_tails(c));   // the inputs are typically results of h2agg_g1_msm_device_async
    TRY(ensure(c, c->out, 64 * n));
    TRY(clear_flags(c));
    hipLaunchKernelGGL(k_g1_batch_to_affine, dim3(grid_for(c, n)), dim3(BLOCK), 0, c->stream, d_in_jac, n,
                       (uint8_t*)c->out.p, c->d_flags);
    HIP_TRY(c, hipMemcpyAsync(out, c->out.p, 64 * n, hipMemcpyDeviceToHost, c->stream));
    return finish(c);
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_g1_batch_decompress(h2agg_ctx* c, const uint8_t* in, size_t n, uint8_t* out_aff, uint8_t* ok) try {
    TRY(bind(c));
    if (n == 0) return H2AGG_OK;
    if (!in || !out_aff) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_a, 32 * n));
    TRY(ensure(c, c->out, 64 * n));
    TRY(ensure(c, c->in_b, n + 16));
    HIP_TRY(c, hipMemcpyAsync(c->in_a.p, in, 32 * n, hipMemcpyHostToDevice, c->stream));
    TRY(clear_flags(c));
    hipLaunchKernelGGL(k_g1_batch_decompress, dim3(grid_for(c, n)), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->in_a.p, n,
                       (uint8_t*)c->out.p, (uint8_t*)c->in_b.p, c->d_flags);
    HIP_TRY(c, hipMemcpyAsync(out_aff, c->out.p, 64 * n, hipMemcpyDeviceToHost, c->stream));
    if (ok) HIP_TRY(c, hipMemcpyAsync(ok, c->in_b.p, n, hipMemcpyDeviceToHost, c->stream));
    return finish(c);
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}
int h2agg_g1_batch_compress(h2agg_ctx* c, const uint8_t* aff, size_t n, uint8_t* out) try {
    TRY(bind(c));
    if (n == 0) return H2AGG_OK;
    if (!aff || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_a, 64 * n));
    TRY(ensure(c, c->out, 32 * n));
    HIP_TRY(c, hipMemcpyAsync(c->in_a.p, aff, 64 * n, hipMemcpyHostToDevice, c->stream));
    TRY(clear_flags(c));
    hipLaunchKernelGGL(k_g1_batch_compress, dim3(grid_for(c, n)), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->in_a.p, n,
                       (uint8_t*)c->out.p, c->d_flags);
    HIP_TRY(c, hipMemcpyAsync(out, c->out.p, 32 * n, hipMemcpyDeviceToHost, c->stream));
    return finish(c);
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_g1_sum(h2agg_ctx* c, const uint8_t* in, size_t n, uint8_t out[96]) try {
    TRY(bind(c));
    if (!out || (n && !in)) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_a, 96 * n + 96));
    if (n) HIP_TRY(c, hipMemcpyAsync(c->in_a.p, in, 96 * n, hipMemcpyHostToDevice, c->stream));
    TRY(clear_flags(c));
    hipLaunchKernelGGL(k_g1_sum, dim3(1), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->in_a.p, n, c->d_res_jac,
                       c->d_flags);
    return fetch_result_jac(c, out);
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

// ---------------------------------------------------------------- base tables
int h2agg_bases_upload(h2agg_ctx* c, const uint8_t* bases, size_t n, uint64_t* handle_out) try {
    TRY(bind(c));
    if (!bases || !handle_out || n == 0) return fail(c, H2AGG_ERR_INVALID, "null buffer or n == 0");
    Table t;
    t.n = n;
    if (hipMalloc((void**)&t.d, 64 * n) != hipSuccess) return fail(c, H2AGG_ERR_NOMEM, "hipMalloc(base table)");
    int rc = ensure(c, c->tmp_bases, 64 * n);
    if (rc == H2AGG_OK) {
        hipError_t e = hipMemcpyAsync(c->tmp_bases.p, bases, 64 * n, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) rc = fail(c, H2AGG_ERR_HIP, hipGetErrorString(e));
    }
    if (rc == H2AGG_OK) rc = clear_flags(c);
    if (rc == H2AGG_OK) {
        hipLaunchKernelGGL(k_bases_to_mont, dim3(grid_for(c, n)), dim3(BLOCK), 0, c->stream,
                           (const uint8_t*)c->tmp_bases.p, n, t.d, c->d_flags);
        rc = finish(c);
    }
    if (rc != H2AGG_OK) {
        hipFree(t.d);
        return rc;
    }
    t.no_identity = table_word_clear(c->table_word);
    uint64_t h = c->next_handle++;
    c->tables[h] = t;
    *handle_out = h;
    return H2AGG_OK;
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

}  // extern "C"
namespace {
// out[i] = k_i * G (Montgomery affine) through the fixed-base comb: d * 2^(8w) * G for every byte position, built once per
// context (32 x 255 points, 510 KiB).  Queued on the context's stream.
int comb_generate_launch(h2agg_ctx* c, const uint8_t* d_k, size_t n, uint8_t* out) {
    if (!c->comb_ready) {
        TRY(ensure(c, c->comb, (size_t)COMB_WINDOWS * COMB_ROW * 64));
        hipLaunchKernelGGL(k_comb_table_build, dim3((COMB_WINDOWS * COMB_ROW + SM_GROUPS - 1) / SM_GROUPS), dim3(SM_THREADS), 0,
                           c->stream, (uint8_t*)c->comb.p, c->d_flags);
        c->comb_ready = true;
    }
    size_t blocks = (n + BLOCK - 1) / BLOCK;
    if (blocks > 65535 * 16) blocks = 65535 * 16;
    hipLaunchKernelGGL(k_bases_generate_comb, dim3((unsigned)blocks), dim3(BLOCK), 0, c->stream, d_k, n, (const uint8_t*)c->comb.p,
                       out, c->d_flags);
    return H2AGG_OK;
}
}  // namespace
extern "C" {
int h2agg_bases_generate(h2agg_ctx* c, const void* d_k, size_t n, uint64_t* handle_out) try {
    TRY(bind(c));
    if (!d_k || !handle_out || n == 0) return fail(c, H2AGG_ERR_INVALID, "null buffer or n == 0");
    Table t;
    t.n = n;
    if (hipMalloc((void**)&t.d, 64 * n) != hipSuccess) return fail(c, H2AGG_ERR_NOMEM, "hipMalloc(base table)");
    int rc = clear_flags(c);
    if (rc == H2AGG_OK) {
        static const bool ladder = knob("H2AGG_SCALAR_MUL") && !strcmp(knob("H2AGG_SCALAR_MUL"), "ladder");
        if (ladder) {
            size_t blocks = (n + BLOCK - 1) / BLOCK;
            if (blocks > 65535 * 16) blocks = 65535 * 16;
            hipLaunchKernelGGL(k_bases_generate, dim3((unsigned)blocks), dim3(BLOCK), 0, c->stream, (const uint8_t*)d_k, n, t.d,
                               c->d_flags);
        } else {
            rc = comb_generate_launch(c, (const uint8_t*)d_k, n, t.d);
        }
        if (rc == H2AGG_OK) rc = finish(c);
    }
    if (rc != H2AGG_OK) {
        hipFree(t.d);
        return rc;
    }
    t.no_identity = table_word_clear(c->table_word);
    uint64_t h = c->next_handle++;
    c->tables[h] = t;
    *handle_out = h;
    return H2AGG_OK;
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_bases_download(h2agg_ctx* c, uint64_t handle, size_t first, size_t n, uint8_t* out) try {
    TRY(bind(c));
    auto it = c->tables.find(handle);
    if (it == c->tables.end()) return fail(c, H2AGG_ERR_INVALID, "unknown base-table handle");
    if (!out || first + n > it->second.n) return fail(c, H2AGG_ERR_INVALID, "range outside the table");
    if (n == 0) return H2AGG_OK;
    TRY(ensure(c, c->out, 64 * n));
    hipLaunchKernelGGL(k_bases_from_mont, dim3(grid_for(c, n)), dim3(BLOCK), 0, c->stream, it->second.d + 64 * first,
                       n, (uint8_t*)c->out.p);
    HIP_TRY(c, hipMemcpyAsync(out, c->out.p, 64 * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return H2AGG_OK;
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_bases_free(h2agg_ctx* c, uint64_t handle) try {
    TRY(bind(c));
    auto it = c->tables.find(handle);
    if (it == c->tables.end()) return fail(c, H2AGG_ERR_INVALID, "unknown base-table handle");
    TRY(join_tails(c));   // tails and accumulations on the context's other streams (and a deferred tail) may still read the table
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    hipFree(it->second.d);
    if (it->second.endo_x) hipFree(it->second.endo_x);
    if (it->second.pre) hipFree(it->second.pre);
    it->second.free_combs();
    c->tables.erase(it);
    return H2AGG_OK;
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

// ---------------------------------------------------------------- MSM
}  // extern "C"
namespace {
// beta * x column of a resident table, made once
int table_endo(h2agg_ctx* c, Table& t, const uint8_t** out) {
    if (!t.endo_x) {
        if (hipMalloc((void**)&t.endo_x, 32 * t.n) != hipSuccess) return fail(c, H2AGG_ERR_NOMEM, "hipMalloc(endo table)");
        hipLaunchKernelGGL(k_bases_endo_x, dim3(grid_for(c, t.n)), dim3(BLOCK), 0, c->stream, (const uint8_t*)t.d, t.n,
                           t.endo_x);
    }
    *out = t.endo_x;
    return H2AGG_OK;
}
}  // namespace
extern "C" {
// width of the fixed-base levels: n * ceil(255 / c) bucket insertions + one reduction of 2^(c-1) buckets (~4 mixed-add
// equivalents per bucket), minimised over c; capped so the sort's packed items and partitions stay in range
int choose_pre_window(size_t n) {
    int best = 16;
    double best_cost = 1e300;
    for (int cc = 8; cc <= 20; ++cc) {
        const double cost = (double)n * ((255 + cc - 1) / cc) + 4.0 * (double)((size_t)1 << (cc - 1));
        if (cost < best_cost) {
            best_cost = cost;
            best = cc;
        }
    }
    return best;
}

int h2agg_bases_precompute(h2agg_ctx* c, uint64_t handle, int window_bits) try {
    TRY(bind(c));
    auto it = c->tables.find(handle);
    if (it == c->tables.end()) return fail(c, H2AGG_ERR_INVALID, "unknown base-table handle");
    Table& t = it->second;
    if (window_bits != 0 && (window_bits < 4 || window_bits > 20))
        return fail(c, H2AGG_ERR_INVALID, "fixed-base window must be 0 (auto) or in [4, 20]");
    int cc = window_bits ? window_bits : choose_pre_window(t.n);
    // tables whose levels outgrow the packed sort item take c = 20 and the (level, point) sort of fb_sort_kernels.hpp
    if (!window_bits && (size_t)((255 + cc - 1) / cc) * t.n > ((size_t)1 << 22)) cc = FB_C;
    const int W = (255 + cc - 1) / cc;
    if (cc == FB_C && t.n > (size_t)FB_MAX_TILES * FB_T)
        return fail(c, H2AGG_ERR_INVALID, "table too large for fixed-base levels (at most 2^22 points)");
    // other widths are addressed through the sort's packed 32-bit item (22 index bits next to 9 sub-bucket bits + sign):
    // beyond that the sort falls back to its two-array kernels and the levels stop paying for themselves (round 4, with the
    // limit lifted: 16 MSMs over a 2^22-point table 74 ms on the ordinary path, 113 ms through levels at c = 20 + the two-array
    // sort).  debug key "pre_big" lifts the limit for A/B runs of exactly that.
    if (cc != FB_C && (size_t)W * t.n > ((size_t)1 << 22) && !c->dbg_pre_big)
        return fail(c, H2AGG_ERR_INVALID, "table too large for fixed-base levels (ceil(255 / c) * n must be <= 2^22)");
    if (!window_bits) {
        // auto mode is the opportunistic call: it does not take a large share of what is left of the device for levels
        // (832 B per point at c = 20: 3.25 GiB for a 2^22-point table) — the caller who wants them regardless names the width
        size_t free_b = 0, total_b = 0;
        HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
        if ((size_t)W * t.n * 64 > free_b / 4)
            return fail(c, H2AGG_ERR_NOMEM, "fixed-base levels (auto) would take more than a quarter of the free device memory; pass window_bits to insist");
    }
    TRY(join_tails(c));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (t.pre) {
        hipFree(t.pre);
        t.pre = nullptr;
    }
    t.free_combs();
    if (hipMalloc((void**)&t.pre, (size_t)W * t.n * 64) != hipSuccess)
        return fail(c, H2AGG_ERR_NOMEM, "hipMalloc(fixed-base levels)");
    HIP_TRY(c, hipMemcpyAsync(t.pre, t.d, t.n * 64, hipMemcpyDeviceToDevice, c->stream));
    for (int w = 1; w < W; ++w)
        hipLaunchKernelGGL(k_bases_shift, dim3(grid_for(c, t.n)), dim3(BLOCK), 0, c->stream,
                           (const uint8_t*)t.pre + (size_t)(w - 1) * t.n * 64, t.n, cc, t.pre + (size_t)w * t.n * 64);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    t.pre_c = cc;
    t.pre_W = W;
    return H2AGG_OK;
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

}   // extern "C"
namespace {
// `batch` MSMs of n <= COMB_MSM_MAX scalars each over the leading bases of a table with fixed-base levels: through the table's
// comb (made here on first use).  Returns false when the comb route does not apply.
bool comb_msm_applies(const h2agg_ctx* c, const Table& t, size_t n) {
    const bool off = !c->dbg_comb_msm;
    return !off && t.pre && !c->cfg_c && n >= 1 && n <= (size_t)COMB_MSM_MAX;
}
// *done = false: the comb could not be made (no memory for it): the caller takes the bucket path, which needs none.
int comb_msm_run(h2agg_ctx* c, Table& t, const uint8_t* d_scalars, size_t n, size_t batch, uint8_t* d_out_jac, bool* done) {
    *done = true;
    if (!t.comb || t.comb_n < n) {
        // sized for what is asked (a one-point multi_exp does not pay for 256 bases' rows: 520 KiB per base), doubling so that
        // a caller whose sizes creep up rebuilds O(log) times; everything is ordered by the context's stream, no host wait:
        // the comb it replaces may still be read by kernels in flight and is only retired (Table::free_combs)
        const size_t cap_n = t.n < (size_t)COMB_MSM_MAX ? t.n : (size_t)COMB_MSM_MAX;
        size_t nb = 16;
        while (nb < n) nb *= 2;
        if (nb > cap_n) nb = cap_n;
        const size_t entries = nb * (size_t)COMB_WINDOWS * COMB_ROW;
        uint8_t* fresh = nullptr;
        if (hipMalloc((void**)&fresh, entries * 64) != hipSuccess) {
            (void)hipGetLastError();
            *done = false;
            return H2AGG_OK;
        }
        if (t.comb) t.comb_retired.push_back(t.comb);
        t.comb = fresh;
        size_t grid = (entries + SM_GROUPS - 1) / SM_GROUPS;
        const size_t cap = (size_t)c->cu_count * 16;
        if (grid > cap) grid = cap;
        hipLaunchKernelGGL(k_comb_table_build, dim3((unsigned)grid), dim3(SM_THREADS), 0, c->stream, t.comb, c->d_flags,
                           (const uint8_t*)t.d, (uint32_t)nb);
        t.comb_n = nb;
    }
    hipLaunchKernelGGL(k_comb_msm, dim3((unsigned)batch), dim3(BLOCK), 0, c->stream, (const uint8_t*)t.comb, d_scalars, (uint32_t)n,
                       d_out_jac, c->d_flags);
    HIP_TRY(c, hipGetLastError());
    return H2AGG_OK;
}
}   // namespace
extern "C" {

int h2agg_g1_msm_device_async(h2agg_ctx* c, uint64_t handle, const void* d_scalars, size_t n, void* d_out_jac) try {
    TRY(bind(c));
    auto it = c->tables.find(handle);
    if (it == c->tables.end()) return fail(c, H2AGG_ERR_INVALID, "unknown base-table handle");
    if (!d_scalars || !d_out_jac) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    if (n == 0) return fail(c, H2AGG_ERR_EMPTY, "multi_exp of zero pairs (reference panics: mock/arith/ecc.rs:128)");
    if (n > it->second.n) return fail(c, H2AGG_ERR_INVALID, "more scalars than bases in the table");
    if (comb_msm_applies(c, it->second, n)) {
        bool done = false;
        TRY(comb_msm_run(c, it->second, (const uint8_t*)d_scalars, n, 1, (uint8_t*)d_out_jac, &done));
        if (done) return H2AGG_OK;
    }
    const uint8_t* endo = nullptr;
    TRY(table_endo(c, it->second, &endo));
    // Beyond 2^22 points the packed (index | sub-bucket) sort item no longer fits 32 bits and the sort would fall back to
    // its slower two-array kernels: cut the MSM into slices of <= 2^22 points instead (their tails overlap the next
    // slice's bulk) and add the slices' results.
    if (it->second.pre && !c->cfg_c) {   // fixed-base levels (h2agg_bases_precompute); an explicit window_bits overrides
        const PreTable pt{it->second.pre, it->second.n, it->second.pre_c, it->second.pre_W};
        if ((size_t)pt.W * n < ((size_t)1 << 32)) {
            MsmCall call{it->second.d, (const uint8_t*)d_scalars, n, (uint8_t*)d_out_jac};
            call.pre = &pt;
            return msm_run(c, call);
        }
    }
    const size_t SLICE = (size_t)1 << 22;
    MsmCall call{it->second.d, (const uint8_t*)d_scalars, n, (uint8_t*)d_out_jac};
    call.d_endo_x = endo;
    call.no_identity = it->second.no_identity;
    if (n <= SLICE) return msm_run(c, call);
    // The slices share ONE bucket set (chain modes of msm_run): every slice adds its points to the sums the buckets already
    // hold, and only the last one is followed by the bucket reduction / window sums / Horner tail.
    const size_t nsl = (n + SLICE - 1) / SLICE;
    const bool was_overlap = c->tail_overlap;
    {
        OverlapScope overlap(c);
        call.chain_n = n;
        call.chain_glv = false;
        for (size_t k = 0; k < nsl; ++k) {
            const size_t off = k * SLICE;
            call.d_bases = it->second.d + 64 * off;
            call.d_scalars = (const uint8_t*)d_scalars + 32 * off;
            call.d_endo_x = endo + 32 * off;
            call.n_base = n - off < SLICE ? n - off : SLICE;
            call.chain = k == 0 ? CHAIN_FIRST : (k + 1 == nsl ? CHAIN_LAST : CHAIN_MID);
            TRY(msm_run(c, call));
        }
    }
    if (!was_overlap) TRY(join_tails(c));   // without overlap mode the caller's stream orders the result
    return H2AGG_OK;
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_g1_msm_device_batch_async(h2agg_ctx* c, uint64_t handle, const void* d_scalars, size_t n, size_t batch,
                                    void* d_out_jac) try {
    TRY(bind(c));
    auto it = c->tables.find(handle);
    if (it == c->tables.end()) return fail(c, H2AGG_ERR_INVALID, "unknown base-table handle");
    if (!d_scalars || !d_out_jac) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    if (n == 0 || batch == 0)
        return fail(c, H2AGG_ERR_EMPTY, "multi_exp of zero pairs (reference panics: mock/arith/ecc.rs:128)");
    if (n > it->second.n) return fail(c, H2AGG_ERR_INVALID, "more scalars than bases in the table");
    if (comb_msm_applies(c, it->second, n)) {
        bool done = false;
        TRY(comb_msm_run(c, it->second, (const uint8_t*)d_scalars, n, batch, (uint8_t*)d_out_jac, &done));
        if (done) return H2AGG_OK;
    }
    // MSMs per set of launches: the level-1 sort partitions (batch * W * NB >> sub_bits, sub_bits <= 11) must fit its
    // LDS counters, and the entry count its 32-bit offsets
    // fixed-base levels (h2agg_bases_precompute).  Levels at c = 20 pay only through their own sort, which takes one MSM at
    // a time and no sort knobs: where it does not apply (a configured context; a batch of short columns over a big table, which
    // would also want batch x 2^19 buckets) the levels are left alone and the ordinary path runs over the table — the two-array
    // sort over c = 20 levels measured 113 ms against the ordinary path's 74 (16 MSMs, 2^22 points).
    const bool fb_table = it->second.pre && it->second.pre_c == FB_C && !c->dbg_pre_big;
    const bool use_pre = it->second.pre && !c->cfg_c && (!fb_table || (fb_sort_knobs_clear(c) && (batch == 1 || n >= ((size_t)1 << 18))));
    const PreTable pt{it->second.pre, it->second.n, it->second.pre_c, it->second.pre_W};
    const MsmPlan p1 = make_plan(c, n, 1);
    const uint32_t nb1 = use_pre ? (1u << (pt.c - 1)) : p1.NB;
    const size_t sets1 = use_pre ? 1 : (size_t)p1.W;                               // bucket sets per MSM
    uint32_t ppw_min = nb1 >> 11;
    if (ppw_min < 1) ppw_min = 1;
    size_t per = (size_t)SORT_MAX_PW / (sets1 * ppw_min);
    const size_t ent1 = use_pre ? n * (size_t)pt.W : n * (size_t)p1.W * (p1.glv ? 2 : 1);
    if (per * ent1 >= ((size_t)1 << 31)) per = (((size_t)1 << 31) - 1) / ent1;
    if (per * n >= ((size_t)1 << 29)) per = (((size_t)1 << 29) - 1) / n;
    if (per < 1) per = 1;
    // From 2^20 points on an MSM fills the chip by itself and takes the digit-major sort / two-dimensional reduction, which
    // batches do not: one MSM after another, each one's tail under the next one's bulk (2^22 points: 6.1 -> 5.4 ms each)
    const bool one_by_one = use_pre ? (pt.c == FB_C && n >= ((size_t)1 << 18)) : n >= ((size_t)1 << 20);
    if (one_by_one) per = 1;
    const uint8_t* endo = nullptr;
    TRY(table_endo(c, it->second, &endo));
    const bool was_overlap = c->tail_overlap;
    {
        OverlapScope overlap(c, one_by_one && batch > 1);
        MsmCall call;
        call.d_bases = it->second.d;
        call.n_base = n;
        call.d_endo_x = use_pre ? nullptr : endo;
        call.pre = use_pre ? &pt : nullptr;
        call.no_identity = !use_pre && it->second.no_identity;
        for (size_t q = 0; q < batch; q += per) {
            call.d_scalars = (const uint8_t*)d_scalars + 32 * n * q;
            call.d_out_jac = (uint8_t*)d_out_jac + 96 * q;
            call.batch = (uint32_t)(batch - q < per ? batch - q : per);
            TRY(msm_run(c, call));
        }
    }
    if (one_by_one && batch > 1 && !was_overlap) TRY(join_tails(c));   // without overlap mode the caller's stream orders the results
    return H2AGG_OK;
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_g1_msm_device(h2agg_ctx* c, uint64_t handle, const void* d_scalars, size_t n, uint8_t out[96]) try {
    TRY(bind(c));
    if (!out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    set_identity_jac(out);
    TRY(clear_flags(c));
    TRY(h2agg_g1_msm_device_async(c, handle, d_scalars, n, c->d_res_jac));
    return fetch_result_jac(c, out);
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_g1_msm_preloaded(h2agg_ctx* c, uint64_t handle, const uint8_t* scalars, size_t n, uint8_t out[96]) try {
    TRY(bind(c));
    if (!out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    set_identity_jac(out);
    if (n == 0) return fail(c, H2AGG_ERR_EMPTY, "multi_exp of zero pairs (reference panics: mock/arith/ecc.rs:128)");
    if (!scalars) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_b, 32 * n));
    HIP_TRY(c, hipMemcpyAsync(c->in_b.p, scalars, 32 * n, hipMemcpyHostToDevice, c->stream));
    return h2agg_g1_msm_device(c, handle, c->in_b.p, n, out);
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

// assign_instance_commitment for one instance column (verify.rs:601-603, 623-639)
int h2agg_instance_commitment(h2agg_ctx* c, uint64_t g_lagrange_handle, const uint8_t* instance, size_t len,
                              size_t max_len, uint8_t out_jac[96]) try {
    TRY(bind(c));
    if (!out_jac) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    set_identity_jac(out_jac);
    if (len > max_len)
        return fail(c, H2AGG_ERR_INVALID, "assert!(instance.len() <= params.n() - (blinding_factors + 1)) failed (verify.rs:601-603)");
    if (len == 0) return H2AGG_OK;  // None => pchip.assign_const(identity)  (verify.rs:638)
    return h2agg_g1_msm_preloaded(c, g_lagrange_handle, instance, len, out_jac);
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_host_alloc(h2agg_ctx* c, size_t bytes, void** out) try {
    TRY(bind(c));
    if (!out || bytes == 0) return fail(c, H2AGG_ERR_INVALID, "null out or zero size");
    hipError_t e = hipHostMalloc(out, bytes, hipHostMallocDefault);
    if (e != hipSuccess) return fail(c, H2AGG_ERR_NOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    return H2AGG_OK;
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}
int h2agg_host_free(h2agg_ctx* c, void* p) try {
    TRY(bind(c));
    if (p) HIP_TRY(c, hipHostFree(p));
    return H2AGG_OK;
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

}   // extern "C"
namespace {
// h2agg_g1_msm / h2agg_g1_msm_jac: host buffers in.  stride = 64: canonical affine bases; 96: canonical Jacobian points,
// normalised on the device (k_jac_to_mont_affine) where the affine entry point converts to Montgomery form (k_bases_to_mont)
int msm_host(h2agg_ctx* c, const uint8_t* bases, size_t stride, const uint8_t* scalars, size_t n, uint8_t out[96]);
}
extern "C" {
int h2agg_g1_msm(h2agg_ctx* c, const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t out[96]) try {
    return msm_host(c, bases, 64, scalars, n, out);
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}
int h2agg_g1_msm_jac(h2agg_ctx* c, const uint8_t* points_jac, const uint8_t* scalars, size_t n, uint8_t out[96]) try {
    return msm_host(c, points_jac, 96, scalars, n, out);
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;
} catch (...) {
    return H2AGG_ERR_INVALID;
}
}   // extern "C"
namespace {
int msm_host(h2agg_ctx* c, const uint8_t* bases, size_t stride, const uint8_t* scalars, size_t n, uint8_t out[96]) {
    TRY(bind(c));
    if (!out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    set_identity_jac(out);
    if (n == 0) return fail(c, H2AGG_ERR_EMPTY, "multi_exp of zero pairs (reference panics: mock/arith/ecc.rs:128)");
    if (!bases || !scalars) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_a, stride * n));
    TRY(ensure(c, c->in_b, 32 * n));
    TRY(ensure(c, c->tmp_bases, 64 * n));
    TRY(clear_flags(c));
    // Large inputs are cut into slices that cross PCIe on a copy stream while the previous slice is being computed
    // (an MSM is a sum over points, so the slices' results just add up): 96 B/point of transfer hide under ~1.7 ns/point
    // of arithmetic, instead of preceding it.  Slices of >= 2^19 points keep the per-MSM efficiency (2^18-point slices lose more than the overlap gains).
    const bool chain_env_off = !c->dbg_pcie_chain;
    const bool chained = !chain_env_off;
    // chained slices (below) of ~200 K points: the transfer (1.73 ns/point) and the slice's sort + accumulation (~90 us +
    // 1.3 ns/point) then take turns of equal length — measured, profiles/r03_sweeps.txt section 10: 2^20 points 3.03 / 2.97 /
    // 2.92 / 2.96 / 3.15 ms with 3 / 4 / 5 / 6 / 8 slices
    const size_t MIN_SLICE = chained ? (size_t)200 << 10 : (size_t)1 << 19;
    size_t nslices = chained ? (n + MIN_SLICE / 2) / MIN_SLICE : n / MIN_SLICE;
    if (nslices > MSM_MAX_SLICES) nslices = MSM_MAX_SLICES;
    const int env_slices = c->dbg_pcie_slices;   // (h2agg_debug_configure "pcie_slices": tests vary it per call)
    if (env_slices >= 1 && env_slices <= MSM_MAX_SLICES && n >= ((size_t)1 << 10) * (size_t)env_slices) nslices = (size_t)env_slices;
    if (nslices < 2) {
        HIP_TRY(c, hipMemcpyAsync(c->in_a.p, bases, stride * n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->in_b.p, scalars, 32 * n, hipMemcpyHostToDevice, c->stream));
        if (stride == 96)
            hipLaunchKernelGGL(k_jac_to_mont_affine, dim3(grid_for(c, (n + TA_K - 1) / TA_K)), dim3(BLOCK), 0, c->stream,
                               (const uint8_t*)c->in_a.p, n, (uint8_t*)c->tmp_bases.p, c->d_flags);
        else
            hipLaunchKernelGGL(k_bases_to_mont, dim3(grid_for(c, n)), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->in_a.p, n,
                               (uint8_t*)c->tmp_bases.p, c->d_flags);
        TRY(msm_run(c, MsmCall{(const uint8_t*)c->tmp_bases.p, (const uint8_t*)c->in_b.p, n, c->d_res_jac}));
        return fetch_result_jac(c, out);
    }
    TRY(ensure(c, c->out, 96 * MSM_MAX_SLICES));
    // the copy stream must not overwrite in_a / in_b while earlier work on the main stream still reads them
    HIP_TRY(c, hipEventRecord(c->ev_ready, c->stream));
    HIP_TRY(c, hipStreamWaitEvent(c->copy_stream, c->ev_ready, 0));
    const size_t per = (n + nslices - 1) / nslices;
    // The slices share one bucket set (chain modes of msm_run): slice k only sorts its keys and adds its points to the bucket
    // sums; ONE reduction / window-sum / Horner chain follows the last slice — that chain (0.6-0.9 ms of pure latency) is what
    // is left exposed behind the last byte of the transfer, so the slices can be small.  H2AGG_PCIE_CHAIN=0: the earlier
    // scheme (every slice a whole MSM, results added) for A/B runs.
    const int chain_glv_env = c->dbg_pcie_glv;
    MsmCall call;
    if (chained) {
        call.chain_n = n;
        call.chain_glv = chain_glv_env ? chain_glv_env > 0 : (c->cfg_glv >= 0 && n < ((size_t)1 << 22));
    }
    int rc = H2AGG_OK;
    size_t done = 0, k = 0;
    OverlapScope overlap(c);
    for (; done < n && rc == H2AGG_OK; done += per, ++k) {
        const size_t m = n - done < per ? n - done : per;
        chaos_wait(16, c->copy_stream);
        hipError_t e = hipMemcpyAsync((uint8_t*)c->in_b.p + 32 * done, scalars + 32 * done, 32 * m, hipMemcpyHostToDevice,
                                      c->copy_stream);
        if (e == hipSuccess) e = hipEventRecord(c->ev_copy_s[k], c->copy_stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync((uint8_t*)c->in_a.p + stride * done, bases + stride * done, stride * m, hipMemcpyHostToDevice,
                               c->copy_stream);
        if (e == hipSuccess) e = hipEventRecord(c->ev_copy[k], c->copy_stream);
        // the sort of a slice only reads its scalars: it runs while the slice's bases are still on their way (chained
        // slices; the earlier scheme waits for both, as it always did)
        if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, chained ? c->ev_copy_s[k] : c->ev_copy[k], 0);
        if (e != hipSuccess) {
            rc = fail(c, H2AGG_ERR_HIP, hipGetErrorString(e));
            break;
        }
        auto convert = [=](hipStream_t st) {
            if (stride == 96)
                hipLaunchKernelGGL(k_jac_to_mont_affine, dim3(grid_for(c, (m + TA_K - 1) / TA_K)), dim3(BLOCK), 0, st,
                                   (const uint8_t*)c->in_a.p + 96 * done, m, (uint8_t*)c->tmp_bases.p + 64 * done, c->d_flags);
            else
                hipLaunchKernelGGL(k_bases_to_mont, dim3(grid_for(c, m)), dim3(BLOCK), 0, st,
                                   (const uint8_t*)c->in_a.p + 64 * done, m, (uint8_t*)c->tmp_bases.p + 64 * done, c->d_flags);
        };
        if (chained) {
            call.chain = done == 0 ? CHAIN_FIRST : (done + per >= n ? CHAIN_LAST : CHAIN_MID);
            hipEvent_t ev_bases = c->ev_copy[k];
            c->bases_hook = [=](hipStream_t st) -> int {
                HIP_TRY(c, hipStreamWaitEvent(st, ev_bases, 0));
                convert(st);
                return H2AGG_OK;
            };
        } else {
            convert(c->stream);
        }
        call.d_bases = (const uint8_t*)c->tmp_bases.p + 64 * done;
        call.d_scalars = (const uint8_t*)c->in_b.p + 32 * done;
        call.n_base = m;
        call.d_out_jac = chained ? c->d_res_jac : (uint8_t*)c->out.p + 96 * k;
        rc = msm_run(c, call);
        c->bases_hook = nullptr;
    }
    overlap.restore();
    TRY(rc);
    TRY(join_tails(c));
    if (!chained)
        hipLaunchKernelGGL(k_g1_sum, dim3(1), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->out.p, k, c->d_res_jac, c->d_flags);
    return fetch_result_jac(c, out);
}
}   // namespace
extern "C" {

int h2agg_eval_flat(h2agg_ctx* c, const uint8_t* pts, const uint8_t* scalars, const uint8_t* has_scalar, size_t n,
                    uint8_t out[96]) try {
    TRY(bind(c));
    if (!out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    set_identity_jac(out);
    if (n && (!pts || !scalars || !has_scalar)) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    // host-side partition of the flat list (evaluation.rs:189-196): entries with / without a scalar
    std::vector<uint8_t> ps, ss, pn;
    for (size_t i = 0; i < n; ++i) {
        if (has_scalar[i]) {
            ps.insert(ps.end(), pts + 64 * i, pts + 64 * i + 64);
            ss.insert(ss.end(), scalars + 32 * i, scalars + 32 * i + 32);
        } else {
            pn.insert(pn.end(), pts + 64 * i, pts + 64 * i + 64);
        }
    }
    const size_t m = ss.size() / 32, k = pn.size() / 64;
    if (m == 0) return fail(c, H2AGG_ERR_EMPTY, "multi_exp of zero pairs (reference panics: mock/arith/ecc.rs:128)");
    TRY(ensure(c, c->in_a, 64 * m));
    TRY(ensure(c, c->in_b, 32 * m));
    TRY(ensure(c, c->in_c, 64 * k + 64));
    TRY(ensure(c, c->tmp_bases, 64 * m));
    HIP_TRY(c, hipMemcpyAsync(c->in_a.p, ps.data(), 64 * m, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->in_b.p, ss.data(), 32 * m, hipMemcpyHostToDevice, c->stream));
    if (k) HIP_TRY(c, hipMemcpyAsync(c->in_c.p, pn.data(), 64 * k, hipMemcpyHostToDevice, c->stream));
    // pageable-host sources must stay alive until the copies are done
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    TRY(clear_flags(c));
    hipLaunchKernelGGL(k_bases_to_mont, dim3(grid_for(c, m)), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->in_a.p, m,
                       (uint8_t*)c->tmp_bases.p, c->d_flags);
    TRY(msm_run(c, MsmCall{(const uint8_t*)c->tmp_bases.p, (const uint8_t*)c->in_b.p, m, nullptr}));
    TRY(join_tails(c));
    hipLaunchKernelGGL(k_eval_tail, dim3(1), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->d_res_xyzz,
                       (const uint8_t*)c->in_c.p, k, c->d_res_jac, c->d_flags);
    return fetch_result_jac(c, out);
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

// ---------------------------------------------------------------- tuning / measurement
int h2agg_msm_configure(h2agg_ctx* c, int window_bits, int reduce_segment, int big_bucket_threshold) try {
    if (!c) return H2AGG_ERR_INVALID;
    if (window_bits != 0 && (window_bits < 2 || window_bits > 20))
        return fail(c, H2AGG_ERR_INVALID, "window_bits must be 0 or in [2, 20]");
    if (reduce_segment < 0 || (reduce_segment & (reduce_segment - 1)))
        return fail(c, H2AGG_ERR_INVALID, "reduce_segment must be 0 or a power of two");
    if (big_bucket_threshold < 0) return fail(c, H2AGG_ERR_INVALID, "big_bucket_threshold must be >= 0");
    c->cfg_c = window_bits;
    c->cfg_seg = reduce_segment;
    c->cfg_big = big_bucket_threshold;
    return H2AGG_OK;
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_msm_configure_glv(h2agg_ctx* c, int mode) try {
    if (!c) return H2AGG_ERR_INVALID;
    if (mode < -1 || mode > 1) return fail(c, H2AGG_ERR_INVALID, "mode must be -1 (off), 0 (auto) or 1 (on)");
    c->cfg_glv = mode;
    return H2AGG_OK;
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}
int h2agg_msm_configure_lanes_per_bucket(h2agg_ctx* c, int lanes) try {
    if (!c) return H2AGG_ERR_INVALID;
    if (lanes != 0 && lanes != 1 && lanes != 2 && lanes != 4 && lanes != 8 && lanes != 16)
        return fail(c, H2AGG_ERR_INVALID, "lanes must be 0, 1, 2, 4, 8 or 16");
    c->cfg_lpb = lanes;
    return H2AGG_OK;
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_msm_configure_sort(h2agg_ctx* c, int sub_bits, int tile) try {
    if (!c) return H2AGG_ERR_INVALID;
    if (sub_bits != 0 && (sub_bits < 4 || sub_bits > SORT_MAX_SUB_BITS))
        return fail(c, H2AGG_ERR_INVALID, "sub_bits must be 0 or in [4, 12]");
    if (tile != 0 && tile != -1 && tile != -2 && tile != -3 && (tile < BLOCK || tile > (1 << 16)))
        return fail(c, H2AGG_ERR_INVALID, "tile must be 0, -1, -2 or in [256, 65536]");
    c->cfg_sub_bits = sub_bits;
    c->cfg_no_stage = tile == -1;   // -1: force the direct two-array sort kernels
    c->cfg_no_dm = tile == -3;      // -3: packed two-level sort even where the digit-major one applies
    c->cfg_stage_l1 = tile == -2;   // -2: also stage level 1 through LDS (experiment: slower, kept for tests)
    c->cfg_tile = tile > 0 ? tile : 0;
    return H2AGG_OK;
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_debug_configure(h2agg_ctx* c, const char* key, int value) try {
    if (!c || !key) return H2AGG_ERR_INVALID;
    const std::string k(key);
    if (k == "pcie_slices") c->dbg_pcie_slices = value;
    else if (k == "pcie_glv") c->dbg_pcie_glv = value;
    else if (k == "pcie_chain") c->dbg_pcie_chain = value;
    else if (k == "comb_msm") c->dbg_comb_msm = value;
    else if (k == "plan_cache") c->dbg_plan_cache = value;
    else if (k == "small_sort") c->dbg_small_sort = value;   // 0: small MSMs take the packed two-level sort again
    else if (k == "eval_split") c->dbg_eval_split = value;   // 0: an evaluation's two multi_exps are two MSMs again
    else if (k == "shard_fail") c->dbg_shard_fail = value;   // tests: this rank of a sharded aggregation fails before (1) / between (2) the exchanges, or inside exchange 1 (3) / 2 (4) before its all-gather
    else if (k == "lean_acc") {   // 0: the bucket accumulation through the generic kernel (k_msm_accumulate) instead of the lean one
#ifdef H2AGG_MEASURE_KNOBS
        c->dbg_lean_acc = value;
#else
        if (value != 1) return fail(c, H2AGG_ERR_INVALID, "h2agg_debug_configure: the generic accumulation kernel is in the measure build only (build_ext.py --measure)");
#endif
    }
    else if (k == "tape_lds") {
        if (c->dbg_tape_lds != value) agg_plans_release(c);   // (kept recordings carry their tape in one encoding or the other)
        c->dbg_tape_lds = value;
    }       // 0: every Fr tape through k_tape_run (register file in L2) instead of the LDS one
    else if (k == "prewake") c->dbg_prewake = value;         // 0: the sponge workers sleep until their chains are posted (A/B of the pre-wake)
    else if (k == "phases") c->dbg_phases = value;           // 1: every h2agg_verify_aggregation* call keeps its wall-clock split for h2agg_last_phases
    else if (k == "seg_chunk") c->dbg_seg_chunk = value;     // segmented multi_exp: at most n points per set of launches (0 = automatic)
    else if (k == "seg_c") {                                 // segmented multi_exp: window bits 4 .. 8 (0 = default)
        if (value != 0 && (value < 4 || value > 8)) return fail(c, H2AGG_ERR_INVALID, "h2agg_debug_configure: seg_c must be 0 or 4 .. 8");
        c->dbg_seg_c = value;
    }
    else if (k == "fr_fft_local") {                          // Fr FFT: radix-2 stages fused per pass, 1 .. 11 (0 = the default, 10)
        if (value < 0 || value > (int)FR_FFT_TILE_LOG) return fail(c, H2AGG_ERR_INVALID, "h2agg_debug_configure: fr_fft_local must be 0 or 1 .. 11");
        c->dbg_fr_fft_local = value;
    }
    else if (k == "fr_fft_batch_chunk") {                    // Fr FFT: a batch runs in chunks of this many columns (0 = as many as the work array holds)
        if (value < 0) return fail(c, H2AGG_ERR_INVALID, "h2agg_debug_configure: fr_fft_batch_chunk must be >= 0");
        c->dbg_fr_fft_batch_chunk = value;
    }
    else if (k == "fr_poly_chunk") {                         // KZG openings: log2 of the coefficients per workgroup, 3 .. 11 (0 = the default, 11)
        if (value != 0 && (value < (int)FR_CHUNK_PER_LOG || value > (int)FR_CHUNK_LOG)) return fail(c, H2AGG_ERR_INVALID, "h2agg_debug_configure: fr_poly_chunk must be 0 or 3 .. 11");
        c->dbg_fr_poly_chunk = value;
    }
    else if (k == "fr_scan_chunk") {                         // grand products: log2 of the elements per workgroup, 3 .. 11 (0 = the default, 11)
        if (value != 0 && (value < (int)FR_CHUNK_PER_LOG || value > (int)FR_CHUNK_LOG)) return fail(c, H2AGG_ERR_INVALID, "h2agg_debug_configure: fr_scan_chunk must be 0 or 3 .. 11");
        c->dbg_fr_scan_chunk = value;
    }
    else if (k == "fr_sort_tile") {                          // lookup permutation: log2 of the keys per workgroup, 4 .. 11 (0 = the default, 11)
        if (value != 0 && (value < (int)LK_TILE_LOG_MIN || value > (int)LK_TILE_LOG)) return fail(c, H2AGG_ERR_INVALID, "h2agg_debug_configure: fr_sort_tile must be 0 or 4 .. 11");
        c->dbg_fr_sort_tile = value;
    }
    else if (k == "commit_chunk") {
        if (value < 0) return fail(c, H2AGG_ERR_INVALID, "h2agg_debug_configure: commit_chunk must be >= 0");
        c->dbg_commit_chunk = value;
    }
    else if (k == "lean_full") c->dbg_lean_full = value;     // 1: the bucket accumulation keeps its identity test and endomorphism select whatever the table / plan
    else if (k == "pre_big") c->dbg_pre_big = value;         // 1: h2agg_bases_precompute takes any explicit width (levels through the two-array sort)
    else return fail(c, H2AGG_ERR_INVALID, "h2agg_debug_configure: unknown key " + k);
    return H2AGG_OK;
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_debug_lean_variant(int table_no_identity, int plan_glv) {
    return msm_lean_variant(table_no_identity != 0, plan_glv != 0);
}

int h2agg_debug_table_identity(h2agg_ctx* c, uint64_t handle, int* may_hold_out, int* last_variant_out) try {
    TRY(bind(c));
    if (may_hold_out) {
        auto it = c->tables.find(handle);
        if (it == c->tables.end()) return fail(c, H2AGG_ERR_INVALID, "unknown base-table handle");
        *may_hold_out = it->second.no_identity ? 0 : 1;
    }
    if (last_variant_out) *last_variant_out = c->last_lean_variant;
    return H2AGG_OK;
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_msm_set_tail_overlap(h2agg_ctx* c, int enable) try {
    TRY(bind(c));
    TRY(join_tails(c));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->tail_overlap = enable != 0;
    if (enable >= 1 && enable <= 3) c->overlap_level = enable;
    return H2AGG_OK;
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_profile_enable(h2agg_ctx* c, int enable) try {
    TRY(bind(c));
    if (enable && !c->prof_events_created) {
        for (int r = 0; r < h2agg_ctx::PROF_RING; ++r)
            for (int s = 0; s < ST_N; ++s)
                for (int k = 0; k < 2; ++k) HIP_TRY(c, hipEventCreateWithFlags(&c->prof[r].ev[s][k], EV_TIME_FLAGS));
        c->prof_events_created = true;
    }
    if (!enable) profile_harvest_all(c);
    c->profiling = enable != 0;
    c->prof_only = (enable >= 2 && enable - 2 < ST_N) ? enable - 2 : -1;
    return H2AGG_OK;
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}
int h2agg_profile_reset(h2agg_ctx* c) try {
    if (!c) return H2AGG_ERR_INVALID;
    profile_harvest_all(c);
    for (int s = 0; s < ST_N; ++s) {
        c->stage_ms[s] = 0;
        c->stage_launches[s] = 0;
    }
    return H2AGG_OK;
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}
int h2agg_profile_stage_count(h2agg_ctx*) { return ST_N; }
const char* h2agg_profile_stage_name(h2agg_ctx*, int i) { return (i >= 0 && i < ST_N) ? STAGE_NAMES[i] : ""; }
int h2agg_profile_stage_get(h2agg_ctx* c, int i, double* total_ms, uint64_t* launches) try {
    if (!c || i < 0 || i >= ST_N) return H2AGG_ERR_INVALID;
    profile_harvest_all(c);
    if (total_ms) *total_ms = c->stage_ms[i];
    if (launches) *launches = c->stage_launches[i];
    return H2AGG_OK;
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

// ---------------------------------------------------------------- pairing check (host)
extern "C++" {
namespace {
// csrc/transcript.inc (HostPool): if a pool worker is spinning for work, `on_worker` runs there while `here` runs on the
// calling thread, both done on return (true); otherwise nothing has run (false)
bool host_pool_pair_if_awake(const std::function<void()>& on_worker, const std::function<void()>& here);
bool pairing_adx_ok() {
#ifdef H2AGG_PAIRING_ADX_BUILD
    static const bool ok = __builtin_cpu_supports("bmi2") && __builtin_cpu_supports("adx") && !getenv("H2AGG_PAIRING_PORTABLE");
    return ok;
#else
    return false;
#endif
}
template <class P>
int pairing_load(h2agg_ctx* c, const uint8_t* g1_aff, const uint8_t* g2_aff, size_t n, std::vector<typename P::G1>& ps,
                 std::vector<typename P::G2>& qs) {
    if (n && (!g1_aff || !g2_aff)) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    ps.resize(n);
    qs.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const int r1 = P::load1(g1_aff + 64 * i, ps[i]);
        if (r1 == 1) return fail(c, H2AGG_ERR_NONCANONICAL, "pairing: G1 coordinate >= p");
        if (r1) return fail(c, H2AGG_ERR_BAD_POINT, "pairing: G1 point not on the curve");
        const int r2 = P::load2(g2_aff + 128 * i, qs[i]);
        if (r2 == 1) return fail(c, H2AGG_ERR_NONCANONICAL, "pairing: G2 coordinate >= p");
        if (r2 == 2) return fail(c, H2AGG_ERR_BAD_POINT, "pairing: G2 point not on the twist");
        if (r2) return fail(c, H2AGG_ERR_BAD_POINT, "pairing: G2 point outside the order-r subgroup");
    }
    return H2AGG_OK;
}
template <class P>
int pairing_product_t(h2agg_ctx* c, const uint8_t* g1_aff, const uint8_t* g2_aff, size_t n, uint8_t out_gt[384]) {
    std::vector<typename P::G1> ps;
    std::vector<typename P::G2> qs;
    TRY(pairing_load<P>(c, g1_aff, g2_aff, n, ps, qs));
    // (prepared lines: a G2 point that comes back — [s]_2, [1]_2 of one ParamsKZG — pays its doubling / addition steps once)
    std::vector<std::shared_ptr<const typename P::Prepared>> keep(n);
    std::vector<const typename P::Prepared*> preps(n);
    for (size_t i = 0; i < n; ++i) {
        keep[i] = P::prepared(g2_aff + 128 * i, false, qs[i]);
        preps[i] = keep[i].get();
    }
    P::product_prepared(ps, preps, out_gt);
    return H2AGG_OK;
}
template <class P>
int pairing_check_t(h2agg_ctx* c, const uint8_t* g1_aff, const uint8_t* g2_aff, size_t n, int* ok) {
    std::vector<typename P::G1> ps;
    std::vector<typename P::G2> qs;
    TRY(pairing_load<P>(c, g1_aff, g2_aff, n, ps, qs));
    *ok = P::check(ps, qs) ? 1 : 0;
    return H2AGG_OK;
}
// e(left, [s]_2) * e(right, -[1]_2) == 1 ?   (verify.rs:733-739: `n_g2_prepared = -params.g2()`)
template <class P>
int final_pair_check_t(h2agg_ctx* c, const uint8_t left_aff[64], const uint8_t right_aff[64], const uint8_t s_g2[128], const uint8_t g2[128],
                       int* ok) {
    uint8_t g1s[128], g2s[256];
    memcpy(g1s, left_aff, 64);
    memcpy(g1s + 64, right_aff, 64);
    memcpy(g2s, s_g2, 128);
    memcpy(g2s + 128, g2, 128);
    std::vector<typename P::G1> ps;
    std::vector<typename P::G2> qs;
    TRY(pairing_load<P>(c, g1s, g2s, 2, ps, qs));
    P::negate(qs[1]);
    const std::shared_ptr<const typename P::Prepared> keep[2] = {P::prepared(s_g2, false, qs[0]), P::prepared(g2, true, qs[1])};
    const std::vector<const typename P::Prepared*> preps = {keep[0].get(), keep[1].get()};
    // With a pool worker already awake and waiting (h2agg_verify_aggregation wakes one while the evaluation is on the device),
    // the second pair's Miller loop runs there beside the first one's here: 64 squarings + 89 sparse products per thread
    // instead of 64 + 178 on one — the loop part of the check 0.25 -> 0.16 ms.  Without one (a busy pool: many calls in
    // flight; a direct call of this entry point) both pairs share one loop, which is less work in total.
    typename P::Gt f0, f1;
    const bool split = host_pool_pair_if_awake(
        [&] { f1 = P::miller_prepared(std::vector<typename P::G1>{ps[1]}, std::vector<const typename P::Prepared*>{preps[1]}); },
        [&] { f0 = P::miller_prepared(std::vector<typename P::G1>{ps[0]}, std::vector<const typename P::Prepared*>{preps[0]}); });
    *ok = (split ? P::check_product(f0, f1) : P::check_prepared(ps, preps)) ? 1 : 0;
    return H2AGG_OK;
}
}  // namespace
}  // extern "C++"

int h2agg_pairing_product(h2agg_ctx* c, const uint8_t* g1_aff, const uint8_t* g2_aff, size_t n, uint8_t out_gt[384]) try {
    if (!out_gt) return fail(c, H2AGG_ERR_INVALID, "null buffer");
#ifdef H2AGG_PAIRING_ADX_BUILD
    if (pairing_adx_ok()) return pairing_product_t<pairing_adx::Api>(c, g1_aff, g2_aff, n, out_gt);
#endif
    return pairing_product_t<pairing::Api>(c, g1_aff, g2_aff, n, out_gt);
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_pairing_check(h2agg_ctx* c, const uint8_t* g1_aff, const uint8_t* g2_aff, size_t n, int* ok) try {
    if (!ok) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    *ok = 0;
#ifdef H2AGG_PAIRING_ADX_BUILD
    if (pairing_adx_ok()) return pairing_check_t<pairing_adx::Api>(c, g1_aff, g2_aff, n, ok);
#endif
    return pairing_check_t<pairing::Api>(c, g1_aff, g2_aff, n, ok);
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

// ParamsKZG's g2 / s_g2 as stored by ParamsKZG::write (fs.rs:40-55 reads them back through halo2_proofs): 64-byte
// compressed G2 points -> the 128-byte affine form the pairing entry points take
int h2agg_g2_batch_decompress(h2agg_ctx* c, const uint8_t* in, size_t n, uint8_t* out_aff) try {
    if (n && (!in || !out_aff)) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    for (size_t i = 0; i < n; ++i) {
        pairing::G2Affine q;
        const int r = pairing::g2_decompress(in + 64 * i, q);
        if (r == 1) return fail(c, H2AGG_ERR_NONCANONICAL, "G2 coordinate >= p");
        if (r) return fail(c, H2AGG_ERR_BAD_POINT, "invalid G2 point encoding (x^3 + b is not a square)");
        pairing::g2_to_bytes(q, out_aff + 128 * i);
    }
    return H2AGG_OK;
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_final_pair_check(h2agg_ctx* c, const uint8_t left_aff[64], const uint8_t right_aff[64], const uint8_t s_g2[128],
                           const uint8_t g2[128], int* ok) try {
    if (!ok || !left_aff || !right_aff || !s_g2 || !g2) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    *ok = 0;
#ifdef H2AGG_PAIRING_ADX_BUILD
    if (pairing_adx_ok()) return final_pair_check_t<pairing_adx::Api>(c, left_aff, right_aff, s_g2, g2, ok);
#endif
    return final_pair_check_t<pairing::Api>(c, left_aff, right_aff, s_g2, g2, ok);
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

}  // extern "C"

#include "schema_api.inc"
#include "transcript.inc"
#include "seg_msm.inc"
#include "comm.inc"
#include "verifier.inc"
#include "verify_run.inc"
#include "fr_host.inc"
#include "params.inc"
#include "fr_fft.inc"
#include "poly_open.inc"
#include "prod.inc"
#include "lookup.inc"
#include "quotient.inc"
#include "keygen.inc"
