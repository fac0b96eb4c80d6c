// libh2agg.so — the context and its life (create / destroy / stream / synchronize); the C ABI declared in include/h2agg.h is
// in the families included at the end of this file, one .inc each, on top of csrc/host.inc.
// Everything numeric runs in the HIP kernels of batch_kernels.hpp / msm_kernels.hpp; there is no CPU
// arithmetic path in this library (a context cannot be created without a HIP device).
#include "../../include/h2agg.h"

#include <hip/hip_runtime.h>

#include <chrono>
#include <climits>
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

#include "hip_owners.hpp"
#include "scalar_mul_kernels.hpp"
#include "lp_kernels.hpp"
#include "seg_msm_kernels.hpp"
#include "g1_fft_kernels.hpp"
#include "fr_fft_kernels.hpp"
#include "poly_kernels.hpp"
#include "shplonk_kernels.hpp"
#include "prod_kernels.hpp"
#include "lookup_kernels.hpp"
#include "quotient_kernels.hpp"
#include "keygen_kernels.hpp"
#include "witness_kernels.hpp"
#include "columns_kernels.hpp"
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
#include "schema_shplonk.hpp"   // (behind schema.hpp, which poseidon_kernels.hpp brings in)
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

enum Stage {
    ST_PART_COUNT = 0, ST_PART_SCATTER, ST_BUCKET_SORT, ST_ORDER, ST_ACCUM, ST_ACCUM_BIG, ST_REDUCE, ST_WINDOW_SUM,
    ST_FINAL, ST_N
};
const char* const STAGE_NAMES[ST_N] = {"msm_part_count", "msm_part_scatter",   "msm_bucket_sort",
                                       "msm_order",      "msm_accumulate",     "msm_accumulate_big",
                                       "msm_reduce",     "msm_window_sum",     "msm_final"};

struct Table {   // owns its device buffers: they go with it, behind a synchronisation of whatever may still read them
    DevMem d;        // Montgomery affine, 64 B / point
    DevMem endo_x;   // beta * x, 32 B / point (made on the first GLV MSM over this table)
    size_t n = 0;
    // the call that wrote the table stored no identity base (flags[1], batch_kernels.hpp): MSMs over it take the bucket
    // accumulation without the per-entry identity test.  false = not known: "may hold one" (msm_lean_variant)
    bool no_identity = false;
    // fixed-base levels (h2agg_bases_precompute): pre[(w * n + i) * 64] = 2^(pre_c * w) * P_i, w < pre_W
    DevMem pre;
    int pre_c = 0, pre_W = 0;
    // comb of the first comb_n bases (k_comb_table_build with bases; made on the first small MSM over a table that has
    // fixed-base levels, i.e. one its owner declared constant): comb[((b * 32 + w) * 255 + d - 1) * 64] = d * 2^(8w) * P_b
    DevMem comb;
    size_t comb_n = 0;
    std::vector<DevMem> comb_retired;   // smaller combs this one replaced: kernels in flight may still read them, so they
                                        // are freed where the table's other buffers are (behind a synchronisation)
    Table() = default;
    Table(Table&&) = default;
    void free_combs() {
        comb.reset();
        comb_n = 0;
        comb_retired.clear();
    }
};
struct ColumnStore {   // a slab [m][2^k] of canonical Fr behind a handle (csrc/columns.inc): owns it, as a Table owns its columns
    DevMem d;
    size_t m = 0;
    unsigned k = 0;
    size_t col() const { return (size_t)32 << k; }   // bytes of a column
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
    // ---- The handles the context owns (csrc/hip_owners.hpp).  h2agg_destroy synchronises every stream that may hold work and
    // then deletes the context; members die in reverse order of declaration.  So everything declared BELOW this block goes
    // first: the base tables, the grow-only buffers and the pinned blocks, and each hipFree among them waits for the device
    // once more.  Then the events, then the streams, the context's own stream last: memory goes while the streams that
    // ordered its users still exist, an event goes before the streams it was recorded on.  (h2agg_create's failure path
    // deletes a context behind nothing but place_streams' probes, in the same order.)
    static constexpr int TAIL_SLOTS = 3;    // tail streams (see below)
    static constexpr int PROF_RING = 32;    // per-call event sets of the profile (see below)
    static constexpr int N_STREAMS = 1 + TAIL_SLOTS + 3 + 4;
    Stream streams[N_STREAMS];   // in the order h2agg_create makes them: own, tails, accumulation, aux, copy, four spares.
                                 // The role members below are plain handles into this array (place_streams permutes them)
    Event ev_aux, ev_aux_go;
    Event ev_copy[MSM_MAX_SLICES], ev_copy_s[MSM_MAX_SLICES], ev_ready;
    Event ev_bulk[TAIL_SLOTS], ev_tail[TAIL_SLOTS];
    Event ev_sortdone, ev_sorted[2], ev_accdone[2];
    struct ProfSlot {
        Event ev[ST_N][2];   // made by the first h2agg_profile_enable
        bool used[ST_N] = {};
        bool pending = false;
    };
    ProfSlot prof[PROF_RING];
    // ---- end of the owned handles

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
    PinnedBuf h_pinned;               // pinned staging for small results / flags (its first 4 KiB are used)

    // schema-layer scratch (grow-only; the schema API is synchronous, one evaluation is in flight per context):
    // the Fr register file, the uploaded staging block, per-side MSM scalars / Montgomery bases, pinned staging
    DevBuf sch_regs, sch_in, sch_scalars[2], sch_bases[2], sch_endo;
    PinnedBuf h_stage;
    PinnedBuf h_down;                 // page-locked landing block of the from-bytes call's downloads (csrc/verify_run.inc)
    const void* sch_owner = nullptr;  // the schema whose tape sch_regs reflects
    struct AggPlanCache* agg_plans = nullptr;   // recorded aggregations kept for the next call of the same shape (csrc/verifier.inc)

    // host-buffer MSM: slices are copied on this stream while the previous slice is computed
    hipStream_t copy_stream = nullptr;
    hipStream_t spare_streams[4] = {};   // what place_streams() did not give a role (see there)
    // verifier pipeline: point decompression of a circuit's proofs runs here, beside the instance-column MSMs
    hipStream_t aux_stream = nullptr;

    std::map<uint64_t, Table> tables;
    std::map<uint64_t, ColumnStore> stores;   // Fr column stores (csrc/columns.inc); handles come from the tables' counter
    uint64_t next_handle = 1;

    // multi-GPU: this context's rank in an RCCL communicator (csrc/comm.inc); ncclComm_t kept opaque here
    void* comm = nullptr;
    int comm_rank = 0, comm_size = 0;

    // h2agg_debug_configure: test hooks read per call.  One member per key of DEBUG_KEYS (csrc/config_api.inc), with the key's
    // default; include/h2agg.h "Test hooks" documents them.
    int dbg_pcie_slices = 0;          // h2agg_g1_msm's host buffers cut into n slices (0 = automatic)
    int dbg_pcie_glv = 0;             // GLV for those slices: -1 off, 1 on (0 = automatic)
    int dbg_pcie_chain = 1;           // 0: every slice a whole MSM, results added, instead of one shared bucket set
    int dbg_comb_msm = 1;             // 0: small MSMs over tables with fixed-base levels take the bucket path, not the comb
    int dbg_plan_cache = 1;           // 0: h2agg_verify_aggregation records every call anew
    int dbg_small_sort = 1;           // 0: small MSMs take the packed two-level sort again
    int dbg_eval_split = 1;           // 0: an evaluation's two multi_exps are two MSMs again
    int dbg_lean_acc = 1;             // 0: the bucket accumulation through the generic kernel (k_msm_accumulate; measure build only)
    int dbg_lean_full = 0;            // 1: every bucket accumulation takes the instantiation for any table / any plan
    int dbg_pre_big = 0;              // 1: h2agg_bases_precompute takes any explicit width (levels through the two-array sort)
    int dbg_tape_lds = 1;             // 0: every Fr tape through k_tape_run (register file in L2) instead of the LDS one
    int dbg_prewake = 1;              // 0: the sponge workers sleep until their chains are posted (A/B of the pre-wake)
    int dbg_phases = 0;               // 1: every h2agg_verify_aggregation* call keeps its wall-clock split for h2agg_last_phases
    int dbg_shard_fail = 0;           // tests: this rank of a sharded aggregation fails before (1) / between (2) the exchanges, or inside exchange 1 (3) / 2 (4)
    int dbg_seg_chunk = 0;            // segmented multi_exp: points per set of launches (0 = automatic)
    int dbg_seg_c = 0;                // segmented multi_exp: window bits 4 .. 8 (0 = default)
    int dbg_fr_fft_local = 0;         // Fr FFT: radix-2 stages fused per pass (0 = FR_FFT_LOCAL)
    int dbg_fr_fft_batch_chunk = 0;   // Fr FFT: columns per set of launches of a batched transform (0 = by the work array)
    int dbg_fr_poly_chunk = 0;        // KZG openings: log2 of the coefficients per workgroup (0 = FR_CHUNK_LOG)
    int dbg_fr_scan_chunk = 0;        // grand products: log2 of the elements per workgroup (0 = FR_CHUNK_LOG)
    int dbg_fr_sort_tile = 0;         // lookup permutation: log2 of the keys per workgroup (0 = LK_TILE_LOG)
    int dbg_commit_chunk = 0;         // h2agg_commit_columns: columns per set of MSM launches (0 = by the work-memory budget)
    int dbg_launch_cus = 0;           // grid-stride launches capped by the CU count: compute units the cap counts (0 = cu_count)
    int dbg_shard_calls = 0;          // (no key: the all-gathers of the sharded call in progress, counted for shard_fail 3 / 4)
    uint32_t table_word = 0;                // flags[1] as the last finish() read it: the creating call stored an identity base
    int last_lean_variant = -1;             // VAR of the last lean accumulation launched (h2agg_debug_table_identity)
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
    // KZG openings (csrc/poly_open.inc): the chunk values of every level above the coefficients, the queries / group lists of
    // the call in progress, the combined polynomials (then their quotients) of a multiopen, its Jacobian commitments
    DevBuf poly_work, poly_desc, poly_slab, poly_jac;
    // grand products (csrc/prod.inc): the num and den columns of a permutation / lookup call (den: then R^2 / den, also for
    // h2agg_fr_grand_product), the chunk products of every level above the elements, the two-level table of w^i
    DevBuf prod_num, prod_den, prod_lvl, prod_tab;
    // lookup permutation (csrc/lookup.inc): the key buffers, rank columns, count matrix, histograms and plans of a call
    // (lk_layout), the descriptor of a compression, the status words of a batch (one per lookup)
    DevBuf lk_work, lk_desc, lk_status;
    // quotient polynomial (csrc/quotient.inc): a coset's value slab with the columns behind it and the extended evaluations
    // (qt_layout), the compiled programs and the permutation columns' places, the two-level table of w^i
    DevBuf qt_work, qt_prog, qt_tab;
    // keygen (csrc/keygen.inc): one bit per cell of a permutation's mapping, the table of delta^c, the Jacobian commitments of a
    // slab commit
    DevBuf kg_bitmap, kg_delta, kg_jac;
    // witness check (csrc/witness.inc): the flag lines of a chunk of constraints, the tile sums and minima of its report, a
    // lookup's two theta-folds, the report (wc_layout); programs go to qt_prog, the sort works in lk_work
    DevBuf wc_work;
    std::string last_phases;   // debug key phases: the last h2agg_verify_aggregation's wall-clock split (h2agg_last_phases)
    // tuning
    int cfg_c = 0, cfg_seg = 0, cfg_big = 0, cfg_sub_bits = 0, cfg_tile = 0;
    int cfg_glv = 0;   // 0 = auto, 1 = on, -1 = off
    int cfg_lpb = 0;   // lanes per bucket in the accumulate kernel: 0 = auto, 1 / 2 / 4 / 8 / 16
    int cfg_quotient_split = 0;   // h2agg_quotient_configure: 1 = every quotient takes the coset-split ending (0: only where k + e > 24)
    size_t cfg_lookup_chunk = 0;   // h2agg_lookup_configure: most lookups per set of launches of a batch (0: by the rows, csrc/lookup.inc)
    bool cfg_no_stage = false, cfg_stage_l1 = false, staged_attr_set = false, cfg_no_dm = false, dm_attr_set = false, r2d_attr_set = false;

    // optional overlap of the serial tail (k_msm_final) of MSM k with the bulk of MSM k+1
    bool tail_overlap = false;
    int overlap_level = 2;  // 1: only the Horner tail on the second stream; 2: reduction + window sums + tail
    // TAIL_SLOTS tail streams used round-robin, each with its own buckets / segsum / wsum set: the latency-shaped
    // tails of consecutive MSMs overlap one another as well as the next MSMs' bulk (small MSMs are otherwise
    // bound by one tail chain: ~0.7 ms per MSM at 2^14 points against 0.5 ms of bulk).
    // what a tail reads: one independent allocation per slot, so MSMs with DIFFERENT plans (bucket counts, segment
    // counts, window counts) in flight on different slots can never alias one another, whatever their sizes
    DevBuf r2d_ticket[TAIL_SLOTS];
    DevBuf buckets[TAIL_SLOTS], segsum[TAIL_SLOTS], wsum[TAIL_SLOTS];
    hipStream_t tail_streams[TAIL_SLOTS] = {};
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
    hipStream_t acc_stream = nullptr;
    bool accdone_pending[2] = {};
    int sort_par = 0;

    // profiling: a ring of per-call event sets (prof[PROF_RING]), harvested lazily so that measuring does not serialise
    // back-to-back asynchronous MSMs
    bool profiling = false;
    int prof_only = -1;   // >= 0: only this stage is bracketed (one event pair per MSM instead of nine)
    bool prof_events_created = false;
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

#define TRY(expr)                      \
    do {                               \
        int rc_ = (expr);              \
        if (rc_ != H2AGG_OK) return rc_; \
    } while (0)

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

// what h2agg_destroy releases first
void comm_release(h2agg_ctx* c);        // csrc/comm.inc
void agg_plans_release(h2agg_ctx* c);   // csrc/verifier.inc

}  // namespace

#include "host.inc"
namespace {
#include "msm_run.inc"
}  // namespace

extern "C" {

int h2agg_create(int device_ordinal, h2agg_ctx** out) try {
    if (!out) return H2AGG_ERR_INVALID;
    *out = nullptr;
    int count = 0;
    if (device_ordinal < 0 || hipGetDeviceCount(&count) != hipSuccess || device_ordinal >= count)
        return H2AGG_ERR_HIP;  // no CPU mode: a HIP device is required
    if (hipSetDevice(device_ordinal) != hipSuccess) return H2AGG_ERR_HIP;
    std::unique_ptr<h2agg_ctx> ctx(new h2agg_ctx());   // every failure below is a plain return: the owners release what was made
    h2agg_ctx* c = ctx.get();
    c->device = device_ordinal;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) != hipSuccess) return H2AGG_ERR_HIP;
    c->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    char buf[256];
    snprintf(buf, sizeof buf, "h2agg 0.1 %s cu=%d", prop.gcnArchName, c->cu_count);
    c->desc = buf;
    // The streams, in a fixed order: the own stream, the tail streams, the accumulation's, then the auxiliary stream, the copy
    // stream and four spares.  The last six are made HERE, behind the others, not at their first use: where the runtime places
    // a stream depends on how many streams the process has made before it (profiles/r03_sweeps.txt section 18: back-to-back
    // MSMs run at 1.25 or at 1.55 ms per step depending on the number of streams made between the main stream and the tail
    // streams), and a placement that changes with what else the process did first is not reproducible.
    // H2AGG_TAIL_PRIO / H2AGG_ACC_PRIO (experiments): -1 = lowest, 1 = highest priority for the tail / accumulation streams
    static const int tail_prio = knob("H2AGG_TAIL_PRIO") ? atoi(knob("H2AGG_TAIL_PRIO")) : 0;
    static const int acc_prio = knob("H2AGG_ACC_PRIO") ? atoi(knob("H2AGG_ACC_PRIO")) : 0;
    int pr_lo = 0, pr_hi = 0;
    hipDeviceGetStreamPriorityRange(&pr_lo, &pr_hi);   // lo = least (numerically greatest)
    const int tail_pr = tail_prio < 0 ? pr_lo : pr_hi, acc_pr = acc_prio < 0 ? pr_lo : pr_hi;
    Stream* s = c->streams;
    if (s->create(hipStreamNonBlocking) != hipSuccess || ensure_pinned(c, c->h_pinned, 4096, "result staging") != H2AGG_OK ||
        ensure(c, c->small, 4096) != H2AGG_OK)
        return H2AGG_ERR_HIP;
    for (int i = 1; i < h2agg_ctx::N_STREAMS; ++i) {
        const int* pr = i <= h2agg_ctx::TAIL_SLOTS ? (tail_prio ? &tail_pr : nullptr)
                                                   : (i == h2agg_ctx::TAIL_SLOTS + 1 && acc_prio ? &acc_pr : nullptr);
        if (s[i].create(hipStreamNonBlocking, pr) != hipSuccess) return H2AGG_ERR_HIP;
    }
    c->stream = c->own_stream = *s++;
    for (hipStream_t& t : c->tail_streams) t = *s++;
    c->acc_stream = *s++;
    c->aux_stream = *s++;
    c->copy_stream = *s++;
    for (hipStream_t& t : c->spare_streams) t = *s++;
    // the events, each with the flags of its use: device-scope ordering between the MSM's streams, plain ordering for the rest
    bool ok = c->ev_aux.create(hipEventDisableTiming) == hipSuccess && c->ev_aux_go.create(hipEventDisableTiming) == hipSuccess &&
              c->ev_ready.create(hipEventDisableTiming) == hipSuccess && c->ev_sortdone.create(EV_SYNC_FLAGS) == hipSuccess;
    for (int k = 0; k < MSM_MAX_SLICES; ++k)
        ok = ok && c->ev_copy[k].create(hipEventDisableTiming) == hipSuccess && c->ev_copy_s[k].create(hipEventDisableTiming) == hipSuccess;
    for (int k = 0; k < h2agg_ctx::TAIL_SLOTS; ++k)
        ok = ok && c->ev_bulk[k].create(EV_SYNC_FLAGS) == hipSuccess && c->ev_tail[k].create(EV_SYNC_FLAGS) == hipSuccess;
    for (int q = 0; q < 2; ++q)
        ok = ok && c->ev_sorted[q].create(EV_SYNC_FLAGS) == hipSuccess && c->ev_accdone[q].create(EV_SYNC_FLAGS) == hipSuccess;
    if (!ok) return H2AGG_ERR_HIP;
    c->d_flags = (uint32_t*)c->small.p;
    c->d_res_xyzz = (uint8_t*)c->small.p + 1024;   // 144 B
    c->d_res_jac = (uint8_t*)c->small.p + 256;   // 96 B
    hipMemset(c->small.p, 0, 4096);
    if (place_streams(c) != H2AGG_OK) return H2AGG_ERR_HIP;
    *out = ctx.release();
    return H2AGG_OK;
} API_CATCH

// What no destructor can do: the communicator and the recorded plans go, a tail that still waits is launched, and every
// stream that may hold work is waited for (c->stream may be the caller's).  The owners do the rest, in the order the
// context's declaration states.
void h2agg_destroy(h2agg_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    comm_release(c);
    agg_plans_release(c);
    flush_deferred_tail(c, false);
    if (c->stream) hipStreamSynchronize(c->stream);
    for (Stream& s : c->streams)
        if (s) hipStreamSynchronize(s);
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
} API_CATCH

int h2agg_synchronize(h2agg_ctx* c) try {
    TRY(bind(c));
    TRY(join_tails(c));
    // also the place where status flags raised by asynchronous calls surface (e.g. a scalar >= r handed to
    // h2agg_g1_msm_device_async -> H2AGG_ERR_NONCANONICAL here)
    TRY(clear_flags(c));
    return finish(c);
} API_CATCH

}  // extern "C"

#include "chips_api.inc"
#include "bases_api.inc"
#include "msm_api.inc"
#include "config_api.inc"
#include "pairing_api.inc"
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
#include "shplonk.inc"
#include "prod.inc"
#include "lookup.inc"
#include "quotient.inc"
#include "keygen.inc"
#include "pk.inc"
#include "witness.inc"
#include "columns.inc"
