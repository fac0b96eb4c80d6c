// The host side of one multi_exp (included by h2agg.hip; DESIGN.md section 5.1 "host side").  Every MSM of the library goes
// through msm_run below, in five steps that are functions of their own:
//     msm_route   every decision, from the call and a const context: no HIP call, no allocation       -> MsmRoute
//     msm_bind    grows the context's buffers and derives this call's pointers (sort slot, tail slot)   -> MsmWorkspace
//     msm_sort / msm_order / msm_accumulate / msm_big_kernels / msm_tail     the launches, one stage each
// The plain types (MsmCall, MsmRoute, MsmWorkspace, MsmTailJob) stand in h2agg.hip above the context, which keeps a deferred
// tail by value.

// ---- the plan ---------------------------------------------------------------------------------------------------------------
// bits of the scalar that fall into the top window (a narrow top window means a few huge buckets).
// plain: 254-bit scalars, W*c >= 255; GLV: 127-bit magnitudes, W*c >= 128
int window_count(int c, bool glv) { return glv ? (128 + c - 1) / c : (255 + c - 1) / c; }
int top_window_bits(int c, bool glv) { return (glv ? 127 : 254) - c * (window_count(c, glv) - 1); }
int choose_window(size_t n, bool glv) {
    // Measured on MI355X (tools/window_sweep.py, profiles/r01_window_sweep_*.txt).  Two things decide it, and the
    // classic "log2(n) - 4" rule sees neither: (1) the tail (bucket reduce -> window sums -> Horner) is a serial
    // chain whose length grows with the number of windows, so below ~2^17 points FEWER, WIDER windows win even
    // though they leave most buckets empty; (2) only widths whose top window is as sparse as the others
    // (GLV 8/13/16, plain 8/15/16: top window as sparse as the others) avoid a dense top window that costs as much as all the
    // other windows together.
    // (re-measured in round 4 behind the one-launch sort and the limb-parallel Horner chain, profiles/r04_sweeps.txt section 5:
    // 8 bits up to 2^12 points — 2^11: 0.457 against 0.490 ms alone, 0.194 against 0.250 back to back; 2^12 equal; the two
    // multi_exps of an evaluation of 4 proofs, 1 750 pairs: 0.68 against 0.76 ms)
    if (glv) return n <= ((size_t)1 << 12) ? 8 : n <= ((size_t)1 << 14) ? 13 : 16;
    // 17 bits from 1.5 * 2^20 points on: a bucket costs 2 general additions (~2.8 insertions) whatever the point count, a
    // window's insertions grow with it — 15 windows of 2^16 buckets overtake 16 of 2^15 between 2^20 points (+0.7 %) and
    // 2^21 (+5.7 %; 2^22: +8.8 %, profiles/r03_sweeps.txt section 11)
    return n <= ((size_t)1 << 12) ? 8 : n < ((size_t)1 << 19) ? 15 : n < ((size_t)3 << 19) ? 16 : 17;
}

// glv_mode: 0 = the context's setting (h2agg_msm_configure_glv), 1 / -1 = on / off whatever the context says (a chain's
// caller fixes the split for all its slices)
MsmPlan make_plan(const h2agg_ctx* c, size_t n, uint32_t batch = 1, int glv_mode = 0) {
    MsmPlan p;
    const int cfg_glv = glv_mode ? glv_mode : c->cfg_glv;
    // GLV halves the latency-shaped stages (reduction, Horner tail) at the price of the decomposition pass and the
    // slice-combine pass of the half-as-many buckets: a win whenever those stages are exposed — single-MSM latency
    // mode, or small / medium MSMs — and a small loss when a large MSM's tail is hidden under the next one's bulk
    // (profiles/r01_sweeps.txt), or when the tail is a small share anyway.  auto = on unless (overlap mode and n >= 2^20) or
    // n >= 2^22.
    p.glv = cfg_glv > 0 || (cfg_glv == 0 && !(c->tail_overlap && n >= ((size_t)1 << 20)) && n < ((size_t)1 << 22));
    p.c = c->cfg_c ? c->cfg_c : choose_window(n, p.glv);
    p.W = window_count(p.c, p.glv);
    p.NB = 1u << (p.c - 1);
    p.NBT = (uint32_t)p.W * batch * p.NB;   // a batch of MSMs over one table is one MSM with batch x W windows
    // segment length of the bucket reduction: ~1024 waves of running sums (profiles/r01_sweeps.txt)
    // (short segments = short chains; when the tail is hidden under the next MSM's bulk its WORK is what costs, and the
    // double-and-add by the segment offset — as much work as 8 buckets of running sums — amortises over longer segments)
    uint32_t seg = c->cfg_seg ? (uint32_t)c->cfg_seg
                              : (p.NBT >= (1u << 18) ? (c->tail_overlap && p.NBT >= (1u << 19) ? 32u : 8u)
                                                     : (p.NBT >= (1u << 15) ? 4u : 2u));
    if (seg > p.NB) seg = p.NB;
    p.seg = seg;
    p.spw = p.NB / seg;
    p.big = c->cfg_big ? (uint32_t)c->cfg_big : 256u;
    return p;
}

// Tail overlap forced to level 2 while the guard lives (slices of one MSM, the MSMs of a one-by-one batch, the evaluation's two
// multi_exps: their callers join before they return); the context's own setting comes back on every way out.
struct OverlapScope {
    h2agg_ctx* c;
    const bool was_overlap;
    const int was_level;
    explicit OverlapScope(h2agg_ctx* c_, bool force = true) : c(c_), was_overlap(c_->tail_overlap), was_level(c_->overlap_level) {
        if (force) {
            c->tail_overlap = true;
            c->overlap_level = 2;
        }
    }
    void restore() {
        c->tail_overlap = was_overlap;
        c->overlap_level = was_level;
    }
    ~OverlapScope() { restore(); }
    OverlapScope(const OverlapScope&) = delete;
    OverlapScope& operator=(const OverlapScope&) = delete;
};

// ---- the route --------------------------------------------------------------------------------------------------------------
// The experiment switches of msm_run (measure build; a shipped library reads none: knob() is nullptr there), read once.
struct MsmKnobs {
    int par4_env;         // H2AGG_PAR4: 4 lanes per chain in the bucket reduction / window sums, > 0 on, < 0 off
    bool dm_env_off;      // H2AGG_SORT=packed
    bool small_env_off;   // H2AGG_SMALL_SORT=0
    // (experiment knob: 256-thread workgroups + H2AGG_ACC_LDS pin the accumulation at exactly N waves per SIMD and leave the rest
    // of the CU — registers and LDS — to whatever else is in flight; see profiles/r03_sweeps.txt section 10)
    int acc_block;        // H2AGG_ACC_BLOCK (the generic accumulation only)
    int acc_lds;          // H2AGG_ACC_LDS, experiment: unused LDS per wave caps the occupancy
    bool r2d_env_off;     // H2AGG_REDUCE=segments keeps the segment kernels
    bool final_par4;      // H2AGG_FINAL=par4
    bool defer_env_off;   // H2AGG_DEFER_TAILS=0
#ifdef H2AGG_MEASURE_KNOBS
    // the generic kernel (compiler-scheduled formulas, 166 VGPRs) lives in the measure build only, behind the debug key
    // lean_acc = 0 / H2AGG_ACC=generic, for A/B runs; the shipped library carries the lean one alone (VERDICT r5 item 6)
    bool lean_env;
    bool lean_dual;       // (H2AGG_ACC=lean1: one chain per product instead of two in lock step: an A/B variant, not in the shipped library)
    int dbg_skip;         // H2AGG_DBG_SKIP, timing experiments only (WRONG results): 1 skips the bucket reduction, 2 the window sums, 4 the Horner tail
#else
    static constexpr int dbg_skip = 0;   // (a shipped library has no switch that changes results)
#endif
};
const MsmKnobs& msm_knobs() {
    static const MsmKnobs k = [] {
        const auto is = [](const char* name, const char* value) { return knob(name) && !strcmp(knob(name), value); };
        const auto num = [](const char* name, int dflt) { return knob(name) ? atoi(knob(name)) : dflt; };
        MsmKnobs k{};
        k.par4_env = num("H2AGG_PAR4", 0);
        k.dm_env_off = is("H2AGG_SORT", "packed");
        k.small_env_off = is("H2AGG_SMALL_SORT", "0");
        k.acc_block = num("H2AGG_ACC_BLOCK", 64);
        k.acc_lds = num("H2AGG_ACC_LDS", 0);
        k.r2d_env_off = is("H2AGG_REDUCE", "segments");
        k.final_par4 = is("H2AGG_FINAL", "par4");
        k.defer_env_off = is("H2AGG_DEFER_TAILS", "0");
#ifdef H2AGG_MEASURE_KNOBS
        k.lean_env = !is("H2AGG_ACC", "generic");
        k.lean_dual = !is("H2AGG_ACC", "lean1");
        k.dbg_skip = num("H2AGG_DBG_SKIP", 0);
#endif
        return k;
    }();
    return k;
}

// the (level, point) sort of fb_sort_kernels.hpp has no sort / segment knobs: a context configured with any
// (h2agg_msm_configure_sort, reduce_segment) does not take it
bool fb_sort_knobs_clear(const h2agg_ctx* c) {
    return !c->cfg_no_dm && !c->cfg_no_stage && !c->cfg_stage_l1 && !c->cfg_sub_bits && !c->cfg_tile && !c->cfg_seg;
}
// a forced sort configuration keeps the packed / two-array kernels: no one-launch sort, no digit-major sort
bool sort_knobs_clear(const h2agg_ctx* c) { return !c->cfg_no_stage && !c->cfg_stage_l1 && !c->cfg_sub_bits && !c->cfg_tile; }

// Which instantiation of the lean bucket accumulation a call takes (msm_kernels.hpp VAR): the identity test stays unless the
// table is KNOWN to hold none, the endomorphism select stays when the plan splits scalars.  Pure: h2agg_debug_lean_variant.
int msm_lean_variant(bool table_no_identity, bool plan_glv) {
    return (table_no_identity ? 0 : LEAN_ID) | (plan_glv ? LEAN_ENDO : 0);
}
// what the creating call's base-table word says about the table it wrote (word: flags[1] as finish() read it)
bool table_word_clear(uint32_t word) { return word == 0; }

using AccLeanKernel = decltype(&k_msm_accumulate_lean<0, true>);
template <bool DUAL>
AccLeanKernel acc_lean_kernel(int chain, int var) {
    const int ch = chain == CHAIN_FIRST ? 1 : (chain == CHAIN_MID || chain == CHAIN_LAST) ? 2 : 0;
#define ACC_LEAN_ROW(CH)                                                                                      \
    case CH:                                                                                                   \
        return var == 0 ? k_msm_accumulate_lean_v<CH, DUAL, 0> : var == LEAN_ID ? k_msm_accumulate_lean_v<CH, DUAL, LEAN_ID> \
             : var == LEAN_ENDO ? k_msm_accumulate_lean_v<CH, DUAL, LEAN_ENDO> : k_msm_accumulate_lean<CH, DUAL>;
    switch (ch) {
        ACC_LEAN_ROW(1)
        ACC_LEAN_ROW(2)
        default:
        ACC_LEAN_ROW(0)
    }
#undef ACC_LEAN_ROW
}

// the plan of a call: the context's plan for its size, or what the table's fixed-base levels dictate
void route_plan(const h2agg_ctx* c, const MsmCall& call, bool fbdm, MsmRoute& r) {
    const PreTable* pre = call.pre;
    MsmPlan& p = r.p;
    // (a chain's caller fixed the point count the plan is made for and the split, for all its slices)
    p = r.chain ? make_plan(c, call.chain_n, r.batch, call.chain_glv ? 1 : -1) : make_plan(c, call.n_base, r.batch);
    r.Wd = p.W;                               // digit positions per scalar (what the recoding loops over)
    if (pre) {
        p.glv = false;
        p.c = pre->c;
        r.Wd = pre->W;
        p.W = 1;                              // one bucket set per MSM
        p.NB = 1u << (p.c - 1);
        p.NBT = fbdm ? FB_NBT : r.batch * p.NB;   // (the top digit's own slots: fb_sort_kernels.hpp)
        // measured (tools/instance_seg_sweep.py, 2^17-point columns): 16-bucket segments up to 8 MSMs per batch, 32 beyond
        p.seg = c->cfg_seg ? (uint32_t)c->cfg_seg : (r.batch >= 16 ? 32u : 16u);
        if (p.seg > p.NB) p.seg = p.NB;
        p.spw = p.NB / p.seg;
    }
    r.W1 = p.W;                               // windows (bucket sets) per MSM
    r.WT = (uint32_t)r.W1 * r.batch;          // windows in total
    r.nent = r.n * (size_t)r.Wd * (p.glv ? 2 : 1);   // bucket insertions
    if (!c->cfg_big) {
        // a lane walks a bucket alone up to `big` entries: 8x the mean keeps a denser top window (up to 4x the mean
        // when it holds c-2 bits) out of the workgroup-per-chunk path, whose LDS tree only pays for real outliers
        const size_t mean = r.nent / p.NBT;
        if (8 * mean > p.big) p.big = (uint32_t)(8 * mean);
    }
}

// the sort family of a call (r.sort) with its plans; fbdm: the call takes the fixed-base level sort
void route_sort(const h2agg_ctx* c, const MsmCall& call, bool fbdm, MsmRoute& r) {
    const MsmKnobs& K = msm_knobs();
    const PreTable* pre = call.pre;
    const MsmPlan& p = r.p;
    const uint32_t batch = r.batch;
    const size_t n = r.n;
    SortPlan& sp = r.sp;
    int want_sub = c->cfg_sub_bits ? c->cfg_sub_bits : SORT_SUB_BITS;
    if (pre && !c->cfg_sub_bits) {
        // one bucket set per MSM: keep >= 256 level-2 partitions (one workgroup each) so the sort still fills the chip
        while (want_sub > 4 && (((size_t)p.NB * batch) >> want_sub) < 256) --want_sub;
    }
    sp.sub_bits = (p.c - 1 < want_sub) ? p.c - 1 : want_sub;
    while ((r.WT * (p.NB >> sp.sub_bits)) > (uint32_t)SORT_MAX_PW && sp.sub_bits < p.c - 1 &&
           sp.sub_bits < SORT_MAX_SUB_BITS)
        ++sp.sub_bits;  // keep the level-1 partition count within its LDS counters
    sp.SB = 1u << sp.sub_bits;
    sp.ppw = p.NB >> sp.sub_bits;
    sp.PW = r.WT * sp.ppw;
    if (batch > 1 && !call.split) {
        sp.n_base = (uint32_t)call.n_base;
        sp.W1 = (uint32_t)r.W1;
    }
    if (pre) sp.pre_n = (uint32_t)pre->n_level;
    sp.tile = c->cfg_tile ? (uint32_t)c->cfg_tile : 2048u;
    // packed-item staged path: index field of 31 - sub_bits bits, a tile's keys must fit the LDS stage
    sp.glv = p.glv;
    r.idx_bits = (p.glv ? 30 : 31) - sp.sub_bits;   // packed item: sub | neg | (endo) | idx
    // items carry the BASE index (fixed-base mode: up to W * n_level of them)
    bool staged = !c->cfg_no_stage && (pre ? (size_t)pre->W * pre->n_level : call.n_base) <= ((size_t)1 << r.idx_bits);
    const size_t keys_per_scalar = (size_t)r.Wd * (p.glv ? 2 : 1);
    if (staged && c->cfg_stage_l1 && (size_t)sp.tile * keys_per_scalar > (size_t)STAGE_ITEMS_L1)
        sp.tile = (uint32_t)(STAGE_ITEMS_L1 / keys_per_scalar);
    if (staged && sp.tile < (uint32_t)BLOCK) staged = false;
    r.ntiles = (unsigned)((n + sp.tile - 1) / sp.tile);
    r.fb_ntile = (uint32_t)((n + FB_T - 1) / FB_T);
    // digit-major sort (sort_kernels.hpp): plain 16-bit windows over one table, 2^16 .. 2^22 points
    const size_t dm_row = p.glv ? 2 * n : n;   // keys per window (GLV: both halves of a scalar land in the same 8 windows)
    // (c = 17, plain scalars: 15 windows of 2^16 buckets, 16-bit magnitude codes + sign / zero bit rows — k_dm_digits17, k_dm_partition<true>)
    r.dm17 = p.c == 17 && !p.glv;
    const bool dm = !K.dm_env_off && !c->cfg_no_dm && sort_knobs_clear(c) && !pre && batch == 1 &&
                    (p.c == 16 || r.dm17) && dm_row >= ((size_t)1 << 16) && dm_row <= ((size_t)1 << 22);
    r.dm_nwin = p.glv ? 8u : (r.dm17 ? 15u : 16u);
    // the one-launch sort of small MSMs (sort_kernels.hpp k_small_sort); a forced sort configuration keeps its own kernels
    const bool small_sort = !K.small_env_off && c->dbg_small_sort && !pre && !dm && n <= (size_t)SMALL_SORT_N &&
                            p.NB <= (uint32_t)SMALL_SORT_NB && sort_knobs_clear(c);
    r.sort = small_sort ? SortKind::SMALL : fbdm ? SortKind::FB_LEVELS : dm ? SortKind::DIGIT_MAJOR
             : !staged ? SortKind::TWO_ARRAY : c->cfg_stage_l1 ? SortKind::PACKED_L1 : SortKind::PACKED;
    DmPlan& dp = r.dp;
    if (dm) {
        dp.n_pts = p.glv ? (uint32_t)(dm_row / 2) : 0xffffffffu;
        dp.n = (uint32_t)dm_row;
        dp.n_pad = r.dm17 ? (uint32_t)((dm_row + 63) & ~(size_t)63) : (uint32_t)((dm_row + 7) & ~(size_t)7);   // (17-bit windows: bit rows, 64 keys per word)
        dp.ntile = (uint32_t)((dm_row + DM_T1 - 1) / DM_T1);
        dp.n_row = dp.ntile * (uint32_t)DM_T1;
        dp.ppw = r.dm17 ? 128 : 64;   // (level 2 keeps <= 512 buckets per partition in LDS: sub_bits <= 9)
        while (dm_row / dp.ppw > 4096 && dp.ppw < (uint32_t)DM_MAX_PPW) dp.ppw *= 2;   // ~4 K keys per level-2 partition (8 K at 2^22)
        dp.sub_bits = p.c - 1;
        for (uint32_t q = dp.ppw; q > 1; q >>= 1) --dp.sub_bits;
        dp.SB = 1u << dp.sub_bits;
        dp.idx_bits = 31 - dp.sub_bits;
    }
    // per-tile partition counts from the counting pass, read back by the scatter pass (same tiles).  (A call in the
    // one-launch sort's range reserves what the packed sort of its size would.)
    r.tile_counts_bytes = fbdm ? (size_t)r.fb_ntile * (FB_NPART + 1) * 4
                          : dm ? (size_t)r.dm_nwin * dp.ntile * (dp.ppw + 1) * 4
                          : (staged && !c->cfg_stage_l1) ? (size_t)r.ntiles * sp.PW * 4 : 0;
}

MsmRoute msm_route(const h2agg_ctx* c, const MsmCall& call) {
    const MsmKnobs& K = msm_knobs();
    MsmRoute r{};
    const PreTable* pre = call.pre;
    const uint32_t split = call.split;
    r.batch = split ? 2 : call.batch;
    r.split = split;
    r.n_base = call.n_base;
    r.n = split ? call.n_base : call.n_base * r.batch;   // scalars
    const auto refuse = [&r](const char* msg) {
        r.refuse_code = H2AGG_ERR_INVALID;
        r.refuse_msg = msg;
        return r;
    };
    if (r.n >= ((size_t)1 << 30)) return refuse("n must be < 2^30");
    r.chain = (pre || r.batch != 1) ? CHAIN_OFF : call.chain;
    // fixed-base levels at c = 20 (tables of 2^18 .. 2^22 points): the (level, point) sort of fb_sort_kernels.hpp
    const bool fbdm = pre && r.batch == 1 && pre->c == FB_C && pre->W == FB_W && pre->n_level <= ((size_t)FB_MAX_TILES * FB_T) &&
                      fb_sort_knobs_clear(c);
    route_plan(c, call, fbdm, r);
    const MsmPlan& p = r.p;
    if (r.nent >= ((size_t)1 << 32)) return refuse("n * windows must be < 2^32");
    route_sort(c, call, fbdm, r);
    if (r.sp.PW > (uint32_t)SORT_MAX_PW) return refuse("too many sort partitions");
    if (split && (r.sort != SortKind::SMALL || split >= call.n_base)) return refuse("split MSM outside the one-launch sort's range");
    // ordering the buckets by length balances the lanes of a wave; with few entries the longest run bounds the kernel
    // either way and the three launches (~25 us) are pure latency
    r.ordered = r.nent >= ((size_t)1 << 16);
    // lanes per bucket: keep >= ~8192 waves in flight (3 per SIMD x 1024 SIMDs, 2-3 rounds) when buckets are few
    // With few buckets the kernel is bound by its longest run (one mixed add is ~6 us of dependent latency): 8 lanes
    // per bucket turn a 60-entry run into 8 entries + 7 adds of the combine.
    r.lpb = 1;
    if (c->cfg_lpb) r.lpb = (uint32_t)c->cfg_lpb;
    else   // ... but only while the mean run still covers the slices (measured, profiles/r01_sweeps.txt): sparse buckets
           // (small MSMs with wide windows) gain nothing from slices and pay lpb - 1 additions per bucket in the combine
        while (r.lpb < 8 && (size_t)p.NBT * r.lpb < (size_t)8192 * 64 &&
               (r.chain ? call.chain_n * (size_t)r.Wd * (p.glv ? 2 : 1) : r.nent) >= (size_t)r.lpb * p.NBT)
            r.lpb *= 2;   // (a chain's slices all cut their buckets alike: the slots are resumed)
    r.max_slots = r.nent / BIG_CHUNK + r.nent / ((size_t)p.big + 1) + 2;   // chunks of over-long buckets
    r.max_keys = r.nent / ((size_t)p.big + 1) + 2;
    // (no bucket can hold more keys than its bucket set receives: a multi_exp of a dozen points skips the two launches,
    // ~35 us at the head of its tail)
    r.big_possible = r.nent / r.WT > p.big;
#ifdef H2AGG_MEASURE_KNOBS
    r.lean = K.lean_env && c->dbg_lean_acc;
    r.lean_dual = K.lean_dual;
#else
    r.lean = true;
    r.lean_dual = true;
#endif
    r.lean_var = msm_lean_variant(call.no_identity && !c->dbg_lean_full, p.glv || c->dbg_lean_full);
    r.glv_here = p.glv && !split;          // (a split MSM's caller hands over the decomposed words and the beta * x column: k_eval_prep)
    r.endo_here = p.glv && !call.d_endo_x;
    // two-dimensional bucket reduction for 16-bit windows (msm_kernels.hpp); H2AGG_REDUCE=segments keeps the segment kernels
    const int r2d_lc = p.NB == (uint32_t)(R2D_ROWS * R2D<7>::COLS) ? 7 : p.NB == (uint32_t)(R2D_ROWS * R2D<8>::COLS) ? 8 : 0;
    const bool r2d = !K.r2d_env_off && !c->cfg_seg && !pre && r2d_lc != 0;
    r.tail = fbdm ? TailKind::FB_GRIDS : !r2d ? TailKind::SEGMENTS : r2d_lc == 7 ? TailKind::R2D7 : TailKind::R2D8;
    r.nseg_total = r.WT * p.spw;
    // 4 lanes per chain in the bucket reduction / window sums (latency) or 1 (least work): see msm_kernels.hpp
    // measured: wins up to 16384 segments (c <= 13; also a 2^20-point MSM with 32-bucket segments in throughput mode,
    // where 1 024 waves of 94-addition chains would otherwise outlast the step), loses to the extra work above
    // (a split MSM is two such MSMs side by side, each within the range)
    r.par4 = K.par4_env ? K.par4_env > 0 : r.nseg_total <= (split ? 32768u : 16384u);
    // overlap level 3 (see h2agg_ctx::acc_stream): this MSM's accumulation leaves the context's stream
    r.piped = c->tail_overlap && c->overlap_level >= 3;
    // overlap level >= 2: consecutive MSMs alternate between the two sets of sort outputs, so that what still reads one set
    // behind the accumulation (over-long-bucket kernels, zeroing of the counters: tail stream) never holds up the next sort
    r.altbuf = c->tail_overlap && c->overlap_level >= 2;
    // Buckets longer than `big` (skewed scalars; none for uniform ones, where the two launches only find empty lists):
    // with alternating sort outputs they leave the bulk stream and go in front of the bucket reduction on the tail stream,
    // followed by the zeroing of this slot's counters for the MSM after next.
    r.tail_big = r.altbuf && r.lpb == 1 && (r.chain == CHAIN_OFF || r.chain == CHAIN_LAST) && !split;
    // Everything after the bucket accumulation is latency-shaped (one wave per SIMD or less): bucket
    // reduction, per-window sums, Horner tail.  In overlap mode it runs on one of the context's tail streams, under the
    // accumulation of the next MSM; results are picked up by join_tails().  A split MSM's tail stays on the context's
    // stream — nothing follows that it could hide under, and a stream hand-over costs 10-20 us each way.
    r.tails_off_stream = r.altbuf && !split;
    r.final_off_stream = c->tail_overlap && !split;   // (overlap level 1: only the last chain leaves the stream)
    // The tail is launched from the NEXT MSM's call, behind that MSM's sort (h2agg_ctx::deferred_job).
    // deferral needs another MSM to carry it; a full per-stage profiling pass keeps every stage inside its own call
    // (and it only pays from 2^20 points on — measured, profiles/r02_sweeps.txt: below that the tail is a large share of the
    // MSM and wants to start at once; the two multi_exps of an evaluation in particular)
    // (not for the fixed-base levels of big tables: their sort's whole-CU workgroups collide with a tail either way — a tail always
    // ends up beside some later MSM's sort, profiles/r05_sweeps.txt section 1(g) — and the batch of 16 x 2^22 measures 71.6 ms with
    // the tail launched at once against 72.5 deferred)
    r.defer = r.tails_off_stream && !K.defer_env_off && !(c->profiling && c->prof_only < 0) && r.n >= ((size_t)1 << 20) && !fbdm;
    return r;
}

// can two MSMs of n_total points in all run as one split MSM (msm_run, MsmCall::split)?  The one-launch sort's range, nothing
// forced: what the route says of such a call (wherever the table is cut: only the refusal of an empty side looks at that)
bool msm_split_ok(const h2agg_ctx* c, size_t n_total) {
    MsmCall call;
    call.n_base = n_total;
    call.split = 1;
    return msm_route(c, call).refuse_code == H2AGG_OK;
}

// ---- the workspace ----------------------------------------------------------------------------------------------------------
// pmeta words: pcount [PW] | pstart [PW + 1] | pcursor [PW] | bin_count [SIZE_BINS] | bin_start [SIZE_BINS + 1] |
//              bin_cursor [SIZE_BINS] | big-bucket counters [2], each padded by 64 words
constexpr uint32_t META_PW = DM_MAX_PW;   // (the digit-major path has up to 16 x 512 partitions)
constexpr uint32_t M_PSTART = META_PW + 64, M_PCURSOR = M_PSTART + META_PW + 64,
                   M_BCOUNT = M_PCURSOR + META_PW + 64, M_BSTART = M_BCOUNT + SIZE_BINS + 64,
                   M_BCURSOR = M_BSTART + SIZE_BINS + 64, M_BIG = M_BCURSOR + SIZE_BINS + 64, M_WORDS = M_BIG + 64;

// Grows what the call needs and derives its pointers.  sq: the sort slot (overlap level >= 2 alternates between two sets of
// sort outputs), par: the tail slot.  An ensure() that has to replace a buffer launches a deferred tail and waits for the
// device first; the buffers of later stages (beta * x, decomposed scalars, slices, fix list, tickets) grow in their stages.
int msm_bind(h2agg_ctx* c, const MsmCall& call, const MsmRoute& r, MsmWorkspace& w) {
    const MsmPlan& p = r.p;
    const DmPlan& dp = r.dp;
    const bool fbdm = r.sort == SortKind::FB_LEVELS, dm = r.sort == SortKind::DIGIT_MAJOR;
    const int sq = w.sq = r.altbuf ? c->sort_par : 0;
    {
        const size_t cap0 = c->pmeta[sq].cap;
        TRY(ensure(c, c->pmeta[sq], M_WORDS * 4));
        if (c->pmeta[sq].cap != cap0) c->meta_clean[sq] = false;
    }
    TRY(ensure(c, c->hist[sq], (size_t)p.NBT * 4));
    TRY(ensure(c, c->offs[sq], (size_t)p.NBT * 4));
    TRY(ensure(c, c->order[sq], (size_t)p.NBT * 4));
    TRY(ensure(c, c->item_idx, fbdm ? (size_t)r.fb_ntile * FB_KEYS1 * 4 : dm ? (size_t)r.dm_nwin * dp.n_row * 4 : r.nent * 4));
    if (fbdm) TRY(ensure(c, c->fb_long, FB_LONG_WORDS * 4));   // very long partitions across workgroups (fb_sort_kernels.hpp)
    TRY(ensure(c, c->item_sub, fbdm ? 0 : dm ? (size_t)r.dm_nwin * dp.n_pad * 2 + (r.dm17 ? (size_t)2 * r.dm_nwin * (dp.n_pad / 8) : 0) : r.nent * 2));
    TRY(ensure(c, c->entries[sq], r.nent * 4));
    // buckets / segsum / wsum exist once per tail slot: in overlap mode the reduction of MSM k (tail stream)
    // runs while MSM k+1 fills the next slot's set.  (They were one allocation cut at par * this-plan's-size: two MSMs
    // with different plans in flight then overlapped — ADVICE r1.)
    const int par = w.par = c->parity;
    TRY(ensure(c, c->buckets[par], (size_t)p.NBT * XYZZ_BYTES));
    {   // (the two-dimensional reduction keeps 4096 partial sums per window there)
        const size_t r2d_records = p.NB == (uint32_t)(R2D_ROWS * R2D<7>::COLS) ? (size_t)r.WT * (R2D<7>::THREADS + 2)
                                   : p.NB == (uint32_t)(R2D_ROWS * R2D<8>::COLS) ? (size_t)r.WT * (R2D<8>::THREADS + 2) : 0;
        const size_t fb_records = fbdm ? (size_t)FB_R2D_WINDOWS * (R2D<7>::THREADS + 3) : 0;   // parts, halves, bucket sums
        TRY(ensure(c, c->segsum[par], std::max(std::max((size_t)r.nseg_total, r2d_records), fb_records) * XYZZ_BYTES));
    }
    TRY(ensure(c, c->wsum[par], (size_t)(fbdm ? FB_R2D_WINDOWS + 2 : r.WT) * XYZZ_BYTES));
    TRY(ensure(c, c->big_list[sq], r.max_slots * 12));
    TRY(ensure(c, c->big_keys[sq], r.max_keys * 12));
    TRY(ensure(c, c->big_part[sq], r.max_slots * XYZZ_BYTES));
    uint32_t* meta = w.meta = (uint32_t*)c->pmeta[sq].p;
    w.pcount = meta, w.pstart = meta + M_PSTART, w.pcursor = meta + M_PCURSOR;
    w.bin_count = meta + M_BCOUNT, w.bin_start = meta + M_BSTART, w.bin_cursor = meta + M_BCURSOR;
    w.big_count = meta + M_BIG;   // [0] chunk slots, [1] multi-chunk buckets (zeroed with the rest of meta)
    w.hist = (uint32_t*)c->hist[sq].p;
    w.offs = (uint32_t*)c->offs[sq].p;
    w.order = (uint32_t*)c->order[sq].p;
    w.item_idx = (uint32_t*)c->item_idx.p;
    w.item_sub = (uint16_t*)c->item_sub.p;
    w.fb_long = (uint32_t*)c->fb_long.p;
    w.entries = (uint32_t*)c->entries[sq].p;
    c->d_res_xyzz = (uint8_t*)c->small.p + 1024 + 144 * par;   // each tail slot has its own XYZZ result
    if (r.split) c->d_res_xyzz = (uint8_t*)c->small.p + 2048 + 2 * 144 * par;   // ... or its own two
    w.res_xyzz = c->d_res_xyzz;
    w.buckets = (uint8_t*)c->buckets[par].p;
    w.segsum = (uint8_t*)c->segsum[par].p;
    w.wsum = (uint8_t*)c->wsum[par].p;
    w.big_list = (uint32_t*)c->big_list[sq].p;
    w.big_keys = (uint32_t*)c->big_keys[sq].p;
    w.big_part = (uint8_t*)c->big_part[sq].p;
    w.tile_counts = nullptr;
    if (r.tile_counts_bytes) {
        TRY(ensure(c, c->tile_counts, r.tile_counts_bytes));
        w.tile_counts = (uint32_t*)c->tile_counts.p;
    }
    w.meta_was_clean = r.altbuf && c->meta_clean[sq];
    c->meta_clean[sq] = false;
    // the call's inputs and output, as the stages see them (msm_glv_prepare swaps in the scalars' decomposed words and the
    // beta * x column it makes; fixed-base levels: the level table)
    w.d_bases = call.pre ? call.pre->d : call.d_bases;
    w.d_scalars = call.d_scalars;
    w.d_endo_x = call.d_endo_x;
    w.d_out_jac = call.d_out_jac;
    w.acc_out = w.buckets;
    w.fix_list = nullptr;
    w.ticket = nullptr;
    return H2AGG_OK;
}

// ---- the stages -------------------------------------------------------------------------------------------------------------
void launch_bases_endo_x(h2agg_ctx* c, const MsmRoute& r, const MsmWorkspace& w, hipStream_t st) {
    hipLaunchKernelGGL(k_bases_endo_x, dim3(grid_for(c, r.n_base)), dim3(BLOCK), 0, st, w.d_bases, r.n_base, (uint8_t*)c->endo_buf.p);
}

// the beta * x column of a table that brought none, and the scalars' decomposition, in front of the sort
int msm_glv_prepare(h2agg_ctx* c, const MsmRoute& r, MsmWorkspace& w, hipStream_t st) {
    if (r.endo_here) {   // (with a bases hook the beta*x column is computed behind it, in front of the accumulation)
        TRY(ensure(c, c->endo_buf, r.n_base * 32));
        if (!c->bases_hook) launch_bases_endo_x(c, r, w, st);
        w.d_endo_x = (const uint8_t*)c->endo_buf.p;
    }
    debug_sync(1);
    chaos_wait(4, st);
    if (r.glv_here) {  // k = k1 + lambda*k2: the sort reads the decomposed words instead of the scalars
        TRY(ensure(c, c->glv_buf, r.n * 32));
        StageTimer t(c, ST_PART_COUNT);
        hipLaunchKernelGGL(k_glv_decompose, dim3(grid_for(c, r.n)), dim3(BLOCK), 0, st, w.d_scalars, r.n,
                           (uint8_t*)c->glv_buf.p, c->d_flags);
        w.d_scalars = (const uint8_t*)c->glv_buf.p;
    }
    return H2AGG_OK;
}

int sort_small(h2agg_ctx* c, const MsmRoute& r, const MsmWorkspace& w, hipStream_t st) {
    const MsmPlan& p = r.p;
    StageTimer t(c, ST_BUCKET_SORT);
    // (the length-ordering pass counts into the scratch words: then they are cleared as a whole)
    if (r.ordered && !w.meta_was_clean) HIP_TRY(c, hipMemsetAsync(w.meta, 0, M_WORDS * 4, st));
    hipLaunchKernelGGL(k_small_sort, dim3(r.WT), dim3(SMALL_SORT_TB), 0, st, w.d_scalars, (uint32_t)r.n, p.c, r.Wd,
                       (r.batch > 1 && !r.split) ? (uint32_t)r.n_base : 0u, r.split, p.glv, p.NB, w.hist, w.offs, w.entries, c->d_flags,
                       w.big_count);
    return H2AGG_OK;
}

int sort_fb(h2agg_ctx* c, const MsmRoute& r, const MsmWorkspace& w, hipStream_t st) {
    const uint32_t fb_ntile = r.fb_ntile, n_level = r.sp.pre_n;
    {
        StageTimer t(c, ST_PART_SCATTER);
        if (!w.meta_was_clean) HIP_TRY(c, hipMemsetAsync(w.meta, 0, M_WORDS * 4, st));
        hipLaunchKernelGGL(k_fb_partition, dim3(fb_ntile), dim3(FB_TB1), 0, st, w.d_scalars, (uint32_t)r.n, w.pcount, w.tile_counts, w.item_idx,
                           c->d_flags);
        hipLaunchKernelGGL(k_fb_scan_list, dim3(1), dim3(1024), 0, st, (const uint32_t*)w.pcount, w.pstart, fb_ntile, w.fb_long);
    }
    {
        StageTimer t(c, ST_BUCKET_SORT);
        hipLaunchKernelGGL(k_fb_bucket_sort, dim3(FB_NPART), dim3(FB_TB2), 0, st, (const uint32_t*)w.pstart, (const uint32_t*)w.tile_counts,
                           (const uint32_t*)w.item_idx, n_level, fb_ntile, w.hist, w.offs, w.entries);
        // partitions too long for the stage (skewed / small scalars): the very long ones split over workgroups, the rest one
        // workgroup each; with uniform scalars every workgroup of the three launches leaves at once
        hipLaunchKernelGGL(k_fb_long_count, dim3(FB_LONG_CAP, FB_LONG_S), dim3(FB_TB2), 0, st, (const uint32_t*)w.pstart,
                           (const uint32_t*)w.tile_counts, (const uint32_t*)w.item_idx, n_level, fb_ntile, w.fb_long, w.hist, w.offs);
        hipLaunchKernelGGL(k_fb_long_place, dim3(FB_LONG_CAP, FB_LONG_S), dim3(FB_TB2), 0, st, (const uint32_t*)w.pstart,
                           (const uint32_t*)w.tile_counts, (const uint32_t*)w.item_idx, n_level, fb_ntile,
                           (const uint32_t*)w.fb_long, w.entries);
        hipLaunchKernelGGL(k_fb_bucket_sort_long, dim3(FB_NPART), dim3(FB_TB2), 0, st, (const uint32_t*)w.pstart,
                           (const uint32_t*)w.tile_counts, (const uint32_t*)w.item_idx, n_level, fb_ntile,
                           (const uint32_t*)w.fb_long, w.hist, w.offs, w.entries);
    }
    return H2AGG_OK;
}

int sort_dm(h2agg_ctx* c, const MsmRoute& r, const MsmWorkspace& w, hipStream_t st) {
    const MsmPlan& p = r.p;
    const DmPlan& dp = r.dp;
    const uint32_t dm_nwin = r.dm_nwin, PW = dm_nwin * dp.ppw;
    {
        StageTimer t(c, ST_PART_COUNT);
        if (!w.meta_was_clean) HIP_TRY(c, hipMemsetAsync(w.meta, 0, M_WORDS * 4, st));
        const unsigned dg = (unsigned)((r.n + BLOCK * DM_DIG_PER - 1) / (BLOCK * DM_DIG_PER));
        if (p.glv)   // d_scalars: the decomposed words (range-checked by k_glv_decompose)
            hipLaunchKernelGGL(k_dm_digits_glv, dim3(dg), dim3(BLOCK), 0, st, w.d_scalars, (uint32_t)r.n, dp.n_pad, w.item_sub);
        else if (r.dm17)
            hipLaunchKernelGGL(k_dm_digits17, dim3(dg), dim3(BLOCK), 0, st, w.d_scalars, dp.n, dp.n_pad, w.item_sub, c->d_flags);
        else
            hipLaunchKernelGGL(k_dm_digits, dim3(dg), dim3(BLOCK), 0, st, w.d_scalars, dp.n, dp.n_pad, w.item_sub, c->d_flags);
    }
    {
        StageTimer t(c, ST_PART_SCATTER);
        const auto kpart = r.dm17 ? k_dm_partition<true> : k_dm_partition<false>;
        hipLaunchKernelGGL(kpart, dim3(dp.ntile, dm_nwin), dim3(DM_TB1), 0, st, (const uint16_t*)w.item_sub, dp, w.pcount,
                           w.tile_counts, w.item_idx);
        hipLaunchKernelGGL(k_dm_scan, dim3(1), dim3(1024), 0, st, (const uint32_t*)w.pcount, PW, w.pstart);
    }
    {
        StageTimer t(c, ST_BUCKET_SORT);
        const auto ksort = dp.n / dp.ppw <= 4096 ? k_dm_bucket_sort<16> : k_dm_bucket_sort<32>;
        hipLaunchKernelGGL(ksort, dim3(PW), dim3(DM_TB2), 0, st, (const uint32_t*)w.pstart,
                           (const uint32_t*)w.tile_counts, (const uint32_t*)w.item_idx, dp, p.NB, w.hist, w.offs, w.entries);
    }
    return H2AGG_OK;
}

// the two-level sort over (partition, sub-bucket) items: packed items staged in LDS (PACKED; PACKED_L1: level 1 staged as
// well), or index and sub-bucket in two arrays where the index does not fit the packed item (TWO_ARRAY)
int sort_packed(h2agg_ctx* c, const MsmRoute& r, const MsmWorkspace& w, hipStream_t st) {
    const MsmPlan& p = r.p;
    const SortPlan& sp = r.sp;
    const size_t n = r.n;
    {
        StageTimer t(c, ST_PART_COUNT);
        if (!w.meta_was_clean) HIP_TRY(c, hipMemsetAsync(w.meta, 0, M_WORDS * 4, st));
        hipLaunchKernelGGL(k_part_count, dim3(r.ntiles), dim3(BLOCK), 0, st, w.d_scalars, n, p.c, r.Wd, sp, w.pcount,
                           c->d_flags, w.tile_counts);
        hipLaunchKernelGGL(k_scan_small, dim3(1), dim3(BLOCK), 0, st, w.pcount, sp.PW, w.pstart, w.pcursor);
    }
    if (r.sort == SortKind::TWO_ARRAY) {
        {
            StageTimer t(c, ST_PART_SCATTER);
            hipLaunchKernelGGL(k_part_scatter, dim3(r.ntiles), dim3(BLOCK), 0, st, w.d_scalars, n, p.c, r.Wd, sp, w.pcursor,
                               w.item_idx, w.item_sub);
        }
        {
            StageTimer t(c, ST_BUCKET_SORT);
            hipLaunchKernelGGL(k_bucket_sort, dim3(sp.PW), dim3(BLOCK), 0, st, w.pstart, w.item_idx, w.item_sub, sp, p.NB,
                               w.hist, w.offs, w.entries);
        }
        return H2AGG_OK;
    }
    // LDS-staged sort: keys leave the CU as contiguous runs (n fits the packed item's index field)
    const size_t lds1 = (size_t)(4 * SORT_MAX_PW + STAGE_ITEMS_L1) * 4;
    constexpr int SORT2_TB = 1024;   // level-2 workgroup size (one workgroup per CU: see k_bucket_sort_staged)
    const size_t lds2 = (size_t)(SORT_MAX_SB + SORT2_TB + STAGE_ITEMS) * 4;
    if (!c->staged_attr_set) {
        HIP_TRY(c, hipFuncSetAttribute((const void*)k_part_scatter_staged,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1));
        HIP_TRY(c, hipFuncSetAttribute((const void*)k_bucket_sort_staged<SORT2_TB>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
        c->staged_attr_set = true;
    }
    {
        StageTimer t(c, ST_PART_SCATTER);
        if (r.sort == SortKind::PACKED_L1)
            hipLaunchKernelGGL(k_part_scatter_staged, dim3(r.ntiles), dim3(BLOCK), lds1, st, w.d_scalars, n, p.c, r.Wd,
                               sp, r.idx_bits, w.pcursor, w.item_idx);
        else
            hipLaunchKernelGGL(k_part_scatter_packed, dim3(r.ntiles), dim3(BLOCK), 0, st, w.d_scalars, n, p.c, r.Wd, sp,
                               r.idx_bits, w.pcursor, w.item_idx, (const uint32_t*)w.tile_counts);
    }
    {
        StageTimer t(c, ST_BUCKET_SORT);
        hipLaunchKernelGGL(k_bucket_sort_staged<SORT2_TB>, dim3(sp.PW), dim3(SORT2_TB), lds2, st, w.pstart, w.item_idx, sp, r.idx_bits,
                           p.NB, w.hist, w.offs, w.entries);
    }
    return H2AGG_OK;
}

int msm_sort(h2agg_ctx* c, const MsmRoute& r, const MsmWorkspace& w, hipStream_t st) {
    switch (r.sort) {
        case SortKind::SMALL: return sort_small(c, r, w, st);
        case SortKind::FB_LEVELS: return sort_fb(c, r, w, st);
        case SortKind::DIGIT_MAJOR: return sort_dm(c, r, w, st);
        default: return sort_packed(c, r, w, st);
    }
}

void msm_order(h2agg_ctx* c, const MsmRoute& r, const MsmWorkspace& w, hipStream_t st) {
    if (!r.ordered) return;
    StageTimer t(c, ST_ORDER);
    unsigned g = (r.p.NBT + BLOCK * 8 - 1) / (BLOCK * 8);
    if (g > (unsigned)launch_cap(c, 4)) g = (unsigned)launch_cap(c, 4);
    hipLaunchKernelGGL(k_size_count, dim3(g), dim3(BLOCK), 0, st, w.hist, r.p.NBT, w.bin_count);
    hipLaunchKernelGGL(k_scan_small, dim3(1), dim3(BLOCK), 0, st, w.bin_count, (uint32_t)SIZE_BINS, w.bin_start,
                       w.bin_cursor);
    hipLaunchKernelGGL(k_size_scatter, dim3(g), dim3(BLOCK), 0, st, w.hist, r.p.NBT, w.bin_cursor, w.order);
}

// the bucket accumulation on `st`, behind the bases hook (h2agg_ctx::bases_hook) where the caller set one
int msm_accumulate(h2agg_ctx* c, const MsmRoute& r, MsmWorkspace& w, hipStream_t st) {
    const MsmKnobs& K = msm_knobs();
    const MsmPlan& p = r.p;
    const uint32_t lpb = r.lpb;
    if (c->bases_hook) {
        TRY(c->bases_hook(st));
        if (r.endo_here) launch_bases_endo_x(c, r, w, st);
    }
    if (lpb > 1) {
        TRY(ensure(c, c->parts, (size_t)p.NBT * lpb * XYZZ_BYTES));
        w.acc_out = (uint8_t*)c->parts.p;
    }
    if (r.lean) {
        TRY(ensure(c, c->fix_list[w.sq], (size_t)p.NBT * lpb * 8));
        w.fix_list = (uint32_t*)c->fix_list[w.sq].p;
    }
    debug_sync(2);
    chaos_wait(2, st);
    StageTimer t(c, ST_ACCUM, st);
    const uint32_t* order = r.ordered ? w.order : (uint32_t*)nullptr;
    // one-wave workgroups: a 4-wave workgroup needs a free slot on all four SIMDs of a CU at once and its waves retire
    // at different times; single waves fill any slot as it frees up (2^20 points: 1.74 -> 1.67 ms/step)
    if (r.lean) {   // 128 VGPRs, four waves per SIMD; exceptional cases go to fix_list (msm_kernels.hpp)
#ifdef H2AGG_MEASURE_KNOBS
        auto kacc = r.lean_dual ? acc_lean_kernel<true>(r.chain, r.lean_var) : acc_lean_kernel<false>(r.chain, r.lean_var);
#else
        auto kacc = acc_lean_kernel<true>(r.chain, r.lean_var);
#endif
        c->last_lean_variant = r.lean_var;
        hipLaunchKernelGGL(kacc, dim3((unsigned)(((size_t)p.NBT * lpb + 63) / 64)), dim3(64), (size_t)K.acc_lds,
                           st, w.d_bases, w.d_endo_x, w.entries, w.offs, w.hist, order, p.NBT, p.big, lpb, w.acc_out,
                           w.big_list, w.big_keys, w.big_count, w.fix_list);
    } else {
#ifdef H2AGG_MEASURE_KNOBS
        auto kacc = r.chain == CHAIN_FIRST ? k_msm_accumulate<1> : (r.chain == CHAIN_MID || r.chain == CHAIN_LAST) ? k_msm_accumulate<2> : k_msm_accumulate<0>;
        hipLaunchKernelGGL(kacc, dim3((unsigned)(((size_t)p.NBT * lpb + K.acc_block - 1) / K.acc_block)), dim3(K.acc_block), (size_t)K.acc_lds,
                           st, w.d_bases, w.d_endo_x, w.entries, w.offs, w.hist, order, p.NBT, p.big, lpb, w.acc_out,
                           w.big_list, w.big_keys, w.big_count);
#endif
    }
    return H2AGG_OK;
}

// folds the lpb slice slots of every bucket into the bucket set
void launch_bucket_combine(const MsmRoute& r, const MsmWorkspace& w, hipStream_t bs) {
    const MsmPlan& p = r.p;
    const uint32_t lpb = r.lpb, cbig = r.chain ? 0xffffffffu : p.big;
    if (p.NBT > 16384u || (lpb != 2 && lpb != 4 && lpb != 8)) {   // many buckets: one lane each (work, not latency)
        hipLaunchKernelGGL(k_msm_bucket_combine, dim3((p.NBT + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, bs,
                           (const uint8_t*)w.acc_out, w.hist, p.NBT, cbig, lpb, w.buckets);
        return;
    }
    const unsigned gq = (unsigned)(((size_t)p.NBT * 2 * lpb + BLOCK - 1) / BLOCK);
    const auto kcomb = lpb == 8 ? k_msm_bucket_combine_par4<8> : lpb == 4 ? k_msm_bucket_combine_par4<4> : k_msm_bucket_combine_par4<2>;
    hipLaunchKernelGGL(kcomb, dim3(gq), dim3(BLOCK), 0, bs, (const uint8_t*)w.acc_out, w.hist, p.NBT, cbig, w.buckets);
}

// what the accumulation left aside: the lean kernel's fix list, buckets longer than `big`, the slice slots' combine.  On the
// accumulation's stream, or (MsmRoute::tail_big) at the head of the tail.
void msm_big_kernels(h2agg_ctx* c, const MsmRoute& r, const MsmWorkspace& w, hipStream_t bs) {
    const MsmPlan& p = r.p;
    const uint32_t lpb = r.lpb;
    const uint32_t resume = (r.chain == CHAIN_MID || r.chain == CHAIN_LAST) ? 1u : 0u;
    const bool chain_open = r.chain == CHAIN_FIRST || r.chain == CHAIN_MID;   // no tail yet
    StageTimer t(c, ST_ACCUM_BIG, bs);
    if (r.lean)   // (grid-stride over a list that is empty but for the one-limb filter's false positives and adversarial inputs)
        hipLaunchKernelGGL(k_msm_accumulate_fix, dim3((unsigned)std::min<size_t>(launch_cap(c, 12), ((size_t)p.NBT * lpb + 63) / 64)), dim3(64), 0, bs, w.d_bases, w.d_endo_x, w.entries, w.offs,
                           w.hist, lpb, w.acc_out, (const uint32_t*)w.big_count, (const uint32_t*)w.fix_list);
    if (!r.big_possible && lpb == 1) return;
    size_t grid = r.max_slots;
    const size_t cap = launch_cap(c, 8);   // one-wave workgroups, grid-stride over the (usually empty) lists
    if (grid > cap) grid = cap;
    hipLaunchKernelGGL(k_msm_accumulate_big, dim3((unsigned)grid), dim3(64), 0, bs, w.d_bases, w.d_endo_x, w.entries, w.offs, w.hist,
                       w.acc_out, lpb, w.big_part, w.big_list, w.big_count, resume);
    size_t gk = r.max_keys < cap ? r.max_keys : cap;
    hipLaunchKernelGGL(k_msm_big_combine, dim3((unsigned)gk), dim3(64), 0, bs, w.big_part, w.big_keys, w.big_count,
                       w.acc_out, lpb, resume);
    // (in a chain only the last slice folds the slice slots, and it folds ALL of them: a bucket that is over-long in this
    // slice may hold ordinary partial sums from earlier ones)
    if (lpb > 1 && !chain_open) launch_bucket_combine(r, w, bs);
}

// arrival counters of the two half-window workgroups of the two-dimensional reduction: zero between MSMs
int msm_tail_tickets(h2agg_ctx* c, const MsmRoute& r, MsmWorkspace& w) {
    if (r.tail == TailKind::SEGMENTS) return H2AGG_OK;
    DevBuf& tk = c->r2d_ticket[w.par];
    const size_t tickets = r.tail == TailKind::FB_GRIDS ? (size_t)FB_R2D_WINDOWS : (size_t)r.WT;
    if (tickets * 4 > tk.cap) {
        TRY(ensure(c, tk, tickets * 4));
        HIP_TRY(c, hipMemset(tk.p, 0, tk.cap));
    }
    w.ticket = (uint32_t*)tk.p;
    return H2AGG_OK;
}

// where the fixed-base tail keeps its records behind the grids' partial sums (segsum) and window sums (wsum)
struct FbTailBufs {
    uint8_t *halves, *tsum, *w2;
};
FbTailBufs fb_tail_bufs(const MsmWorkspace& w) {
    constexpr uint32_t total = FB_R2D_WINDOWS * (uint32_t)R2D<7>::THREADS;
    FbTailBufs b;
    b.halves = w.segsum + XYZZ_BYTES * (size_t)total;
    b.tsum = b.halves + XYZZ_BYTES * (size_t)(2 * FB_R2D_WINDOWS);
    b.w2 = w.wsum + XYZZ_BYTES * (size_t)FB_R2D_WINDOWS;
    return b;
}

// one set of 2^19 buckets as 16 grids of 256 x 128 (msm_kernels.hpp, above k_fb_fold)
void tail_fb(h2agg_ctx* c, const MsmWorkspace& w, hipStream_t ts) {
    constexpr uint32_t total = FB_R2D_WINDOWS * (uint32_t)R2D<7>::THREADS;
    const FbTailBufs fb = fb_tail_bufs(w);
    {
        StageTimer t(c, ST_REDUCE, ts);
        hipLaunchKernelGGL(k_fb_fold, dim3((FB_XB >> FB_XPARTS_LOG) / 64), dim3(64), 0, ts, w.buckets);
        hipLaunchKernelGGL(k_msm_reduce2d_parts<7>, dim3(total / 64), dim3(64), 0, ts, (const uint8_t*)w.buckets, total, w.segsum);
    }
    {
        StageTimer t(c, ST_WINDOW_SUM, ts);
        hipLaunchKernelGGL(k_msm_reduce2d_window<7>, dim3(FB_R2D_WINDOWS, 2), dim3(R2D_TB), 0, ts, (const uint8_t*)w.segsum, fb.halves, w.ticket,
                           w.wsum, fb.tsum);
    }
}

// the two-dimensional bucket reduction of 16-bit (LC = 7) and 17-bit (LC = 8) windows
template <int LC>
void tail_r2d(h2agg_ctx* c, const MsmRoute& r, const MsmWorkspace& w, hipStream_t ts) {
    const int dbg_skip = msm_knobs().dbg_skip;
    const uint32_t per_w = (uint32_t)R2D<LC>::THREADS;
    if (!(dbg_skip & 1)) {
        StageTimer t(c, ST_REDUCE, ts);
        const uint32_t total = r.WT * per_w;
        hipLaunchKernelGGL(k_msm_reduce2d_parts<LC>, dim3(total / 64), dim3(64), 0, ts, (const uint8_t*)w.buckets, total, w.segsum);
    }
    if (!(dbg_skip & 2)) {
        StageTimer t(c, ST_WINDOW_SUM, ts);
        hipLaunchKernelGGL(k_msm_reduce2d_window<LC>, dim3(r.WT, 2), dim3(R2D_TB), 0, ts, (const uint8_t*)w.segsum,
                           w.segsum + XYZZ_BYTES * (size_t)r.WT * per_w, w.ticket, w.wsum);
    }
}

void tail_segments(h2agg_ctx* c, const MsmRoute& r, const MsmWorkspace& w, hipStream_t ts) {
    const int dbg_skip = msm_knobs().dbg_skip;
    const MsmPlan& p = r.p;
    if (!(dbg_skip & 1)) {
        StageTimer t(c, ST_REDUCE, ts);
        if (r.par4)
            hipLaunchKernelGGL(k_msm_reduce_segments_par4, dim3((4 * r.nseg_total + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, ts,
                               w.buckets, p.NB, p.seg, p.spw, r.nseg_total, w.segsum);
        else
            hipLaunchKernelGGL(k_msm_reduce_segments, dim3((r.nseg_total + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, ts, w.buckets,
                               p.NB, p.seg, p.spw, r.nseg_total, w.segsum);
    }
    if (!(dbg_skip & 2)) {
        StageTimer t(c, ST_WINDOW_SUM, ts);
        if (r.par4)
            hipLaunchKernelGGL(k_msm_window_sum_par4, dim3(r.WT), dim3(PAR4_THREADS), 0, ts, w.segsum, p.spw, w.wsum);
        else
            hipLaunchKernelGGL(k_msm_window_sum, dim3(r.WT), dim3(BLOCK), 0, ts, w.segsum, p.spw, w.wsum);
    }
}

// The last chain of every tail: the window sums' Horner chain (fixed-base levels: the sum of the grids' sums).  `from`: the
// stream the accumulation ran on; ts: the stream the tail is on so far.
int tail_final(h2agg_ctx* c, const MsmRoute& r, const MsmWorkspace& w, hipStream_t from, hipStream_t ts) {
    const MsmKnobs& K = msm_knobs();
    const int par = w.par;
    if (r.final_off_stream && !r.tails_off_stream) {   // overlap level 1: only the last chain (the Horner tail) leaves the stream
        HIP_TRY(c, hipEventRecord(c->ev_bulk[par], from));
        HIP_TRY(c, hipStreamWaitEvent(c->tail_streams[par], c->ev_bulk[par], 0));
        ts = c->tail_streams[par];
    }
    if (r.tail == TailKind::FB_GRIDS) {
        const FbTailBufs fb = fb_tail_bufs(w);
        StageTimer t(c, ST_FINAL, ts);
        hipLaunchKernelGGL(k_fb_wsum, dim3(1), dim3(64), 0, ts, (const uint8_t*)w.wsum, (const uint8_t*)fb.tsum, fb.w2);
        hipLaunchKernelGGL(k_msm_final_lp, dim3(1), dim3(64), 0, ts, (const uint8_t*)fb.w2, 15, 2, w.res_xyzz, w.d_out_jac);
    } else if (!(K.dbg_skip & 4)) {
        StageTimer t(c, ST_FINAL, ts);
        uint8_t* const xyzz = (r.batch > 1 && !r.split) ? (uint8_t*)nullptr : w.res_xyzz;
        // the Horner chain in the limb-parallel form (lp_kernels.hpp): 1.2 instead of 2.0 us per doubling
        if (K.final_par4)
            hipLaunchKernelGGL(k_msm_final, dim3(r.batch), dim3(64), 0, ts, w.wsum, r.p.c, r.W1, xyzz, w.d_out_jac);
        else
            hipLaunchKernelGGL(k_msm_final_lp, dim3(r.batch), dim3(64), 0, ts, w.wsum, r.p.c, r.W1, xyzz, w.d_out_jac);
    }
    if (r.final_off_stream) {
        HIP_TRY(c, hipEventRecord(c->ev_tail[par], c->tail_streams[par]));
        c->tail_pending[par] = true;
    }
    return H2AGG_OK;
}

// The tail of one MSM, at once or (deferred) from a later call.  `from`: the stream the accumulation ran on (which recorded
// ev_bulk[par] behind it when the tail leaves it).  behind_sort: the tail stream also waits for c->ev_sortdone.
int msm_tail(h2agg_ctx* c, const MsmRoute& r, const MsmWorkspace& w, hipStream_t from, bool behind_sort) {
    hipStream_t ts = from;
    if (r.tails_off_stream) {
        ts = c->tail_streams[w.par];
        HIP_TRY(c, hipStreamWaitEvent(ts, c->ev_bulk[w.par], 0));
        if (behind_sort) HIP_TRY(c, hipStreamWaitEvent(ts, c->ev_sortdone, 0));
    }
    chaos_wait(1, ts);
    if (r.tail_big) {
        msm_big_kernels(c, r, w, ts);
        HIP_TRY(c, hipMemsetAsync(w.meta, 0, M_WORDS * 4, ts));
        c->meta_clean[w.sq] = true;
        HIP_TRY(c, hipEventRecord(c->ev_accdone[w.sq], ts));
        c->accdone_pending[w.sq] = true;
    }
    switch (r.tail) {
        case TailKind::FB_GRIDS: tail_fb(c, w, ts); break;
        case TailKind::R2D7: tail_r2d<7>(c, r, w, ts); break;
        case TailKind::R2D8: tail_r2d<8>(c, r, w, ts); break;
        case TailKind::SEGMENTS: tail_segments(c, r, w, ts); break;
    }
    return tail_final(c, r, w, from, ts);
}

// launches a deferred tail (h2agg_ctx::deferred_job).  The job is copied out and the flag cleared BEFORE it runs: this is
// re-entered from ensure() inside the next call's msm_bind, and from whatever the tail itself calls.
int flush_deferred_tail(h2agg_ctx* c, bool behind_sort) {
    if (!c->tail_deferred) return H2AGG_OK;
    const MsmTailJob job = c->deferred_job;
    c->tail_deferred = false;
    return msm_tail(c, job.r, job.w, job.from, behind_sort);
}

// make everything queued on the tail stream visible to the main stream
int join_tails(h2agg_ctx* c) {
    TRY(flush_deferred_tail(c, false));
    for (int k = 0; k < h2agg_ctx::TAIL_SLOTS; ++k) {
        if (c->tail_pending[k]) {
            HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_tail[k], 0));
            c->tail_pending[k] = false;
        }
    }
    for (int q = 0; q < 2; ++q) {   // (every accumulation is followed by a tail, so these have completed: bookkeeping)
        if (c->accdone_pending[q]) {
            HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_accdone[q], 0));
            c->accdone_pending[q] = false;
        }
    }
    return H2AGG_OK;
}

// ---- the MSM proper ---------------------------------------------------------------------------------------------------------
// call.d_bases: Montgomery affine table; call.d_scalars: canonical 32-B scalars (device).
// Result: c->d_res_xyzz (Montgomery XYZZ) and, if d_out_jac != nullptr, canonical Jacobian there.
// batch > 1: `batch` MSMs over the SAME n bases, scalars laid out [batch][n]; results: canonical Jacobian at
// d_out_jac[96 * q] (c->d_res_xyzz then only holds MSM 0's XYZZ).  One set of launches does all of them: every
// scalar's windows are numbered q * W + w, and the stages after the sort only see batch * W windows.
// d_endo_x: beta * x per base (Table::endo_x) or nullptr = compute it here when the plan uses GLV.
// pre: fixed-base levels of the table (then d_bases is ignored): plain c-bit digits of ALL positions into one bucket set
// per MSM, bases looked up at level w; no Horner chain.
// split != 0: TWO MSMs over the disjoint parts [0, split) and [split, n_base) of one table (scalars laid out alike), as one
// set of launches with 2 W windows; results: XYZZ at c->d_res_xyzz and c->d_res_xyzz + XYZZ_BYTES.  Only for sizes the
// one-launch sort takes (msm_split_ok): the evaluation's two multi_exps.  When the route's plan uses GLV, d_scalars are
// glv_decompose() words and d_endo_x is given (k_eval_prep wrote both).
// no_identity: the table d_bases points into is known to hold no identity base (Table::no_identity)
// chain: slices of ONE MSM that share a bucket set (MsmCall).
int msm_run(h2agg_ctx* c, const MsmCall& call) {
    const MsmRoute r = msm_route(c, call);
    crumb((uintptr_t)__builtin_return_address(0), ((uint64_t)r.batch << 40) | call.n_base);
    if (r.refuse_code != H2AGG_OK) return fail(c, r.refuse_code, r.refuse_msg);
    MsmWorkspace w;
    TRY(msm_bind(c, call, r, w));
    const int sq = w.sq, par = w.par;
    profile_begin_call(c);
    // the accumulation that last read this slot's sort outputs (two MSMs ago, or any earlier one for an MSM that does not
    // leave the stream: it uses slot 0 and scratch the accumulation stream may still read — beta*x column, slice sums)
    for (int q = 0; q < 2; ++q) {
        if (c->accdone_pending[q] && (!r.altbuf || q == sq || r.endo_here)) {
            HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_accdone[q], 0));
            c->accdone_pending[q] = false;
        }
    }
    hipStream_t st = c->stream;
    TRY(msm_glv_prepare(c, r, w, st));
    TRY(msm_sort(c, r, w, st));
    msm_order(c, r, w, st);
    if (c->tail_deferred) {   // the previous MSM's tail goes out now, behind this MSM's sort — beside the sort it slows the
                              // sort's latency chains by 2x, beside the accumulation it only costs its own instructions
        HIP_TRY(c, hipEventRecord(c->ev_sortdone, st));
        TRY(flush_deferred_tail(c, true));
    }
    if (r.piped) {   // from here on: the accumulation stream
        HIP_TRY(c, hipEventRecord(c->ev_sorted[sq], st));
        HIP_TRY(c, hipStreamWaitEvent(c->acc_stream, c->ev_sorted[sq], 0));
        st = c->acc_stream;
    }
    if (c->tail_pending[par]) {  // the tail TAIL_SLOTS MSMs ago read this slot's buckets / segsum / wsum
        HIP_TRY(c, hipStreamWaitEvent(st, c->ev_tail[par], 0));
        c->tail_pending[par] = false;
    }
    TRY(msm_accumulate(c, r, w, st));
    if (!r.tail_big) {
        msm_big_kernels(c, r, w, st);
        if (r.altbuf) {
            HIP_TRY(c, hipEventRecord(c->ev_accdone[sq], st));
            c->accdone_pending[sq] = true;
        }
    }
    if (r.altbuf) c->sort_par ^= 1;
    if (r.chain == CHAIN_FIRST || r.chain == CHAIN_MID) {   // the bucket set stays open for the next slice: no tail, the slot does not rotate
        HIP_TRY(c, hipGetLastError());
        profile_end_call(c);
        return H2AGG_OK;
    }
    TRY(msm_tail_tickets(c, r, w));
    debug_sync(4);
    if (r.tails_off_stream) HIP_TRY(c, hipEventRecord(c->ev_bulk[par], st));
    if (r.defer) {   // whoever needs the results first (join_tails), or the next MSM behind its sort, launches it
        c->deferred_job = MsmTailJob{r, w, st};
        c->tail_deferred = true;
    } else {
        TRY(msm_tail(c, r, w, st, false));
    }
    // the slot (buckets / segsum / wsum / XYZZ result) rotates on every MSM, overlap or not: a caller may queue
    // two MSMs and read both results afterwards (evaluate_multiopen_proof does)
    c->parity = (c->parity + 1) % h2agg_ctx::TAIL_SLOTS;
    debug_sync(8);
    HIP_TRY(c, hipGetLastError());
    profile_end_call(c);
    return H2AGG_OK;
}
