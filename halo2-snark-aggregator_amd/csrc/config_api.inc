// Tuning, test hooks and measurement (included into h2agg.hip behind msm_api.inc: shares the context internals):
// h2agg_msm_configure*, h2agg_debug_configure and its key table, h2agg_debug_lean_variant / _table_identity,
// h2agg_msm_set_tail_overlap, h2agg_profile_*.

namespace {

// h2agg_debug_configure's keys: the member of the context a key sets (h2agg_ctx's dbg_ block has the defaults and meanings,
// include/h2agg.h "Test hooks" the documentation; tests/test_gpu_debug_keys.py holds the three together) and the values it takes.
struct DebugKey {
    const char* name;
    int h2agg_ctx::*field;
    int lo = 1, hi = 0;     // the accepted values, lo .. hi (hi = INT_MAX: no upper end); lo > hi: any int
    bool zero_ok = false;   // ... and 0, which stands for the default
};
const DebugKey DEBUG_KEYS[] = {
    {"pcie_slices", &h2agg_ctx::dbg_pcie_slices},
    {"pcie_glv", &h2agg_ctx::dbg_pcie_glv},
    {"pcie_chain", &h2agg_ctx::dbg_pcie_chain},
    {"comb_msm", &h2agg_ctx::dbg_comb_msm},
    {"plan_cache", &h2agg_ctx::dbg_plan_cache},
    {"small_sort", &h2agg_ctx::dbg_small_sort},
    {"eval_split", &h2agg_ctx::dbg_eval_split},
    {"lean_acc", &h2agg_ctx::dbg_lean_acc},   // (the product build takes 1 only: h2agg_debug_configure)
    {"lean_full", &h2agg_ctx::dbg_lean_full},
    {"pre_big", &h2agg_ctx::dbg_pre_big},
    {"tape_lds", &h2agg_ctx::dbg_tape_lds},   // (a change drops the kept recordings: h2agg_debug_configure)
    {"prewake", &h2agg_ctx::dbg_prewake},
    {"phases", &h2agg_ctx::dbg_phases},
    {"shard_fail", &h2agg_ctx::dbg_shard_fail},
    {"seg_chunk", &h2agg_ctx::dbg_seg_chunk},
    {"seg_c", &h2agg_ctx::dbg_seg_c, 4, 8, true},
    {"fr_fft_local", &h2agg_ctx::dbg_fr_fft_local, 1, (int)FR_FFT_TILE_LOG, true},
    {"fr_fft_batch_chunk", &h2agg_ctx::dbg_fr_fft_batch_chunk, 0, INT_MAX},
    {"fr_poly_chunk", &h2agg_ctx::dbg_fr_poly_chunk, (int)FR_CHUNK_PER_LOG, (int)FR_CHUNK_LOG, true},
    {"fr_scan_chunk", &h2agg_ctx::dbg_fr_scan_chunk, (int)FR_CHUNK_PER_LOG, (int)FR_CHUNK_LOG, true},
    {"fr_sort_tile", &h2agg_ctx::dbg_fr_sort_tile, (int)LK_TILE_LOG_MIN, (int)LK_TILE_LOG, true},
    {"commit_chunk", &h2agg_ctx::dbg_commit_chunk, 0, INT_MAX},
    {"launch_cus", &h2agg_ctx::dbg_launch_cus, 1, 1024, true},
};

bool debug_key_takes(const DebugKey& k, int value) {
    return k.lo > k.hi || (k.zero_ok && value == 0) || (value >= k.lo && value <= k.hi);
}
// "<key> must be 0 or 3 .. 11", "<key> must be >= 0"
std::string debug_key_range(const DebugKey& k) {
    std::string s = std::string("h2agg_debug_configure: ") + k.name + " must be ";
    if (k.zero_ok) s += "0 or ";
    return s + (k.hi == INT_MAX ? ">= " + std::to_string(k.lo) : std::to_string(k.lo) + " .. " + std::to_string(k.hi));
}

}  // namespace

extern "C" {

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
} API_CATCH

int h2agg_msm_configure_glv(h2agg_ctx* c, int mode) try {
    if (!c) return H2AGG_ERR_INVALID;
    if (mode < -1 || mode > 1) return fail(c, H2AGG_ERR_INVALID, "mode must be -1 (off), 0 (auto) or 1 (on)");
    c->cfg_glv = mode;
    return H2AGG_OK;
} API_CATCH
int h2agg_msm_configure_lanes_per_bucket(h2agg_ctx* c, int lanes) try {
    if (!c) return H2AGG_ERR_INVALID;
    if (lanes != 0 && lanes != 1 && lanes != 2 && lanes != 4 && lanes != 8 && lanes != 16)
        return fail(c, H2AGG_ERR_INVALID, "lanes must be 0, 1, 2, 4, 8 or 16");
    c->cfg_lpb = lanes;
    return H2AGG_OK;
} API_CATCH

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
} API_CATCH

int h2agg_debug_configure(h2agg_ctx* c, const char* key, int value) try {
    if (!c || !key) return H2AGG_ERR_INVALID;
    const std::string k(key);
    const DebugKey* row = nullptr;
    for (const DebugKey& r : DEBUG_KEYS)
        if (k == r.name) row = &r;
    if (!row) return fail(c, H2AGG_ERR_INVALID, "h2agg_debug_configure: unknown key " + k);
    if (!debug_key_takes(*row, value)) return fail(c, H2AGG_ERR_INVALID, debug_key_range(*row));
#ifndef H2AGG_MEASURE_KNOBS
    if (k == "lean_acc" && value != 1)
        return fail(c, H2AGG_ERR_INVALID, "h2agg_debug_configure: the generic accumulation kernel is in the measure build only (build_ext.py --measure)");
#endif
    if (k == "tape_lds" && c->dbg_tape_lds != value) agg_plans_release(c);   // (kept recordings carry their tape in one encoding or the other)
    c->*(row->field) = value;
    return H2AGG_OK;
} API_CATCH

int h2agg_debug_lean_variant(int table_no_identity, int plan_glv) {
    return msm_lean_variant(table_no_identity != 0, plan_glv != 0);
}

int h2agg_debug_table_identity(h2agg_ctx* c, uint64_t handle, int* may_hold_out, int* last_variant_out) try {
    TRY(bind(c));
    if (may_hold_out) {
        Table* t = nullptr;
        TRY(find_table(c, handle, &t));
        *may_hold_out = t->no_identity ? 0 : 1;
    }
    if (last_variant_out) *last_variant_out = c->last_lean_variant;
    return H2AGG_OK;
} API_CATCH

int h2agg_msm_set_tail_overlap(h2agg_ctx* c, int enable) try {
    TRY(bind(c));
    TRY(join_tails(c));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->tail_overlap = enable != 0;
    if (enable >= 1 && enable <= 3) c->overlap_level = enable;
    return H2AGG_OK;
} API_CATCH

int h2agg_profile_enable(h2agg_ctx* c, int enable) try {
    TRY(bind(c));
    if (enable && !c->prof_events_created) {
        for (int r = 0; r < h2agg_ctx::PROF_RING; ++r)
            for (int s = 0; s < ST_N; ++s)
                for (int k = 0; k < 2; ++k) HIP_TRY(c, c->prof[r].ev[s][k].create(EV_TIME_FLAGS));
        c->prof_events_created = true;
    }
    if (!enable) profile_harvest_all(c);
    c->profiling = enable != 0;
    c->prof_only = (enable >= 2 && enable - 2 < ST_N) ? enable - 2 : -1;
    return H2AGG_OK;
} API_CATCH
int h2agg_profile_reset(h2agg_ctx* c) try {
    if (!c) return H2AGG_ERR_INVALID;
    profile_harvest_all(c);
    for (int s = 0; s < ST_N; ++s) {
        c->stage_ms[s] = 0;
        c->stage_launches[s] = 0;
    }
    return H2AGG_OK;
} API_CATCH
int h2agg_profile_stage_count(h2agg_ctx*) { return ST_N; }
const char* h2agg_profile_stage_name(h2agg_ctx*, int i) { return (i >= 0 && i < ST_N) ? STAGE_NAMES[i] : ""; }
int h2agg_profile_stage_get(h2agg_ctx* c, int i, double* total_ms, uint64_t* launches) try {
    if (!c || i < 0 || i >= ST_N) return H2AGG_ERR_INVALID;
    profile_harvest_all(c);
    if (total_ms) *total_ms = c->stage_ms[i];
    if (launches) *launches = c->stage_launches[i];
    return H2AGG_OK;
} API_CATCH

}  // extern "C"
