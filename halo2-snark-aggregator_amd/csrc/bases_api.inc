// Base tables (included into h2agg.hip behind chips_api.inc: shares the context internals; kernels in batch_kernels.hpp and
// scalar_mul_kernels.hpp): h2agg_bases_upload / _generate / _download / _free / _precompute, the generator's comb behind
// h2agg_bases_generate and h2agg_params_setup, and what an MSM over a resident table asks of it: its beta * x column and the
// comb of its leading bases.

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

// beta * x column of a resident table, made once
int table_endo(h2agg_ctx* c, Table& t, const uint8_t** out) {
    if (!t.endo_x) {
        TRY(dev_alloc(c, t.endo_x, 32 * t.n, "endo table"));
        hipLaunchKernelGGL(k_bases_endo_x, dim3(grid_for(c, t.n)), dim3(BLOCK), 0, c->stream, (const uint8_t*)t.d, t.n,
                           t.endo_x);
    }
    *out = t.endo_x;
    return H2AGG_OK;
}

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
        DevMem fresh;
        if (fresh.alloc(entries * 64) != hipSuccess) {
            *done = false;
            return H2AGG_OK;
        }
        if (t.comb) t.comb_retired.push_back(std::move(t.comb));
        t.comb = std::move(fresh);
        size_t grid = (entries + SM_GROUPS - 1) / SM_GROUPS;
        const size_t cap = launch_cap(c, 16);
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

// A table of n points whose column is allocated and nothing else: what every creating call fills.  A call that returns
// before table_register leaves it to its destructor, whose hipFree waits for whatever the call had queued.
int table_new(h2agg_ctx* c, size_t n, Table* t) {
    t->n = n;
    return dev_alloc(c, t->d, 64 * n, "base table");
}

// The finished table of a creating call, behind that call's finish(): into the context, under a new handle.  The word
// finish() read says whether the call stored an identity base.
uint64_t table_register(h2agg_ctx* c, Table&& t) {
    t.no_identity = table_word_clear(c->table_word);
    const uint64_t h = c->next_handle++;
    c->tables.emplace(h, std::move(t));
    return h;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- base tables
int h2agg_bases_upload(h2agg_ctx* c, const uint8_t* bases, size_t n, uint64_t* handle_out) try {
    TRY(bind(c));
    if (!bases || !handle_out || n == 0) return fail(c, H2AGG_ERR_INVALID, "null buffer or n == 0");
    Table t;
    TRY(table_new(c, n, &t));
    TRY(ensure(c, c->tmp_bases, 64 * n));
    TRY(stage_in(c, c->tmp_bases, bases, 64 * n));
    TRY(clear_flags(c));
    hipLaunchKernelGGL(k_bases_to_mont, dim3(grid_for(c, n)), dim3(BLOCK), 0, c->stream,
                       (const uint8_t*)c->tmp_bases.p, n, t.d, c->d_flags);
    TRY(finish(c));
    *handle_out = table_register(c, std::move(t));
    return H2AGG_OK;
} API_CATCH

int h2agg_bases_generate(h2agg_ctx* c, const void* d_k, size_t n, uint64_t* handle_out) try {
    TRY(bind(c));
    if (!d_k || !handle_out || n == 0) return fail(c, H2AGG_ERR_INVALID, "null buffer or n == 0");
    Table t;
    TRY(table_new(c, n, &t));
    TRY(clear_flags(c));
    static const bool ladder = knob("H2AGG_SCALAR_MUL") && !strcmp(knob("H2AGG_SCALAR_MUL"), "ladder");
    if (ladder) {
        size_t blocks = (n + BLOCK - 1) / BLOCK;
        if (blocks > 65535 * 16) blocks = 65535 * 16;
        hipLaunchKernelGGL(k_bases_generate, dim3((unsigned)blocks), dim3(BLOCK), 0, c->stream, (const uint8_t*)d_k, n, t.d,
                           c->d_flags);
    } else {
        TRY(comb_generate_launch(c, (const uint8_t*)d_k, n, t.d));
    }
    TRY(finish(c));
    *handle_out = table_register(c, std::move(t));
    return H2AGG_OK;
} API_CATCH

int h2agg_bases_download(h2agg_ctx* c, uint64_t handle, size_t first, size_t n, uint8_t* out) try {
    TRY(bind(c));
    Table* t = nullptr;
    TRY(find_table(c, handle, &t));
    if (!out || first + n > t->n) return fail(c, H2AGG_ERR_INVALID, "range outside the table");
    if (n == 0) return H2AGG_OK;
    TRY(ensure(c, c->out, 64 * n));
    hipLaunchKernelGGL(k_bases_from_mont, dim3(grid_for(c, n)), dim3(BLOCK), 0, c->stream, t->d + 64 * first,
                       n, (uint8_t*)c->out.p);
    HIP_TRY(c, hipMemcpyAsync(out, c->out.p, 64 * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return H2AGG_OK;
} API_CATCH

int h2agg_bases_free(h2agg_ctx* c, uint64_t handle) try {
    TRY(bind(c));
    Table* t = nullptr;
    TRY(find_table(c, handle, &t));
    TRY(join_tails(c));   // tails and accumulations on the context's other streams (and a deferred tail) may still read the table
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->tables.erase(handle);
    return H2AGG_OK;
} API_CATCH

int h2agg_bases_precompute(h2agg_ctx* c, uint64_t handle, int window_bits) try {
    TRY(bind(c));
    Table* tp = nullptr;
    TRY(find_table(c, handle, &tp));
    Table& t = *tp;
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
    t.pre.reset();
    t.free_combs();
    TRY(dev_alloc(c, t.pre, (size_t)W * t.n * 64, "fixed-base levels"));
    HIP_TRY(c, hipMemcpyAsync(t.pre, t.d, t.n * 64, hipMemcpyDeviceToDevice, c->stream));
    for (int w = 1; w < W; ++w)
        hipLaunchKernelGGL(k_bases_shift, dim3(grid_for(c, t.n)), dim3(BLOCK), 0, c->stream,
                           (const uint8_t*)t.pre + (size_t)(w - 1) * t.n * 64, t.n, cc, t.pre + (size_t)w * t.n * 64);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    t.pre_c = cc;
    t.pre_W = W;
    return H2AGG_OK;
} API_CATCH

}  // extern "C"
