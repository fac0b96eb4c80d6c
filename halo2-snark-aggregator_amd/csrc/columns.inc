// Fr column stores, host side (included into h2agg.hip behind witness.inc: shares the context internals and every family's
// queue functions; the two kernels in columns_kernels.hpp, checks in fr_host.inc, staging and allocation in host.inc):
// h2agg_columns_create / _destroy / _info / _write / _read / _ptr / _move, and the resident forms of the families that take
// whole slabs — h2agg_columns_fft, _commit, _sigmas, _witness_check, _shplonk_begin, and of the lookup batches (lookup.inc) —
// h2agg_lookup_store_permute, h2agg_lookup_store_product.  A store is a slab [m][2^k] of canonical
// Fr in device memory that the context owns behind a handle, as it owns a base table (DESIGN.md 5.20); the yardstick is the
// definition in include/h2agg.h: a resident form answers byte for byte what its host-buffer family answers.
//
// Every resident form is a front over the function its family already runs behind its staging: fr_fft_queue_batch,
// commit_columns_run, perm_sigma_queue, wc_check / wc_queue / wc_report_out, shplonk_begin, lk_batch_permute_queue /
// lk_batch_product_queue.  Nothing here computes.

namespace {

int find_store(h2agg_ctx* c, uint64_t handle, ColumnStore** out) {
    auto it = c->stores.find(handle);
    if (it == c->stores.end()) return fail(c, H2AGG_ERR_INVALID, "unknown column-store handle");
    *out = &it->second;
    return H2AGG_OK;
}

// columns [first, first + count) of the store, count >= 1 -> the device address of the first
int store_range(h2agg_ctx* c, uint64_t handle, size_t first, size_t count, ColumnStore** st, uint8_t** d_first) {
    TRY(find_store(c, handle, st));
    if (count == 0 || first > (*st)->m || count > (*st)->m - first)
        return fail(c, H2AGG_ERR_INVALID, "column range outside the store (or count == 0)");
    *d_first = (*st)->d + (*st)->col() * first;
    return H2AGG_OK;
}

// a slab of a key's columns from a store, or null where the key has none of the kind (the handle is then not looked at)
int store_slab_of_key(h2agg_ctx* c, uint64_t handle, size_t first, size_t count, unsigned k, const uint8_t** d) {
    *d = nullptr;
    if (count == 0) return H2AGG_OK;
    ColumnStore* st = nullptr;
    uint8_t* p = nullptr;
    TRY(store_range(c, handle, first, count, &st, &p));
    if (st->k != k) return fail(c, H2AGG_ERR_INVALID, "the store's k is not the key's");
    *d = p;
    return H2AGG_OK;
}

bool ranges_meet(size_t a, size_t b, size_t count) { return a < b + count && b < a + count; }

}  // namespace

extern "C" {

int h2agg_columns_create(h2agg_ctx* c, size_t m, unsigned k, uint64_t* handle_out) try {
    TRY(bind(c));
    if (!handle_out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    if (m == 0) return fail(c, H2AGG_ERR_INVALID, "columns_create: m == 0");
    TRY(fr_check_k(c, k));
    ColumnStore st;
    st.m = m;
    st.k = k;
    if (m > (SIZE_MAX >> 1) / st.col()) return fail(c, H2AGG_ERR_NOMEM, "columns_create: the slab does not fit the address space");
    TRY(dev_alloc(c, st.d, m * st.col(), "column store"));
    HIP_TRY(c, hipMemsetAsync(st.d, 0, m * st.col(), c->stream));
    const uint64_t h = c->next_handle++;
    c->stores.emplace(h, std::move(st));
    *handle_out = h;
    return H2AGG_OK;
} API_CATCH

int h2agg_columns_destroy(h2agg_ctx* c, uint64_t handle) try {
    TRY(bind(c));
    ColumnStore* st = nullptr;
    TRY(find_store(c, handle, &st));
    TRY(join_tails(c));   // (as h2agg_bases_free: work on the context's other streams may still read the slab)
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->stores.erase(handle);
    return H2AGG_OK;
} API_CATCH

int h2agg_columns_info(h2agg_ctx* c, uint64_t handle, size_t* m_out, unsigned* k_out) try {
    TRY(bind(c));
    ColumnStore* st = nullptr;
    TRY(find_store(c, handle, &st));
    if (m_out) *m_out = st->m;
    if (k_out) *k_out = st->k;
    return H2AGG_OK;
} API_CATCH

int h2agg_columns_write(h2agg_ctx* c, uint64_t handle, size_t first, size_t count, const uint8_t* host) try {
    TRY(bind(c));
    ColumnStore* st = nullptr;
    uint8_t* d = nullptr;
    TRY(store_range(c, handle, first, count, &st, &d));
    if (!host) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    const size_t elems = count << st->k;
    if (c->dbg_phases) c->last_phases.clear();
    enum { STAGE, CHECK, PHASES };   // of h2agg_last_phases (debug key phases)
    static const char* const names[PHASES] = {"stage", "check"};
    PhaseClock phases(c);
    phases.mark(STAGE);
    TRY(stage_in(c, d, host, 32 * elems));
    TRY(clear_flags(c));
    phases.mark(CHECK);
    hipLaunchKernelGGL(k_columns_canonical, dim3(grid_for(c, elems)), dim3(BLOCK), 0, c->stream, (const uint8_t*)d, elems, c->d_flags);
    phases.mark(PhaseClock::END);
    HIP_TRY(c, hipGetLastError());
    const int rc = finish(c);
    phases.report(names, PHASES);
    return rc;
} API_CATCH

int h2agg_columns_read(h2agg_ctx* c, uint64_t handle, size_t first, size_t count, uint8_t* host) try {
    TRY(bind(c));
    ColumnStore* st = nullptr;
    uint8_t* d = nullptr;
    TRY(store_range(c, handle, first, count, &st, &d));
    if (!host) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(clear_flags(c));
    return stage_out(c, host, d, count * st->col());
} API_CATCH

int h2agg_columns_ptr(h2agg_ctx* c, uint64_t handle, size_t first, void** d_ptr_out) try {
    TRY(bind(c));
    if (d_ptr_out) *d_ptr_out = nullptr;
    ColumnStore* st = nullptr;
    uint8_t* d = nullptr;
    TRY(store_range(c, handle, first, 1, &st, &d));
    if (!d_ptr_out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    *d_ptr_out = d;
    return H2AGG_OK;
} API_CATCH

int h2agg_columns_move(h2agg_ctx* c, uint64_t src, size_t sfirst, uint64_t dst, size_t dfirst, size_t count, int32_t rotation) try {
    TRY(bind(c));
    ColumnStore *ss = nullptr, *ds = nullptr;
    uint8_t *d_src = nullptr, *d_dst = nullptr;
    TRY(store_range(c, src, sfirst, count, &ss, &d_src));
    TRY(store_range(c, dst, dfirst, count, &ds, &d_dst));
    if (ss->k != ds->k) return fail(c, H2AGG_ERR_INVALID, "columns_move: the two stores differ in k");
    const unsigned k = ss->k;
    const uint32_t rot = (uint32_t)((int64_t)rotation & (((int64_t)1 << k) - 1));   // the mathematical residue mod 2^k
    if (ss == ds && ranges_meet(sfirst, dfirst, count)) {
        if (sfirst == dfirst && rot == 0) return H2AGG_OK;   // onto itself, unrotated: nothing to do
        return fail(c, H2AGG_ERR_INVALID, "columns_move: the column ranges overlap");
    }
    ColumnsMoveArgs a;
    a.units_log = k + 1;
    a.shift = 2 * rot;
    const size_t units = (size_t)2 << k;
    const unsigned gx = (unsigned)((units + COLUMNS_MOVE_SPAN - 1) / COLUMNS_MOVE_SPAN);
    for (size_t j = 0; j < count; j += 65535) {   // (a grid's second dimension)
        a.src = (const uint4*)(d_src + ss->col() * j);
        a.dst = (uint4*)(d_dst + ds->col() * j);
        hipLaunchKernelGGL(k_columns_move, dim3(gx, (unsigned)std::min<size_t>(65535, count - j)), dim3(BLOCK), 0, c->stream, a);
    }
    HIP_TRY(c, hipGetLastError());
    return H2AGG_OK;
} API_CATCH

int h2agg_columns_fft(h2agg_ctx* c, uint64_t src, size_t sfirst, uint64_t dst, size_t dfirst, size_t count, int inverse,
                      const uint8_t shift[32]) try {
    TRY(bind(c));
    ColumnStore *ss = nullptr, *ds = nullptr;
    uint8_t *d_src = nullptr, *d_dst = nullptr;
    TRY(store_range(c, src, sfirst, count, &ss, &d_src));
    TRY(store_range(c, dst, dfirst, count, &ds, &d_dst));
    if (ss->k != ds->k) return fail(c, H2AGG_ERR_INVALID, "columns_fft: the two stores differ in k");
    if (ss == ds && sfirst != dfirst && ranges_meet(sfirst, dfirst, count))
        return fail(c, H2AGG_ERR_INVALID, "columns_fft: the column ranges overlap (in place is the same range)");
    ph::HFr s;
    TRY(fr_fft_check(c, ss->k, shift, &s));
    const FrFftSeg seg = {d_src, count};
    return fr_fft_queue_batch(c, &seg, 1, count, ss->k, inverse ? 1 : 0, shift ? &s : nullptr, d_dst);
} API_CATCH

int h2agg_columns_commit(h2agg_ctx* c, uint64_t bases_handle, uint64_t src, size_t first, size_t count, uint8_t* out_aff) try {
    TRY(bind(c));
    ColumnStore* st = nullptr;
    uint8_t* d = nullptr;
    TRY(store_range(c, src, first, count, &st, &d));
    if (!out_aff) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    Table* bases = nullptr;
    TRY(find_table(c, bases_handle, &bases));
    if (((size_t)1 << st->k) > bases->n) return fail(c, H2AGG_ERR_INVALID, "commit_columns: the table is shorter than 2^k");
    return commit_columns_run(c, bases_handle, d, count, st->k, out_aff);
} API_CATCH

int h2agg_columns_sigmas(h2agg_ctx* c, const uint32_t* mapping, size_t m, unsigned k, size_t usable, const uint8_t delta[32],
                         uint64_t dst_lagrange, size_t lfirst, uint64_t dst_coeff, size_t cfirst) try {
    TRY(bind(c));
    if (c->dbg_phases) c->last_phases.clear();
    TRY(perm_check_shape(c, m, k, usable));
    if (!mapping || !delta) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    if (!dst_lagrange && !dst_coeff) return fail(c, H2AGG_ERR_INVALID, "columns_sigmas: both outputs absent");
    ColumnStore* st = nullptr;
    uint8_t *s_lag = nullptr, *s_coeff = nullptr;
    if (dst_lagrange) {
        TRY(store_range(c, dst_lagrange, lfirst, m, &st, &s_lag));
        if (st->k != k) return fail(c, H2AGG_ERR_INVALID, "columns_sigmas: the store's k is not the call's");
    }
    if (dst_coeff) {
        TRY(store_range(c, dst_coeff, cfirst, m, &st, &s_coeff));
        if (st->k != k) return fail(c, H2AGG_ERR_INVALID, "columns_sigmas: the store's k is not the call's");
    }
    if (dst_lagrange == dst_coeff && ranges_meet(lfirst, cfirst, m))
        return fail(c, H2AGG_ERR_INVALID, "columns_sigmas: the two outputs overlap");
    ph::HFr d;
    TRY(fr_parse(c, delta, &d));
    const size_t n = (size_t)1 << k, cells = m * n, slab = 32 * cells;
    for (size_t x = 0; x < cells; ++x)   // (as h2agg_permutation_sigmas: the range of every entry, on the host)
        if (mapping[2 * x] >= m || mapping[2 * x + 1] >= n)
            return fail(c, H2AGG_ERR_INVALID, "permutation_sigmas: a mapping entry is outside the m x 2^k cells");
    // The columns are made in the context's work memory and reach the stores behind the device's verdict on the mapping: a
    // refused mapping leaves the stores as they were.  What the host-buffer call copies across PCIe is a device copy here.
    const bool both = s_lag && s_coeff;
    TRY(ensure(c, c->in_a, 8 * cells));
    TRY(ensure(c, c->out, slab));
    if (both) TRY(ensure(c, c->in_b, slab));
    uint8_t* d_lag = (uint8_t*)c->out.p;
    uint8_t* d_coeff = both ? (uint8_t*)c->in_b.p : d_lag;
    enum { STAGE, SIGMA, INVERSE, COPY, PHASES };
    static const char* const names[PHASES] = {"stage", "sigma", "inverse", "copy"};
    PhaseClock phases(c);
    phases.mark(STAGE);
    TRY(stage_in(c, c->in_a, (const uint8_t*)mapping, 8 * cells));
    TRY(clear_flags(c));
    phases.mark(SIGMA);
    TRY(perm_sigma_queue(c, c->in_a.p, m, k, usable, d, d_lag));
    phases.mark(INVERSE);
    if (s_coeff) {
        const FrFftSeg seg = {d_lag, m};
        TRY(fr_fft_queue_batch(c, &seg, 1, m, k, 1, nullptr, d_coeff));
    }
    phases.mark(COPY);
    const int rc = finish(c);
    if (rc != H2AGG_OK) {
        phases.report(names, PHASES, true);
        return rc;
    }
    if (s_lag) HIP_TRY(c, hipMemcpyAsync(s_lag, d_lag, slab, hipMemcpyDeviceToDevice, c->stream));
    if (s_coeff) HIP_TRY(c, hipMemcpyAsync(s_coeff, d_coeff, slab, hipMemcpyDeviceToDevice, c->stream));
    phases.mark(PhaseClock::END);
    phases.report(names, PHASES, true);   // (with the debug key only: waits for the last event)
    return H2AGG_OK;
} API_CATCH

int h2agg_columns_witness_check(h2agg_ctx* c, const h2agg_vk* vk, unsigned what, uint64_t advice, size_t afirst, uint64_t fixed,
                                size_t ffirst, uint64_t instance, size_t ifirst, const uint8_t* challenges, const uint8_t theta[32],
                                const uint32_t* mapping, size_t max_rows, uint32_t* counts, uint32_t* first_rows, uint32_t* rows,
                                uint64_t* total) try {
    TRY(bind(c));
    if (c->dbg_phases) c->last_phases.clear();
    if (!vk) return fail(c, H2AGG_ERR_INVALID, "null verifying key");
    if (!rows) max_rows = 0;
    TRY(fr_check_k(c, vk->k));
    const uint8_t *d_advice = nullptr, *d_fixed = nullptr, *d_instance = nullptr;
    TRY(store_slab_of_key(c, advice, afirst, vk->num_advice, vk->k, &d_advice));
    TRY(store_slab_of_key(c, fixed, ffirst, qe_nfixed(*vk), vk->k, &d_fixed));
    TRY(store_slab_of_key(c, instance, ifirst, vk->num_instance, vk->k, &d_instance));
    WcCall call;
    TRY(wc_check(c, vk, what, d_advice, d_fixed, d_instance, challenges, theta, mapping, max_rows, counts, first_rows, total, &call));
    const WcLayout& l = call.l;
    const size_t n = l.n;
    if (call.permutation)
        for (size_t x = 0; x < l.P * n; ++x)
            if (mapping[2 * x] >= l.P || mapping[2 * x + 1] >= n)
                return fail(c, H2AGG_ERR_INVALID, "witness_check: a mapping entry is outside the P x 2^k cells");
    if (l.C == 0) {
        *total = 0;
        return H2AGG_OK;
    }
    if (call.permutation) {
        TRY(ensure(c, c->in_b, 8 * l.P * n));
        TRY(stage_in(c, c->in_b, (const uint8_t*)mapping, 8 * l.P * n));
    }
    TRY(clear_flags(c));
    TRY(wc_queue(c, *vk, call, d_advice, d_fixed, d_instance, c->in_b.p));
    return wc_report_out(c, l, max_rows, counts, first_rows, rows, total);
} API_CATCH

// The lookup batches over stores (lookup.inc has the host-slab forms and the chunk loop).  With a host block to fill (status /
// last) the call is synchronous; without, it is queued and reports through the context's device status.
int h2agg_lookup_store_permute(h2agg_ctx* c, uint64_t a, size_t afirst, uint64_t s, size_t sfirst, size_t count, size_t u,
                               uint64_t ap, size_t apfirst, uint64_t sp, size_t spfirst, uint32_t* status) try {
    TRY(bind(c));
    if (c->dbg_phases) c->last_phases.clear();
    if (count == 0 || count > LK_MAX_LOOKUPS) return fail(c, H2AGG_ERR_INVALID, "count must be 1 .. 65535");
    const uint64_t h[4] = {a, s, ap, sp};
    const size_t first[4] = {afirst, sfirst, apfirst, spfirst};
    ColumnStore* st[4] = {};
    uint8_t* d[4] = {};
    for (int i = 0; i < 4; ++i) {
        TRY(store_range(c, h[i], first[i], count, &st[i], &d[i]));
        if (st[i]->k != st[0]->k) return fail(c, H2AGG_ERR_INVALID, "lookup_store_permute: the stores differ in k");
    }
    TRY(prod_check_ku(c, st[0]->k, u));
    for (int o = 2; o < 4; ++o)
        for (int i = 0; i < o; ++i)
            if (st[o] == st[i] && ranges_meet(first[o], first[i], count))
                return fail(c, H2AGG_ERR_INVALID, "lookup_store_permute: ap / sp must not overlap a, s or each other");
    if (u == 0) {
        if (status) memset(status, 0, 4 * count);
        return H2AGG_OK;
    }
    enum { SORT, RANK, PHASES };   // of h2agg_last_phases (debug key phases)
    static const char* const names[PHASES] = {"sort", "rank"};
    PhaseClock phases(c);
    uint32_t* d_status = nullptr;
    if (status) {
        TRY(ensure(c, c->lk_status, 4 * count));
        d_status = (uint32_t*)c->lk_status.p;
        TRY(clear_flags(c));
    }
    TRY(lk_batch_permute_queue(c, d[0], d[1], st[0]->col(), count, u, d[2], d[3], d_status, &phases, SORT));
    phases.mark(PhaseClock::END);
    const int rc = status ? lk_batch_finish(c, d_status, count, status) : H2AGG_OK;
    phases.report(names, PHASES);   // (with the debug key only: waits for the last event)
    return rc;
} API_CATCH

int h2agg_lookup_store_product(h2agg_ctx* c, uint64_t a, size_t afirst, uint64_t s, size_t sfirst, uint64_t ap, size_t apfirst,
                               uint64_t sp, size_t spfirst, size_t count, size_t u, const uint8_t beta[32], const uint8_t gamma[32],
                               uint64_t z, size_t zfirst, uint8_t* last) try {
    TRY(bind(c));
    if (c->dbg_phases) c->last_phases.clear();
    if (count == 0 || count > LK_MAX_LOOKUPS) return fail(c, H2AGG_ERR_INVALID, "count must be 1 .. 65535");
    const uint64_t h[5] = {a, s, ap, sp, z};
    const size_t first[5] = {afirst, sfirst, apfirst, spfirst, zfirst};
    ColumnStore* st[5] = {};
    uint8_t* d[5] = {};
    for (int i = 0; i < 5; ++i) {
        TRY(store_range(c, h[i], first[i], count, &st[i], &d[i]));
        if (st[i]->k != st[0]->k) return fail(c, H2AGG_ERR_INVALID, "lookup_store_product: the stores differ in k");
    }
    ph::HFr bf, gf;
    TRY(lookup_check(c, st[0]->k, u, beta, gamma, &bf, &gf));
    for (int i = 0; i < 4; ++i)
        if (st[4] == st[i] && ranges_meet(first[4], first[i], count))
            return fail(c, H2AGG_ERR_INVALID, "lookup_store_product: z must not overlap a, s, ap or sp");
    enum { TERMS, INVERT, SCAN, PHASES };   // of h2agg_last_phases (debug key phases)
    static const char* const names[PHASES] = {"terms", "invert", "scan"};
    PhaseClock phases(c);
    const size_t col = st[0]->col();
    if (last) TRY(clear_flags(c));
    TRY(lk_batch_product_queue(c, d[0], d[1], d[2], d[3], col, count, u, bf, gf, d[4], col, &phases, TERMS));
    phases.mark(PhaseClock::END);
    int rc = H2AGG_OK;
    if (last) {
        HIP_TRY(c, hipMemcpy2DAsync(last, 32, d[4] + 32 * u, col, 32, count, hipMemcpyDeviceToHost, c->stream));
        rc = finish(c);
    }
    phases.report(names, PHASES);   // (with the debug key only: waits for the last event)
    return rc;
} API_CATCH

int h2agg_columns_shplonk_begin(h2agg_ctx* c, uint64_t g_handle, uint64_t src, size_t first, size_t npoly, const uint32_t* queries,
                                size_t nq, const uint8_t* points, size_t npoints, const uint8_t* evals, const uint8_t y[32],
                                const uint8_t v[32], uint8_t h1_aff[64], h2agg_shplonk** out) try {
    TRY(bind(c));
    if (out) *out = nullptr;
    ColumnStore* st = nullptr;
    uint8_t* d = nullptr;
    TRY(store_range(c, src, first, npoly, &st, &d));
    return shplonk_begin(c, g_handle, d, true, npoly, st->k, queries, nq, points, npoints, evals, y, v, h1_aff, out);
} API_CATCH

}  // extern "C"
