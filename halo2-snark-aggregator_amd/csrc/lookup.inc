// The lookup argument in front of its grand product, host side (included into h2agg.hip behind prod.inc: shares the context
// internals; kernels, sort plan and bounds in lookup_kernels.hpp, checks in fr_host.inc, staging in host.inc):
// h2agg_lookup_permute[_device], h2agg_fr_columns_compress[_device].  They stand for halo2_proofs'
// lookup::prover::permute_expression_pair and the theta-fold of commit_permuted — an unvendored git dependency of the
// reference, recalled from upstream (DESIGN.md section 2); the yardstick is the definition in include/h2agg.h.  Which pair a
// verifier accepts is pinned by halo2-snark-aggregator-api/src/systems/halo2/lookup.rs:98-113.

namespace {

constexpr size_t LK_MAX_COLUMNS = (size_t)1 << 16;

// The tile and what goes with it (lookup_kernels.hpp, "Geometry").  Below the default tile — only the debug key fr_sort_tile
// gets there — the scan's step, the threads that take keys in the byte histogram and its grid shrink with the tile, so that
// small inputs walk the step and stride loops that the default geometry reaches only from 2^18 rows up.
struct LkGeom {
    unsigned t;              // log2 of the keys per workgroup
    uint32_t scan_step;      // entries per step of k_lk_scan_rows: a multiple of 4, 4 .. 1024
    uint32_t hist_lanes;     // threads of a workgroup of k_lk_digit_hist that take keys, 4 .. 256
    uint32_t hist_grid;      // most workgroups of k_lk_digit_hist
};

LkGeom lk_geom(const h2agg_ctx* c) {
    const unsigned t = c->dbg_fr_sort_tile ? (unsigned)c->dbg_fr_sort_tile : LK_TILE_LOG;
    if (t >= LK_TILE_LOG) return {t, LK_SCAN_STEP, (uint32_t)LK_THREADS, LK_HIST_GRID};
    const uint32_t quarter = 1u << (t - 2);   // 4 .. 256 as t is LK_TILE_LOG_MIN .. LK_TILE_LOG - 1
    return {t, quarter, quarter, 2u};
}

// The work memory of one h2agg_lookup_permute over u >= 1 rows, cut out of the context's lk_work (offsets in bytes, each a
// multiple of 256): two key buffers per sort, the five u32 columns of the rank step, the tile sums of its prefix sums, the
// count matrix of a pass (shared by the two sorts: they run one behind the other), the histograms and plans of both sorts.
struct LkLayout {
    size_t keys[4], non_head, left, non_head_pre, left_pre, left_idx, sums, counts, hist[2], plan[2], total;
    uint32_t tiles, ncols;
};

LkLayout lk_layout(size_t u, unsigned t) {
    LkLayout l;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    };
    l.tiles = (uint32_t)((u + ((size_t)1 << t) - 1) >> t);
    l.ncols = LK_WAVES * l.tiles;
    for (size_t& k : l.keys) k = take(32 * u);
    l.non_head = take(4 * u);
    l.left = take(4 * u);
    l.non_head_pre = take(4 * (u + 1));
    l.left_pre = take(4 * (u + 1));
    l.left_idx = take(4 * u);
    l.sums = take(4 * (size_t)l.tiles);
    l.counts = take(4 * (size_t)LK_BINS * l.ncols);
    for (int q = 0; q < 2; ++q) {
        l.hist[q] = take(4 * LK_PASSES * LK_BINS);
        l.plan[q] = take(4 * LK_PLAN_WORDS);
    }
    l.total = at;
    return l;
}

// Queues the sort of u >= 1 keys: the histogram of every byte, the plan, then three launches per byte (each returns at once
// where the plan skips the pass).  Behind it plan[32] says which of in / w0 / w1 holds the ascending keys.
int lk_sort_queue(h2agg_ctx* c, const uint8_t* d_in, const LkLayout& l, int q, size_t u, const LkGeom& g) {
    uint8_t* w = (uint8_t*)c->lk_work.p;
    FrSortArgs a;
    a.in = d_in;
    a.w0 = w + l.keys[2 * q];
    a.w1 = w + l.keys[2 * q + 1];
    a.hist = (uint32_t*)(w + l.hist[q]);
    a.plan = (uint32_t*)(w + l.plan[q]);
    a.counts = (uint32_t*)(w + l.counts);
    a.flags = c->d_flags;
    a.u = (uint32_t)u;
    a.t = g.t;
    a.ncols = l.ncols;
    a.pass = 0;
    a.hist_lanes = g.hist_lanes;
    HIP_TRY(c, hipMemsetAsync(a.hist, 0, 4 * LK_PASSES * LK_BINS, c->stream));
    const unsigned hist_grid = (unsigned)std::min<size_t>((u + g.hist_lanes - 1) / g.hist_lanes, g.hist_grid);
    hipLaunchKernelGGL(k_lk_digit_hist, dim3(hist_grid), dim3(LK_THREADS), 0, c->stream, a);
    hipLaunchKernelGGL(k_lk_plan, dim3(1), dim3(LK_THREADS), 0, c->stream, a);
    for (uint32_t p = 0; p < LK_PASSES; ++p) {
        a.pass = p;
        hipLaunchKernelGGL(k_lk_tile_hist, dim3(l.tiles), dim3(LK_THREADS), 0, c->stream, a);
        hipLaunchKernelGGL(k_lk_scan_rows, dim3(LK_BINS), dim3(LK_THREADS), 0, c->stream, a.counts, a.ncols, (const uint32_t*)a.hist,
                           (const uint32_t*)a.plan, p, g.scan_step);
        hipLaunchKernelGGL(k_lk_scatter, dim3(l.tiles), dim3(LK_THREADS), 0, c->stream, a);
    }
    HIP_TRY(c, hipGetLastError());
    return H2AGG_OK;
}

// dst[i] = src[0] + .. + src[i - 1], i <= n (n >= 1): tile sums, their prefix (one workgroup), the tiles' prefixes
void lk_prefix_queue(h2agg_ctx* c, const uint32_t* src, uint32_t* sums, uint32_t* dst, size_t n, const LkLayout& l, const LkGeom& g) {
    const unsigned t = g.t;
    hipLaunchKernelGGL(k_lk_block_reduce, dim3(l.tiles), dim3(LK_THREADS), 0, c->stream, src, sums, (uint32_t)n, t);
    hipLaunchKernelGGL(k_lk_scan_rows, dim3(1), dim3(LK_THREADS), 0, c->stream, sums, l.tiles, (const uint32_t*)nullptr,
                       (const uint32_t*)nullptr, 0u, g.scan_step);
    hipLaunchKernelGGL(k_lk_block_scan, dim3(l.tiles), dim3(LK_THREADS), 0, c->stream, src, (const uint32_t*)sums, dst, (uint32_t)n, t);
}

// Both sorts, the heads and their table rows, the two prefix sums, the leftover list, the fill.  Nothing synchronises unless
// the work memory has to grow; nothing is read back.  u >= 1.
int lk_permute_queue(h2agg_ctx* c, const uint8_t* d_a, const uint8_t* d_s, size_t u, uint8_t* d_ap, uint8_t* d_sp) {
    const LkGeom g = lk_geom(c);
    const LkLayout l = lk_layout(u, g.t);
    TRY(ensure(c, c->lk_work, l.total));
    uint8_t* w = (uint8_t*)c->lk_work.p;
    TRY(lk_sort_queue(c, d_a, l, 0, u, g));
    TRY(lk_sort_queue(c, d_s, l, 1, u, g));
    FrLookupPermuteArgs p;
    p.a_in = d_a;
    p.a_w0 = w + l.keys[0];
    p.a_w1 = w + l.keys[1];
    p.a_plan = (const uint32_t*)(w + l.plan[0]);
    p.s_in = d_s;
    p.s_w0 = w + l.keys[2];
    p.s_w1 = w + l.keys[3];
    p.s_plan = (const uint32_t*)(w + l.plan[1]);
    p.non_head = (uint32_t*)(w + l.non_head);
    p.left = (uint32_t*)(w + l.left);
    p.non_head_pre = (uint32_t*)(w + l.non_head_pre);
    p.left_pre = (uint32_t*)(w + l.left_pre);
    p.left_idx = (uint32_t*)(w + l.left_idx);
    p.ap = d_ap;
    p.sp = d_sp;
    p.flags = c->d_flags;
    p.u = (uint32_t)u;
    const dim3 rows((unsigned)((u + BLOCK - 1) / BLOCK));
    HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)p.left, 1, u, c->stream));
    hipLaunchKernelGGL(k_lk_heads, rows, dim3(BLOCK), 0, c->stream, p);
    uint32_t* sums = (uint32_t*)(w + l.sums);
    lk_prefix_queue(c, p.non_head, sums, p.non_head_pre, u, l, g);
    lk_prefix_queue(c, p.left, sums, p.left_pre, u, l, g);
    hipLaunchKernelGGL(k_lk_leftovers, rows, dim3(BLOCK), 0, c->stream, p);
    hipLaunchKernelGGL(k_lk_fill, rows, dim3(BLOCK), 0, c->stream, p);
    HIP_TRY(c, hipGetLastError());
    return H2AGG_OK;
}

bool lk_overlap(const void* p, const void* q, size_t bytes) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + bytes && b < a + bytes;
}

int lk_compress_check(h2agg_ctx* c, size_t m, unsigned k, const uint8_t* theta, ph::HFr* tf) {
    TRY(fr_check_k(c, k));
    if (m == 0 || m > LK_MAX_COLUMNS) return fail(c, H2AGG_ERR_INVALID, "m must be 1 .. 65536");
    if (!theta) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    return fr_parse(c, theta, tf);
}

// out[i] = sum_j theta^(m - 1 - j) cols[j][i]: k_fr_poly_lincomb over one group, the descriptor written on the stream
int lk_compress_queue(h2agg_ctx* c, const uint8_t* d_cols, size_t m, unsigned k, const ph::HFr& theta, uint8_t* d_out) {
    const size_t n = (size_t)1 << k;
    TRY(ensure(c, c->lk_desc, 4 * (m + 2)));
    uint32_t* desc = (uint32_t*)c->lk_desc.p;
    hipLaunchKernelGGL(k_lk_compress_desc, dim3((unsigned)((m + 2 + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream, desc, (uint32_t)m);
    FrLincombArgs la;
    hfr_words(ph::mul(theta, fr_radix()), la.v);
    la.polys = d_cols;
    la.dst = d_out;
    la.list = desc;
    la.goff = desc + m;
    la.flags = c->d_flags;
    la.n = (uint32_t)n;
    hipLaunchKernelGGL(k_fr_poly_lincomb, dim3((unsigned)((n + BLOCK - 1) / BLOCK), 1u), dim3(BLOCK), 0, c->stream, la);
    HIP_TRY(c, hipGetLastError());
    return H2AGG_OK;
}

}  // namespace

extern "C" {

int h2agg_lookup_permute_device(h2agg_ctx* c, const void* d_a, const void* d_s, unsigned k, size_t u, void* d_ap, void* d_sp) try {
    TRY(bind(c));
    TRY(prod_check_ku(c, k, u));
    if (!d_a || !d_s || !d_ap || !d_sp) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    if (u == 0) return H2AGG_OK;
    const size_t bytes = 32 * u;
    if (lk_overlap(d_ap, d_a, bytes) || lk_overlap(d_ap, d_s, bytes) || lk_overlap(d_sp, d_a, bytes) || lk_overlap(d_sp, d_s, bytes) ||
        lk_overlap(d_ap, d_sp, bytes))
        return fail(c, H2AGG_ERR_INVALID, "ap / sp must not overlap a, s or each other");
    return lk_permute_queue(c, (const uint8_t*)d_a, (const uint8_t*)d_s, u, (uint8_t*)d_ap, (uint8_t*)d_sp);
} API_CATCH

int h2agg_lookup_permute(h2agg_ctx* c, const uint8_t* a, const uint8_t* s, unsigned k, size_t u, uint8_t* ap, uint8_t* sp) try {
    TRY(bind(c));
    TRY(prod_check_ku(c, k, u));
    if (!a || !s || !ap || !sp) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    if (u == 0) return H2AGG_OK;
    const size_t bytes = 32 * u;
    TRY(ensure(c, c->in_a, 2 * bytes));
    TRY(ensure(c, c->out, 2 * bytes));
    TRY(stage_in(c, c->in_a, a, bytes));
    TRY(stage_in(c, c->in_a, s, bytes, bytes));
    TRY(clear_flags(c));
    const uint8_t* d_in = (const uint8_t*)c->in_a.p;
    uint8_t* d_out = (uint8_t*)c->out.p;
    TRY(lk_permute_queue(c, d_in, d_in + bytes, u, d_out, d_out + bytes));
    HIP_TRY(c, hipMemcpyAsync(ap, d_out, bytes, hipMemcpyDeviceToHost, c->stream));
    return stage_out(c, sp, d_out + bytes, bytes);
} API_CATCH

int h2agg_fr_columns_compress_device(h2agg_ctx* c, const void* d_cols, size_t m, unsigned k, const uint8_t theta[32], void* d_out) try {
    TRY(bind(c));
    ph::HFr tf;
    TRY(lk_compress_check(c, m, k, theta, &tf));
    if (!d_cols || !d_out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    return lk_compress_queue(c, (const uint8_t*)d_cols, m, k, tf, (uint8_t*)d_out);
} API_CATCH

int h2agg_fr_columns_compress(h2agg_ctx* c, const uint8_t* cols, size_t m, unsigned k, const uint8_t theta[32], uint8_t* out) try {
    TRY(bind(c));
    ph::HFr tf;
    TRY(lk_compress_check(c, m, k, theta, &tf));
    if (!cols || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    const size_t col = (size_t)32 << k;
    TRY(ensure(c, c->in_a, m * col));
    TRY(ensure(c, c->out, col));
    TRY(stage_in(c, c->in_a, cols, m * col));
    TRY(clear_flags(c));
    TRY(lk_compress_queue(c, (const uint8_t*)c->in_a.p, m, k, tf, (uint8_t*)c->out.p));
    return stage_out(c, out, c->out.p, col);
} API_CATCH

}  // extern "C"
