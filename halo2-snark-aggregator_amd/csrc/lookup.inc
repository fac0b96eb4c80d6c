// The lookup argument in front of its grand product, host side (included into h2agg.hip behind prod.inc: shares the context
// internals; kernels, sort plan and bounds in lookup_kernels.hpp, checks in fr_host.inc, staging in host.inc):
// h2agg_lookup_permute[_device], h2agg_fr_columns_compress[_device], and the batches over host slabs — h2agg_lookup_batch_permute,
// h2agg_lookup_batch_product, h2agg_lookup_configure (DESIGN.md 5.21; the store forms are in columns.inc, the chunk of the
// product in prod.inc).  They stand for halo2_proofs'
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

// Lookups per set of launches of a batch over u rows: LK_BATCH_ROWS / u of them, at least 1, at most LK_BATCH_MAX; fewer where
// h2agg_lookup_configure asks for fewer.  B u <= 2^24 is what one inversion takes (prod.inc) and the 2.4 GiB of work memory a
// single call at u = 2^24 - 1 may already hold; 1024 bounds the histograms of a chunk at 64 MiB and keeps the 2 B sort columns
// inside a grid's second dimension.
constexpr size_t LK_BATCH_ROWS = (size_t)1 << 24;
constexpr size_t LK_BATCH_MAX = 1024;
constexpr size_t LK_MAX_LOOKUPS = 65535;
// the bits of a batch's status words as include/h2agg.h names them are the device's status bits
static_assert(H2AGG_LOOKUP_STATUS_NONCANONICAL == FLAG_NONCANONICAL && H2AGG_LOOKUP_STATUS_NOT_IN_TABLE == FLAG_NOT_IN_TABLE,
              "include/h2agg.h names the bits the kernels raise");

size_t lk_batch_chunk(size_t u, size_t forced) {
    const size_t by_rows = std::min(std::max(LK_BATCH_ROWS / std::max<size_t>(u, 1), (size_t)1), LK_BATCH_MAX);
    return forced && forced < by_rows ? forced : by_rows;
}

// The work memory of one chunk of nb lookups over u >= 1 rows, cut out of the context's lk_work (offsets in bytes, each a
// multiple of 256).  2 nb sort columns — c < nb the input column of lookup c, nb + c the table column — with, each, two key
// buffers (w0, w1: key_stride apart), a count matrix, the histograms and a plan; per lookup the five u32 columns of the rank
// step, dense [nb][u] (the prefixes [nb][u + 1]), and the tile sums of its prefix sums [nb][tiles].
struct LkLayout {
    size_t w0, w1, key_stride, non_head, left, non_head_pre, left_pre, left_idx, sums, counts, hist, plan, total;
    uint32_t tiles, ncols;
};

LkLayout lk_layout(size_t u, unsigned t, size_t nb = 1) {
    LkLayout l;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    };
    l.tiles = (uint32_t)((u + ((size_t)1 << t) - 1) >> t);
    l.ncols = LK_WAVES * l.tiles;
    l.key_stride = (32 * u + 255) & ~(size_t)255;
    l.w0 = take(2 * nb * l.key_stride);
    l.w1 = take(2 * nb * l.key_stride);
    l.non_head = take(4 * nb * u);
    l.left = take(4 * nb * u);
    l.non_head_pre = take(4 * nb * (u + 1));
    l.left_pre = take(4 * nb * (u + 1));
    l.left_idx = take(4 * nb * u);
    l.sums = take(4 * nb * (size_t)l.tiles);
    l.counts = take(4 * 2 * nb * (size_t)LK_BINS * l.ncols);
    l.hist = take(4 * 2 * nb * (size_t)(LK_PASSES * LK_BINS));
    l.plan = take(4 * 2 * nb * (size_t)LK_PLAN_WORDS);
    l.total = at;
    return l;
}

// Queues the sorts of `columns` <= 2 nb sort columns of u >= 1 keys each in ONE chain of launches: the histogram of every byte,
// the plans, then three launches per byte (each workgroup returns at once where its column's plan skips the pass).  Sort
// column c < nb reads d_in + c in_stride, column nb + c reads d_in2 + c in_stride.  Behind it plan[32] of a column says which
// of its in / w0 / w1 holds the ascending keys.  d_status: the chunk's word per lookup, or null.
int lk_sort_queue(h2agg_ctx* c, const uint8_t* d_in, const uint8_t* d_in2, size_t in_stride, const LkLayout& l, size_t nb,
                  size_t columns, size_t u, const LkGeom& g, uint32_t* d_status) {
    uint8_t* w = (uint8_t*)c->lk_work.p;
    FrSortArgs a;
    a.in = d_in;
    a.in2 = d_in2;
    a.w0 = w + l.w0;
    a.w1 = w + l.w1;
    a.hist = (uint32_t*)(w + l.hist);
    a.plan = (uint32_t*)(w + l.plan);
    a.counts = (uint32_t*)(w + l.counts);
    a.flags = c->d_flags;
    a.status = d_status;
    a.in_stride = in_stride;
    a.key_stride = l.key_stride;
    a.nb = (uint32_t)nb;
    a.u = (uint32_t)u;
    a.t = g.t;
    a.ncols = l.ncols;
    a.pass = 0;
    a.hist_lanes = g.hist_lanes;
    const unsigned ny = (unsigned)columns;
    HIP_TRY(c, hipMemsetAsync(a.hist, 0, 4 * columns * (size_t)(LK_PASSES * LK_BINS), c->stream));
    const unsigned hist_grid = (unsigned)std::min<size_t>((u + g.hist_lanes - 1) / g.hist_lanes, g.hist_grid);
    hipLaunchKernelGGL(k_lk_digit_hist, dim3(hist_grid, ny), dim3(LK_THREADS), 0, c->stream, a);
    hipLaunchKernelGGL(k_lk_plan, dim3(1, ny), dim3(LK_THREADS), 0, c->stream, a);
    for (uint32_t p = 0; p < LK_PASSES; ++p) {
        a.pass = p;
        hipLaunchKernelGGL(k_lk_tile_hist, dim3(l.tiles, ny), dim3(LK_THREADS), 0, c->stream, a);
        hipLaunchKernelGGL(k_lk_scan_rows, dim3(LK_BINS, ny), dim3(LK_THREADS), 0, c->stream, a.counts, a.ncols, (const uint32_t*)a.hist,
                           (const uint32_t*)a.plan, p, g.scan_step);
        hipLaunchKernelGGL(k_lk_scatter, dim3(l.tiles, ny), dim3(LK_THREADS), 0, c->stream, a);
    }
    HIP_TRY(c, hipGetLastError());
    return H2AGG_OK;
}

// the sort of ONE column (the witness check's table): sort column 0 of a layout of one lookup
int lk_sort_queue(h2agg_ctx* c, const uint8_t* d_in, const LkLayout& l, size_t u, const LkGeom& g) {
    return lk_sort_queue(c, d_in, d_in, 0, l, 1, 1, u, g, nullptr);
}

// dst[b][i] = src[b][0] + .. + src[b][i - 1], i <= n (n >= 1), for each of nb lookups: tile sums, their prefixes (a workgroup
// per lookup), the tiles' prefixes
void lk_prefix_queue(h2agg_ctx* c, const uint32_t* src, uint32_t* sums, uint32_t* dst, size_t n, size_t nb, const LkLayout& l,
                     const LkGeom& g) {
    const unsigned t = g.t, ny = (unsigned)nb;
    hipLaunchKernelGGL(k_lk_block_reduce, dim3(l.tiles, ny), dim3(LK_THREADS), 0, c->stream, src, sums, (uint32_t)n, t);
    hipLaunchKernelGGL(k_lk_scan_rows, dim3(ny), dim3(LK_THREADS), 0, c->stream, sums, l.tiles, (const uint32_t*)nullptr,
                       (const uint32_t*)nullptr, 0u, g.scan_step);
    hipLaunchKernelGGL(k_lk_block_scan, dim3(l.tiles, ny), dim3(LK_THREADS), 0, c->stream, src, (const uint32_t*)sums, dst, (uint32_t)n, t);
}

// One chunk of nb lookups, nb u <= LK_BATCH_ROWS: lookup b reads column b of d_a and d_s and writes rows < u of column b of
// d_ap and d_sp (col_stride bytes apart).  All 2 nb sorts in one chain, the heads and their table rows, the two prefix sums,
// the leftover lists, the fill: memset + 2 + 96 + 10 launches whatever nb is.  Nothing synchronises unless the work memory has
// to grow; nothing is read back.  u >= 1.  phases (or null) is marked with first in front of the sorts, first + 1 in front
// of the rank step.
int lk_permute_queue(h2agg_ctx* c, const uint8_t* d_a, const uint8_t* d_s, size_t col_stride, size_t nb, size_t u, uint8_t* d_ap,
                     uint8_t* d_sp, uint32_t* d_status, PhaseClock* phases = nullptr, int first = 0) {
    const LkGeom g = lk_geom(c);
    const LkLayout l = lk_layout(u, g.t, nb);
    TRY(ensure(c, c->lk_work, l.total));
    uint8_t* w = (uint8_t*)c->lk_work.p;
    if (phases) phases->mark(first);
    TRY(lk_sort_queue(c, d_a, d_s, col_stride, l, nb, 2 * nb, u, g, d_status));
    if (phases) phases->mark(first + 1);
    FrLookupPermuteArgs p;
    p.a_in = d_a;
    p.a_w0 = w + l.w0;
    p.a_w1 = w + l.w1;
    p.a_plan = (const uint32_t*)(w + l.plan);
    p.s_in = d_s;
    p.s_w0 = w + l.w0 + nb * l.key_stride;
    p.s_w1 = w + l.w1 + nb * l.key_stride;
    p.s_plan = (const uint32_t*)(w + l.plan) + nb * LK_PLAN_WORDS;
    p.non_head = (uint32_t*)(w + l.non_head);
    p.left = (uint32_t*)(w + l.left);
    p.non_head_pre = (uint32_t*)(w + l.non_head_pre);
    p.left_pre = (uint32_t*)(w + l.left_pre);
    p.left_idx = (uint32_t*)(w + l.left_idx);
    p.ap = d_ap;
    p.sp = d_sp;
    p.flags = c->d_flags;
    p.status = d_status;
    p.col_stride = col_stride;
    p.key_stride = l.key_stride;
    p.u = (uint32_t)u;
    const dim3 rows((unsigned)((u + BLOCK - 1) / BLOCK), (unsigned)nb);
    HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)p.left, 1, nb * u, c->stream));
    hipLaunchKernelGGL(k_lk_heads, rows, dim3(BLOCK), 0, c->stream, p);
    uint32_t* sums = (uint32_t*)(w + l.sums);
    lk_prefix_queue(c, p.non_head, sums, p.non_head_pre, u, nb, l, g);
    lk_prefix_queue(c, p.left, sums, p.left_pre, u, nb, l, g);
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

// ---- batches: every lookup of a circuit in one call, chunk by chunk on the context's stream (DESIGN.md 5.21)

int lk_batch_check(h2agg_ctx* c, size_t count, unsigned k, size_t u) {
    TRY(prod_check_ku(c, k, u));
    if (count == 0 || count > LK_MAX_LOOKUPS) return fail(c, H2AGG_ERR_INVALID, "count must be 1 .. 65535");
    return H2AGG_OK;
}

// the permutations of `count` lookups over device slabs (columns col_stride bytes apart); d_status: count words or null
// (zeroed here).  u >= 1.
int lk_batch_permute_queue(h2agg_ctx* c, const uint8_t* d_a, const uint8_t* d_s, size_t col_stride, size_t count, size_t u,
                           uint8_t* d_ap, uint8_t* d_sp, uint32_t* d_status, PhaseClock* phases, int first) {
    if (d_status) HIP_TRY(c, hipMemsetAsync(d_status, 0, 4 * count, c->stream));
    const size_t B = lk_batch_chunk(u, c->cfg_lookup_chunk);
    for (size_t j = 0; j < count; j += B) {
        const size_t nb = std::min(B, count - j), at = j * col_stride;
        TRY(lk_permute_queue(c, d_a + at, d_s + at, col_stride, nb, u, d_ap + at, d_sp + at, d_status ? d_status + j : nullptr, phases, first));
    }
    return H2AGG_OK;
}

// the Z columns of `count` lookups over device slabs: z[0 .. u] of every column of d_z
int lk_batch_product_queue(h2agg_ctx* c, const uint8_t* d_a, const uint8_t* d_s, const uint8_t* d_ap, const uint8_t* d_sp,
                           size_t col_stride, size_t count, size_t u, const ph::HFr& beta, const ph::HFr& gamma, uint8_t* d_z,
                           size_t z_stride, PhaseClock* phases, int first) {
    const size_t B = lk_batch_chunk(u, c->cfg_lookup_chunk);
    for (size_t j = 0; j < count; j += B) {
        const size_t nb = std::min(B, count - j), at = j * col_stride;
        TRY(lookup_chunk_queue(c, d_a + at, d_s + at, d_ap + at, d_sp + at, col_stride, nb, u, beta, gamma, d_z + j * z_stride, z_stride,
                               phases, first));
    }
    return H2AGG_OK;
}

// The tail of a synchronous batch: the status words back (d_status null: none), finish(), and the code of the single call
// of the lowest-numbered lookup that failed.  status (the caller's, may be null) gets the words.
int lk_batch_finish(h2agg_ctx* c, const uint32_t* d_status, size_t count, uint32_t* status) {
    std::vector<uint32_t> words(d_status ? count : 0, 0u);
    if (d_status) HIP_TRY(c, hipMemcpyAsync(words.data(), d_status, 4 * count, hipMemcpyDeviceToHost, c->stream));
    const int rc = finish(c);
    if (status) memset(status, 0, 4 * count);
    if (status && d_status) memcpy(status, words.data(), 4 * count);
    for (size_t j = 0; j < words.size(); ++j)
        if (words[j]) return flags_to_status(c, words[j], false);
    return rc;
}

// rows [0, rows) of `count` columns between a host slab and a device slab of other pitch
int lk_copy_rows(h2agg_ctx* c, void* dst, size_t dpitch, const void* src, size_t spitch, size_t rows, size_t count, hipMemcpyKind kind) {
    if (rows) HIP_TRY(c, hipMemcpy2DAsync(dst, dpitch, src, spitch, 32 * rows, count, kind, c->stream));
    return H2AGG_OK;
}

}  // namespace

extern "C" {

size_t h2agg_lookup_chunk_rule(size_t u, size_t batch_chunk) { return lk_batch_chunk(u, batch_chunk > LK_BATCH_MAX ? 0 : batch_chunk); }

int h2agg_lookup_configure(h2agg_ctx* c, size_t batch_chunk) try {
    TRY(bind(c));
    if (batch_chunk > LK_BATCH_MAX) return fail(c, H2AGG_ERR_INVALID, "lookup_configure: batch_chunk must be 0 .. 1024");
    c->cfg_lookup_chunk = batch_chunk;
    return H2AGG_OK;
} API_CATCH

int h2agg_lookup_batch_permute(h2agg_ctx* c, const uint8_t* a, const uint8_t* s, size_t count, unsigned k, size_t u, uint8_t* ap,
                               uint8_t* sp, uint32_t* status) try {
    TRY(bind(c));
    if (c->dbg_phases) c->last_phases.clear();
    TRY(lk_batch_check(c, count, k, u));
    if (!a || !s || !ap || !sp) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    const size_t col = (size_t)32 << k, slab = count * col;
    if (lk_overlap(ap, a, slab) || lk_overlap(ap, s, slab) || lk_overlap(sp, a, slab) || lk_overlap(sp, s, slab) || lk_overlap(ap, sp, slab))
        return fail(c, H2AGG_ERR_INVALID, "ap / sp must not overlap a, s or each other");
    if (u == 0) {
        if (status) memset(status, 0, 4 * count);
        return H2AGG_OK;
    }
    const size_t ds = 32 * u, half = count * ds;   // the device twins are dense: [count][u]
    TRY(ensure(c, c->in_a, 2 * half));
    TRY(ensure(c, c->out, 2 * half));
    TRY(ensure(c, c->lk_status, 4 * count));
    enum { STAGE, SORT, RANK, PHASES };   // of h2agg_last_phases (debug key phases)
    static const char* const names[PHASES] = {"stage", "sort", "rank"};
    PhaseClock phases(c);
    phases.mark(STAGE);
    uint8_t* d_in = (uint8_t*)c->in_a.p;
    uint8_t* d_out = (uint8_t*)c->out.p;
    uint32_t* d_status = (uint32_t*)c->lk_status.p;
    TRY(lk_copy_rows(c, d_in, ds, a, col, u, count, hipMemcpyHostToDevice));
    TRY(lk_copy_rows(c, d_in + half, ds, s, col, u, count, hipMemcpyHostToDevice));
    TRY(clear_flags(c));
    TRY(lk_batch_permute_queue(c, d_in, d_in + half, ds, count, u, d_out, d_out + half, d_status, &phases, SORT));
    phases.mark(STAGE);
    TRY(lk_copy_rows(c, ap, col, d_out, ds, u, count, hipMemcpyDeviceToHost));
    TRY(lk_copy_rows(c, sp, col, d_out + half, ds, u, count, hipMemcpyDeviceToHost));
    phases.mark(PhaseClock::END);
    const int rc = lk_batch_finish(c, d_status, count, status);
    phases.report(names, PHASES);
    return rc;
} API_CATCH

int h2agg_lookup_batch_product(h2agg_ctx* c, const uint8_t* a, const uint8_t* s, const uint8_t* ap, const uint8_t* sp, size_t count,
                               unsigned k, size_t u, const uint8_t beta[32], const uint8_t gamma[32], uint8_t* z, uint8_t* last) try {
    TRY(bind(c));
    if (c->dbg_phases) c->last_phases.clear();
    TRY(lk_batch_check(c, count, k, u));
    ph::HFr bf, gf;
    TRY(lookup_check(c, k, u, beta, gamma, &bf, &gf));
    if (!a || !s || !ap || !sp || !z) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    const size_t col = (size_t)32 << k, slab = count * col;
    if (lk_overlap(z, a, slab) || lk_overlap(z, s, slab) || lk_overlap(z, ap, slab) || lk_overlap(z, sp, slab))
        return fail(c, H2AGG_ERR_INVALID, "z must not overlap a, s, ap or sp");
    const size_t ds = 32 * u, quarter = count * ds, zs = 32 * (u + 1);   // dense device twins: [count][u], z [count][u + 1]
    TRY(ensure(c, c->in_a, 4 * quarter + 32));
    TRY(ensure(c, c->out, count * zs));
    enum { STAGE, TERMS, INVERT, SCAN, PHASES };   // of h2agg_last_phases (debug key phases)
    static const char* const names[PHASES] = {"stage", "terms", "invert", "scan"};
    PhaseClock phases(c);
    phases.mark(STAGE);
    uint8_t* d = (uint8_t*)c->in_a.p;
    uint8_t* d_z = (uint8_t*)c->out.p;
    const uint8_t* cols[4] = {a, s, ap, sp};
    for (int i = 0; i < 4; ++i) TRY(lk_copy_rows(c, d + i * quarter, ds, cols[i], col, u, count, hipMemcpyHostToDevice));
    TRY(clear_flags(c));
    TRY(lk_batch_product_queue(c, d, d + quarter, d + 2 * quarter, d + 3 * quarter, ds, count, u, bf, gf, d_z, zs, &phases, TERMS));
    phases.mark(STAGE);
    TRY(lk_copy_rows(c, z, col, d_z, zs, u + 1, count, hipMemcpyDeviceToHost));
    phases.mark(PhaseClock::END);
    const int rc = finish(c);
    phases.report(names, PHASES);
    if (rc != H2AGG_OK) return rc;
    if (last)
        for (size_t j = 0; j < count; ++j) memcpy(last + 32 * j, z + j * col + 32 * u, 32);
    return H2AGG_OK;
} API_CATCH

int h2agg_lookup_permute_device(h2agg_ctx* c, const void* d_a, const void* d_s, unsigned k, size_t u, void* d_ap, void* d_sp) try {
    TRY(bind(c));
    TRY(prod_check_ku(c, k, u));
    if (!d_a || !d_s || !d_ap || !d_sp) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    if (u == 0) return H2AGG_OK;
    const size_t bytes = 32 * u;
    if (lk_overlap(d_ap, d_a, bytes) || lk_overlap(d_ap, d_s, bytes) || lk_overlap(d_sp, d_a, bytes) || lk_overlap(d_sp, d_s, bytes) ||
        lk_overlap(d_ap, d_sp, bytes))
        return fail(c, H2AGG_ERR_INVALID, "ap / sp must not overlap a, s or each other");
    return lk_permute_queue(c, (const uint8_t*)d_a, (const uint8_t*)d_s, 0, 1, u, (uint8_t*)d_ap, (uint8_t*)d_sp, nullptr);
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
    TRY(lk_permute_queue(c, d_in, d_in + bytes, 0, 1, u, d_out, d_out + bytes, nullptr));
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
