// Grand products, host side (included into h2agg.hip: shares the context internals; kernels and bounds in prod_kernels.hpp,
// level plan and checks in fr_host.inc, staging in host.inc, power tables in fr_fft.inc): h2agg_fr_batch_invert[_device],
// h2agg_fr_grand_product[_device], h2agg_permutation_product[_device], h2agg_lookup_product[_device].  They stand for
// halo2_proofs' ff::BatchInvert, permutation::prover::commit and lookup::prover::commit_product — an unvendored git dependency
// of the reference, recalled from upstream (DESIGN.md section 2); the yardstick is the definition in include/h2agg.h.  Which
// Z a verifier accepts is pinned by halo2-snark-aggregator-api/src/systems/halo2/permutation.rs:70-133 and lookup.rs:98-113.

namespace {

constexpr size_t PROD_MAX_N = (size_t)1 << FFT_MAX_K;

// the levels of one sweep pair over n elements, in the context's level buffer.  (The last level, one element, is never stored:
// the top chunk keeps its root.)  nq > 1: a batch of nq running products of n positions each, level l >= 1 is [nq][cnt[l]] at off[l]
FrLevelPlan prod_plan(const h2agg_ctx* c, size_t n, size_t nq = 1) {
    return fr_level_plan(c->dbg_fr_scan_chunk ? (unsigned)c->dbg_fr_scan_chunk : FR_CHUNK_LOG, n, nq);
}

// Queues both sweeps of `op` over n >= 1 elements (scan: n = u + 1 positions): up-sweeps of the levels below the top one, then
// the down-sweeps from the top.  The level buffer must hold prod_plan(c, n, nq).total elements.  nq > 1 (scan only): nq columns
// in the second grid dimension — column y of src and aux at + y src_stride bytes, of dst at + y dst_stride — with the launch
// count of one column.
void prod_sweeps_queue(h2agg_ctx* c, uint32_t op, const uint8_t* d_src, const uint8_t* d_aux, size_t n, const ph::HFr& top,
                       bool check, uint8_t* d_dst, size_t nq = 1, size_t src_stride = 0, size_t dst_stride = 0) {
    const FrLevelPlan plan = prod_plan(c, n, nq);
    uint8_t* lvl = (uint8_t*)c->prod_lvl.p;
    const size_t L = plan.launches();
    const unsigned ny = (unsigned)nq;
    FrProdArgs a;
    hfr_words(top, a.top);
    a.aux = d_aux;
    a.aux_stride = src_stride;
    a.flags = c->d_flags;
    a.t = plan.t;
    a.op = op;
    a.check = check;
    for (size_t l = 0; l + 1 < L; ++l) {
        a.src = l == 0 ? d_src : lvl + 32 * plan.off[l];
        a.src_stride = l == 0 ? src_stride : 32 * (size_t)plan.cnt[l];
        a.dst = lvl + 32 * plan.off[l + 1];
        a.dst_stride = 32 * (size_t)plan.cnt[l + 1];
        a.carry = nullptr;
        a.carry_stride = 0;
        a.n = plan.cnt[l];
        a.level0 = l == 0;
        hipLaunchKernelGGL(k_fr_prod_chunk, dim3(plan.cnt[l + 1], ny), dim3(FR_CHUNK_THREADS), 0, c->stream, a);
    }
    for (size_t l = L; l-- > 0;) {
        a.src = l == 0 ? d_src : lvl + 32 * plan.off[l];
        a.src_stride = l == 0 ? src_stride : 32 * (size_t)plan.cnt[l];
        a.dst = l == 0 ? d_dst : lvl + 32 * plan.off[l];
        a.dst_stride = l == 0 ? dst_stride : 32 * (size_t)plan.cnt[l];
        a.carry = l + 1 == L ? nullptr : lvl + 32 * plan.off[l + 1];
        a.carry_stride = 32 * (size_t)plan.cnt[l + 1];
        a.n = plan.cnt[l];
        a.level0 = l == 0;
        if (op == FR_PROD_INVERT)
            hipLaunchKernelGGL(k_fr_prod_invert, dim3(plan.cnt[l + 1]), dim3(FR_CHUNK_THREADS), 0, c->stream, a);
        else
            hipLaunchKernelGGL(k_fr_prod_scan, dim3(plan.cnt[l + 1], ny), dim3(FR_CHUNK_THREADS), 0, c->stream, a);
    }
}

int prod_ensure_levels(h2agg_ctx* c, size_t n, size_t nq = 1) { return ensure(c, c->prod_lvl, 32 * prod_plan(c, n, nq).total); }

// out[i] = 1 / in[i] (montgomery2 = false) or R^2 / in[i] (true: what the scan multiplies num with), 0 for 0; n >= 1
int prod_invert_queue(h2agg_ctx* c, const uint8_t* d_in, size_t n, bool montgomery2, bool check, uint8_t* d_out) {
    TRY(prod_ensure_levels(c, n));
    prod_sweeps_queue(c, FR_PROD_INVERT, d_in, nullptr, n, montgomery2 ? fr_radix() : ph::inv(fr_radix()), check, d_out);
    HIP_TRY(c, hipGetLastError());
    return H2AGG_OK;
}

// out[0] = init, out[i + 1] = out[i] * num[i] / den[i], i < u; d_den null: no denominator.  Nothing synchronises unless a
// workspace has to grow.  check: num and den are the caller's.
int prod_grand_queue(h2agg_ctx* c, const uint8_t* d_num, const uint8_t* d_den, size_t u, const ph::HFr& init, bool check,
                     uint8_t* d_out, uint8_t* d_last) {
    const uint8_t* d_aux = nullptr;
    if (d_den && u) {
        uint8_t* inv = (uint8_t*)c->prod_den.p;
        if (d_den != inv) {
            TRY(ensure(c, c->prod_den, 32 * u));
            inv = (uint8_t*)c->prod_den.p;
        }
        TRY(prod_invert_queue(c, d_den, u, true, check, inv));
        d_aux = inv;
    }
    TRY(prod_ensure_levels(c, u + 1));
    prod_sweeps_queue(c, FR_PROD_SCAN, d_num, d_aux, u + 1, init, check, d_out);
    HIP_TRY(c, hipGetLastError());
    if (d_last) HIP_TRY(c, hipMemcpyAsync(d_last, d_out + 32 * u, 32, hipMemcpyDeviceToDevice, c->stream));
    return H2AGG_OK;
}

int prod_check_ku(h2agg_ctx* c, unsigned k, size_t u) {
    TRY(fr_check_k(c, k));
    if (u >= ((size_t)1 << k)) return fail(c, H2AGG_ERR_INVALID, "u must be < 2^k");
    return H2AGG_OK;
}

struct PermConsts {
    ph::HFr beta, gamma, delta, delta_first, init;
};

int perm_check(h2agg_ctx* c, size_t m, unsigned k, size_t u, const uint8_t* beta, const uint8_t* gamma, const uint8_t* delta,
               const uint8_t* delta_first, const uint8_t* init, PermConsts* pc) {
    TRY(prod_check_ku(c, k, u));
    if (m == 0 || m > FR_PROD_MAX_COLUMNS) return fail(c, H2AGG_ERR_INVALID, "m must be 1 .. 16");
    if (!beta || !gamma || !delta || !delta_first || !init) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(fr_parse(c, beta, &pc->beta));
    TRY(fr_parse(c, gamma, &pc->gamma));
    TRY(fr_parse(c, delta, &pc->delta));
    TRY(fr_parse(c, delta_first, &pc->delta_first));
    return fr_parse(c, init, &pc->init);
}

// the term kernel into the context's num / den columns, then the grand product of the two
int perm_queue(h2agg_ctx* c, const uint8_t* d_values, const uint8_t* d_sigmas, size_t m, unsigned k, size_t u, const PermConsts& pc,
               uint8_t* d_out, uint8_t* d_last) {
    if (u) {
        TRY(ensure(c, c->prod_num, 32 * u));
        TRY(ensure(c, c->prod_den, 32 * u));
        TRY(ensure(c, c->prod_tab, fr_table_bytes(k)));
        fr_table_launch(c, fft_omega(k), k, (uint8_t*)c->prod_tab.p);
        FrPermArgs a;
        hfr_words(ph::mul(pc.beta, fr_radix()), a.beta);
        hfr_words(pc.gamma, a.gamma);
        ph::HFr rm = ph::one(), bd = ph::mul(pc.beta, pc.delta_first);
        memset(a.bd, 0, sizeof(a.bd));
        for (size_t j = 0; j < m; ++j) {
            rm = ph::mul(rm, fr_radix());
            hfr_words(bd, a.bd[j]);
            bd = ph::mul(bd, pc.delta);
        }
        hfr_words(rm, a.rm);
        a.values = d_values;
        a.sigmas = d_sigmas;
        a.num = (uint8_t*)c->prod_num.p;
        a.den = (uint8_t*)c->prod_den.p;
        a.wT = fr_table_split(k);
        a.w_lo = (const uint8_t*)c->prod_tab.p;
        a.w_hi = a.w_lo + ((size_t)32 << a.wT);
        a.flags = c->d_flags;
        a.n = 1u << k;
        a.u = (uint32_t)u;
        a.m = (uint32_t)m;
        hipLaunchKernelGGL(k_fr_perm_terms, dim3((unsigned)((u + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream, a);
    }
    return prod_grand_queue(c, (const uint8_t*)c->prod_num.p, (const uint8_t*)c->prod_den.p, u, pc.init, false, d_out, d_last);
}

int lookup_check(h2agg_ctx* c, unsigned k, size_t u, const uint8_t* beta, const uint8_t* gamma, ph::HFr* bf, ph::HFr* gf) {
    TRY(prod_check_ku(c, k, u));
    if (!beta || !gamma) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(fr_parse(c, beta, bf));
    return fr_parse(c, gamma, gf);
}

// The Z columns of a chunk of nb lookups over u rows each, nb u <= 2^24: lookup y reads column y of the four slabs (col_stride
// bytes apart) and writes z[0 .. u] of column y of d_out (out_stride apart).  One term launch into num / den [nb][u], ONE
// inversion of the nb u denominators, one pair of sweeps with the lookups in the second grid dimension: the launch count of
// one lookup.  phases (or null) is marked with first, first + 1, first + 2 in front of the terms, the inversion and the scan.
int lookup_chunk_queue(h2agg_ctx* c, const uint8_t* d_a, const uint8_t* d_s, const uint8_t* d_ap, const uint8_t* d_sp,
                       size_t col_stride, size_t nb, size_t u, const ph::HFr& beta, const ph::HFr& gamma, uint8_t* d_out,
                       size_t out_stride, PhaseClock* phases = nullptr, int first = 0) {
    if (u) {
        TRY(ensure(c, c->prod_num, 32 * nb * u));
        TRY(ensure(c, c->prod_den, 32 * nb * u));
    }
    uint8_t* num = (uint8_t*)c->prod_num.p;
    uint8_t* den = (uint8_t*)c->prod_den.p;
    if (phases) phases->mark(first);
    if (u) {
        FrLookupArgs a;
        hfr_words(beta, a.beta);
        hfr_words(gamma, a.gamma);
        a.a = d_a;
        a.s = d_s;
        a.ap = d_ap;
        a.sp = d_sp;
        a.num = num;
        a.den = den;
        a.flags = c->d_flags;
        a.col_stride = col_stride;
        a.u = (uint32_t)u;
        hipLaunchKernelGGL(k_fr_lookup_terms, dim3((unsigned)((u + BLOCK - 1) / BLOCK), (unsigned)nb), dim3(BLOCK), 0, c->stream, a);
        if (phases) phases->mark(first + 1);
        TRY(prod_invert_queue(c, den, nb * u, true, false, den));   // in place: R^2 / den
    }
    TRY(prod_ensure_levels(c, u + 1, nb));
    if (phases) phases->mark(first + 2);
    prod_sweeps_queue(c, FR_PROD_SCAN, num, u ? den : nullptr, u + 1, ph::one(), false, d_out, nb, 32 * u, out_stride);
    HIP_TRY(c, hipGetLastError());
    return H2AGG_OK;
}

int lookup_queue(h2agg_ctx* c, const uint8_t* d_a, const uint8_t* d_s, const uint8_t* d_ap, const uint8_t* d_sp, size_t u,
                 const ph::HFr& beta, const ph::HFr& gamma, uint8_t* d_out, uint8_t* d_last) {
    TRY(lookup_chunk_queue(c, d_a, d_s, d_ap, d_sp, 0, 1, u, beta, gamma, d_out, 0));
    if (d_last) HIP_TRY(c, hipMemcpyAsync(d_last, d_out + 32 * u, 32, hipMemcpyDeviceToDevice, c->stream));
    return H2AGG_OK;
}

// the tail of every synchronous product call: out[0 .. u] and `last` back to the host
int prod_download(h2agg_ctx* c, size_t u, uint8_t* out, uint8_t* last) {
    TRY(stage_out(c, out, c->out.p, 32 * (u + 1)));
    if (last) memcpy(last, out + 32 * u, 32);
    return H2AGG_OK;
}

}  // namespace

extern "C" {

int h2agg_fr_batch_invert_device(h2agg_ctx* c, const void* d_in, size_t n, void* d_out) try {
    TRY(bind(c));
    if (n > PROD_MAX_N) return fail(c, H2AGG_ERR_INVALID, "n must be <= 2^24");
    if (n == 0) return H2AGG_OK;
    if (!d_in || !d_out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    return prod_invert_queue(c, (const uint8_t*)d_in, n, false, true, (uint8_t*)d_out);
} API_CATCH

int h2agg_fr_batch_invert(h2agg_ctx* c, const uint8_t* in, size_t n, uint8_t* out) try {
    TRY(bind(c));
    if (n > PROD_MAX_N) return fail(c, H2AGG_ERR_INVALID, "n must be <= 2^24");
    if (n == 0) return H2AGG_OK;
    if (!in || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_a, 32 * n));
    TRY(stage_in(c, c->in_a, in, 32 * n));
    TRY(clear_flags(c));
    TRY(prod_invert_queue(c, (const uint8_t*)c->in_a.p, n, false, true, (uint8_t*)c->in_a.p));
    return stage_out(c, out, c->in_a.p, 32 * n);
} API_CATCH

int h2agg_fr_grand_product_device(h2agg_ctx* c, const void* d_num, const void* d_den, unsigned k, size_t u, const uint8_t init[32],
                                  void* d_out, void* d_last) try {
    TRY(bind(c));
    TRY(prod_check_ku(c, k, u));
    if (!d_num || !d_out || !init) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    ph::HFr initf;
    TRY(fr_parse(c, init, &initf));
    return prod_grand_queue(c, (const uint8_t*)d_num, (const uint8_t*)d_den, u, initf, true, (uint8_t*)d_out, (uint8_t*)d_last);
} API_CATCH

int h2agg_fr_grand_product(h2agg_ctx* c, const uint8_t* num, const uint8_t* den, unsigned k, size_t u, const uint8_t init[32],
                           uint8_t* out, uint8_t last[32]) try {
    TRY(bind(c));
    TRY(prod_check_ku(c, k, u));
    if (!num || !out || !init) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    ph::HFr initf;
    TRY(fr_parse(c, init, &initf));
    TRY(ensure(c, c->in_a, 32 * u + 32));
    TRY(ensure(c, c->in_b, 32 * u + 32));
    TRY(ensure(c, c->out, 32 * (u + 1)));
    TRY(stage_in(c, c->in_a, num, 32 * u));
    if (den) TRY(stage_in(c, c->in_b, den, 32 * u));
    TRY(clear_flags(c));
    TRY(prod_grand_queue(c, (const uint8_t*)c->in_a.p, den ? (const uint8_t*)c->in_b.p : nullptr, u, initf, true,
                         (uint8_t*)c->out.p, nullptr));
    return prod_download(c, u, out, last);
} API_CATCH

int h2agg_permutation_product_device(h2agg_ctx* c, const void* d_values, const void* d_sigmas, size_t m, unsigned k, size_t u,
                                     const uint8_t beta[32], const uint8_t gamma[32], const uint8_t delta[32],
                                     const uint8_t delta_first[32], const uint8_t init[32], void* d_out, void* d_last) try {
    TRY(bind(c));
    PermConsts pc;
    TRY(perm_check(c, m, k, u, beta, gamma, delta, delta_first, init, &pc));
    if (!d_values || !d_sigmas || !d_out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    return perm_queue(c, (const uint8_t*)d_values, (const uint8_t*)d_sigmas, m, k, u, pc, (uint8_t*)d_out, (uint8_t*)d_last);
} API_CATCH

int h2agg_permutation_product(h2agg_ctx* c, const uint8_t* values, const uint8_t* sigmas, size_t m, unsigned k, size_t u,
                              const uint8_t beta[32], const uint8_t gamma[32], const uint8_t delta[32],
                              const uint8_t delta_first[32], const uint8_t init[32], uint8_t* out, uint8_t last[32]) try {
    TRY(bind(c));
    PermConsts pc;
    TRY(perm_check(c, m, k, u, beta, gamma, delta, delta_first, init, &pc));
    if (!values || !sigmas || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    const size_t bytes = ((size_t)32 << k) * m;
    TRY(ensure(c, c->in_a, bytes));
    TRY(ensure(c, c->in_b, bytes));
    TRY(ensure(c, c->out, 32 * (u + 1)));
    TRY(stage_in(c, c->in_a, values, bytes));
    TRY(stage_in(c, c->in_b, sigmas, bytes));
    TRY(clear_flags(c));
    TRY(perm_queue(c, (const uint8_t*)c->in_a.p, (const uint8_t*)c->in_b.p, m, k, u, pc, (uint8_t*)c->out.p, nullptr));
    return prod_download(c, u, out, last);
} API_CATCH

int h2agg_lookup_product_device(h2agg_ctx* c, const void* d_a, const void* d_s, const void* d_ap, const void* d_sp, unsigned k,
                                size_t u, const uint8_t beta[32], const uint8_t gamma[32], void* d_out, void* d_last) try {
    TRY(bind(c));
    ph::HFr bf, gf;
    TRY(lookup_check(c, k, u, beta, gamma, &bf, &gf));
    if (!d_a || !d_s || !d_ap || !d_sp || !d_out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    return lookup_queue(c, (const uint8_t*)d_a, (const uint8_t*)d_s, (const uint8_t*)d_ap, (const uint8_t*)d_sp, u, bf, gf,
                        (uint8_t*)d_out, (uint8_t*)d_last);
} API_CATCH

int h2agg_lookup_product(h2agg_ctx* c, const uint8_t* a, const uint8_t* s, const uint8_t* ap, const uint8_t* sp, unsigned k, size_t u,
                         const uint8_t beta[32], const uint8_t gamma[32], uint8_t* out, uint8_t last[32]) try {
    TRY(bind(c));
    ph::HFr bf, gf;
    TRY(lookup_check(c, k, u, beta, gamma, &bf, &gf));
    if (!a || !s || !ap || !sp || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    const size_t col = (size_t)32 << k;
    TRY(ensure(c, c->in_a, 4 * col));
    TRY(ensure(c, c->out, 32 * (u + 1)));
    const uint8_t* cols[4] = {a, s, ap, sp};
    for (int i = 0; i < 4; ++i) TRY(stage_in(c, c->in_a, cols[i], 32 * u, i * col));
    TRY(clear_flags(c));
    const uint8_t* d = (const uint8_t*)c->in_a.p;
    TRY(lookup_queue(c, d, d + col, d + 2 * col, d + 3 * col, u, bf, gf, (uint8_t*)c->out.p, nullptr));
    return prod_download(c, u, out, last);
} API_CATCH

}  // extern "C"
