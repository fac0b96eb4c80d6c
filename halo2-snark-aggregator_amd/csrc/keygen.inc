// The permutation half of keygen and the slab commit, host side (included into h2agg.hip behind quotient.inc: shares the
// context internals; the kernel and its bounds in keygen_kernels.hpp, checks in fr_host.inc, staging in host.inc, transforms and power
// tables in fr_fft.inc): h2agg_permutation_assembly, h2agg_permutation_sigmas, h2agg_commit_columns.  They stand for
// halo2_proofs' permutation::keygen::Assembly (copy, build_vk, build_pk) and the commit_lagrange loop of keygen_vk — an
// unvendored git dependency of the reference, recalled from upstream (DESIGN.md section 2 and 5.15); the yardstick is the
// definition in include/h2agg.h.
//
// There is no _device twin: the resident forms run over column stores (h2agg_columns_sigmas, h2agg_columns_commit in
// csrc/columns.inc, DESIGN.md 5.20), on top of perm_sigma_queue and commit_columns_run below.

namespace {

static_assert(PERM_MAX_COLUMNS == H2AGG_PERM_MAX_COLUMNS, "the header states the limit the kernel supports");

constexpr unsigned KG_COMMIT_WORK_LOG = 22;   // scalars of one set of MSM launches of h2agg_commit_columns: at most 2^22, or one column

// m, k, usable -> refusals shared by the assembly and the sigma columns (c may be null: the assembly has no context)
int perm_check_shape(h2agg_ctx* c, size_t m, unsigned k, size_t usable) {
    if (k > FFT_MAX_K) return fail(c, H2AGG_ERR_INVALID, "k must be <= 24");
    if (m == 0 || m > PERM_MAX_COLUMNS) return fail(c, H2AGG_ERR_INVALID, "permutation: m must be 1 .. 4096");
    if (usable > (size_t)1 << k) return fail(c, H2AGG_ERR_INVALID, "permutation: usable > 2^k");
    return H2AGG_OK;
}

// Queues the sigma columns of the mapping at d_mapping ([m * n] pairs) into the slab d_out[m][n], canonical: the bitmap's
// clear, the delta table, k_perm_sigma.  Nothing synchronises unless a workspace has to grow.  An invalid mapping raises
// FLAG_BAD_MAPPING in the context's device status.
int perm_sigma_queue(h2agg_ctx* c, const void* d_mapping, size_t m, unsigned k, size_t usable, const ph::HFr& delta, uint8_t* d_out) {
    const size_t cells = m << k;
    const size_t bitmap_bytes = 4 * ((cells + 31) / 32);
    TRY(ensure(c, c->kg_bitmap, bitmap_bytes));
    TRY(ensure(c, c->kg_delta, 32 * m));
    if (k) TRY(fr_fft_ensure_twiddles(c, k, 0));
    HIP_TRY(c, hipMemsetAsync(c->kg_bitmap.p, 0, bitmap_bytes, c->stream));
    fr_powers_launch(c, delta, (uint32_t)m, (uint8_t*)c->kg_delta.p, true);   // plain integers: see k_perm_sigma
    PermSigmaArgs a;
    const unsigned K = k ? (unsigned)c->frfft_tw_k[0] : 0;
    a.mapping = (const uint2*)d_mapping;
    a.out = d_out;
    a.bitmap = (uint32_t*)c->kg_bitmap.p;
    a.flags = c->d_flags;
    a.tw_T = fr_table_split(K);
    a.tw_lo = k ? (const uint8_t*)c->frfft_tw[0].p : nullptr;   // (k == 0: the one row is r == 0, which reads no twiddle)
    a.tw_hi = k ? a.tw_lo + ((size_t)32 << a.tw_T) : nullptr;
    a.tw_up = K - k;
    a.delta = (const uint8_t*)c->kg_delta.p;
    a.cells = cells;
    a.m = (uint32_t)m;
    a.k = k;
    a.usable = (uint32_t)usable;
    hipLaunchKernelGGL(k_perm_sigma, dim3(grid_for(c, cells)), dim3(BLOCK), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    return H2AGG_OK;
}

// The commitments of the slab d_cols[m][2^k] in device memory against a table that holds 2^k points or more, as canonical
// affine points to the host: what h2agg_commit_columns runs behind its staging and h2agg_columns_commit over a store.
int commit_columns_run(h2agg_ctx* c, uint64_t bases_handle, const uint8_t* d_cols, size_t m, unsigned k, uint8_t* out_aff) {
    const size_t n = (size_t)1 << k;
    TRY(ensure(c, c->kg_jac, 96 * m));
    TRY(clear_flags(c));
    // B columns per set of MSM launches: as many as hold 2^KG_COMMIT_WORK_LOG scalars (the sort's and the buckets' work memory
    // grows with the scalars in flight), at least one, or the debug key commit_chunk; the batched MSM cuts further by its own limits
    size_t B = std::max<size_t>(1, ((size_t)1 << KG_COMMIT_WORK_LOG) >> k);
    if (c->dbg_commit_chunk) B = (size_t)c->dbg_commit_chunk;
    for (size_t q = 0; q < m; q += B)
        TRY(h2agg_g1_msm_device_batch_async(c, bases_handle, d_cols + 32 * n * q, n, std::min(B, m - q), (uint8_t*)c->kg_jac.p + 96 * q));
    return h2agg_g1_batch_to_affine_device(c, (const uint8_t*)c->kg_jac.p, m, out_aff);   // joins, synchronises, reports the flags
}

}  // namespace

extern "C" {

int h2agg_permutation_assembly(size_t m, unsigned k, size_t usable, const uint32_t* copies, size_t ncopies, uint32_t* mapping) try {
    TRY(perm_check_shape(nullptr, m, k, usable));
    if (!mapping || (ncopies && !copies)) return H2AGG_ERR_INVALID;
    const size_t n = (size_t)1 << k, cells = m * n;
    for (size_t q = 0; q < ncopies; ++q) {   // every refusal before the first write
        const uint32_t* cp = copies + 4 * q;
        if (cp[0] >= m || cp[2] >= m || cp[1] >= usable || cp[3] >= usable) return H2AGG_ERR_INVALID;
    }
    // Assembly::new: every cell maps to itself, is its own cycle's representative, and that cycle has one cell.  Cells are
    // indices j * n + i here; `next` is the mapping.
    std::vector<uint64_t> next(cells), aux(cells), sizes(cells, 1);
    for (size_t x = 0; x < cells; ++x) next[x] = aux[x] = x;
    for (size_t q = 0; q < ncopies; ++q) {   // Assembly::copy
        const uint32_t* cp = copies + 4 * q;
        const uint64_t left = (uint64_t)cp[0] * n + cp[1], right = (uint64_t)cp[2] * n + cp[3];
        uint64_t lc = aux[left], rc = aux[right];
        if (lc == rc) continue;                        // a copy within one cycle
        if (sizes[lc] < sizes[rc]) std::swap(lc, rc);  // the smaller cycle is merged; on a tie the right one
        sizes[lc] += sizes[rc];
        uint64_t x = rc;
        do {
            aux[x] = lc;
            x = next[x];
        } while (x != rc);
        std::swap(next[left], next[right]);
    }
    for (size_t x = 0; x < cells; ++x) {
        mapping[2 * x] = (uint32_t)(next[x] >> k);
        mapping[2 * x + 1] = (uint32_t)(next[x] & (n - 1));
    }
    return H2AGG_OK;
} API_CATCH

int h2agg_permutation_sigmas(h2agg_ctx* c, const uint32_t* mapping, size_t m, unsigned k, size_t usable, const uint8_t delta[32],
                             uint8_t* sigma_lagrange, uint8_t* sigma_coeff) try {
    TRY(bind(c));
    if (c->dbg_phases) c->last_phases.clear();
    TRY(perm_check_shape(c, m, k, usable));
    if (!mapping || !delta || (!sigma_lagrange && !sigma_coeff)) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    ph::HFr d;
    TRY(fr_parse(c, delta, &d));
    const size_t n = (size_t)1 << k, cells = m * n, slab = 32 * cells;
    // the range of every entry, on the host: one pass over memory the copy is about to read.  An out-of-range entry never
    // reaches the device through this entry point (the kernel's own guard is the resident twin's).
    for (size_t x = 0; x < cells; ++x)
        if (mapping[2 * x] >= m || mapping[2 * x + 1] >= n)
            return fail(c, H2AGG_ERR_INVALID, "permutation_sigmas: a mapping entry is outside the m x 2^k cells");
    const bool both = sigma_lagrange && sigma_coeff;
    TRY(ensure(c, c->in_a, 8 * cells));
    TRY(ensure(c, c->out, slab));
    if (both) TRY(ensure(c, c->in_b, slab));
    uint8_t* d_lag = (uint8_t*)c->out.p;
    uint8_t* d_coeff = both ? (uint8_t*)c->in_b.p : d_lag;   // only the coefficients are wanted: the transform runs in place
    // debug key phases: only the phases that finished are named (a refused mapping has no copy)
    enum { STAGE, SIGMA, INVERSE, COPY, PHASES };
    static const char* const names[PHASES] = {"stage", "sigma", "inverse", "copy"};
    PhaseClock phases(c);
    phases.mark(STAGE);
    TRY(stage_in(c, c->in_a, (const uint8_t*)mapping, 8 * cells));
    TRY(clear_flags(c));
    phases.mark(SIGMA);
    TRY(perm_sigma_queue(c, c->in_a.p, m, k, usable, d, d_lag));
    phases.mark(INVERSE);
    if (sigma_coeff) {
        const FrFftSeg seg = {d_lag, m};
        TRY(fr_fft_queue_batch(c, &seg, 1, m, k, 1, nullptr, d_coeff));
    }
    phases.mark(COPY);
    // the verdict first: on a refusal nothing is written to the outputs
    const int rc = finish(c);
    if (rc != H2AGG_OK) {
        phases.report(names, PHASES, true);
        return rc;
    }
    if (sigma_lagrange) HIP_TRY(c, hipMemcpyAsync(sigma_lagrange, d_lag, slab, hipMemcpyDeviceToHost, c->stream));
    if (sigma_coeff) HIP_TRY(c, hipMemcpyAsync(sigma_coeff, d_coeff, slab, hipMemcpyDeviceToHost, c->stream));
    phases.mark(PhaseClock::END);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    phases.report(names, PHASES, true);
    return H2AGG_OK;
} API_CATCH

int h2agg_commit_columns(h2agg_ctx* c, uint64_t bases_handle, const uint8_t* columns, size_t m, unsigned k, uint8_t* out_aff) try {
    TRY(bind(c));
    if (!columns || !out_aff) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    if (m == 0) return fail(c, H2AGG_ERR_INVALID, "commit_columns: m == 0");
    TRY(fr_check_k(c, k));
    const size_t n = (size_t)1 << k;
    Table* bases = nullptr;
    TRY(find_table(c, bases_handle, &bases));
    if (n > bases->n) return fail(c, H2AGG_ERR_INVALID, "commit_columns: the table is shorter than 2^k");
    if (m > (SIZE_MAX >> 1) / (32 * n)) return fail(c, H2AGG_ERR_NOMEM, "commit_columns: the slab does not fit the address space");
    TRY(ensure(c, c->in_b, 32 * n * m));
    TRY(ensure(c, c->kg_jac, 96 * m));
    TRY(stage_in(c, c->in_b, columns, 32 * n * m));   // one staging of the slab
    return commit_columns_run(c, bases_handle, (const uint8_t*)c->in_b.p, m, k, out_aff);
} API_CATCH

}  // extern "C"
