// The proving key as a device object, host side (included into h2agg.hip behind keygen.inc: shares the context internals, the
// quotient's layout and queue function — quotient.inc — and the batched transforms of fr_fft.inc; the kernels are the
// quotient's, quotient_kernels.hpp; checks in fr_host.inc, staging and allocation in host.inc): h2agg_pk_create /
// _create_resident / _bytes / _info / _ptr / _quotient / _quotient_work_bytes / _destroy.
// They stand for what halo2_proofs' ProvingKey caches between proofs of one circuit — fixed_values / fixed_polys /
// fixed_cosets, the permutation's permutations / polys / cosets, l0, l_last, l_active_row — an unvendored git dependency of
// the reference, recalled from upstream (DESIGN.md section 2); the yardstick is the definition in include/h2agg.h: every form is
// byte for byte what the transform entry points give for it, and h2agg_pk_quotient writes what h2agg_quotient_device writes.
//
// Nothing here computes: create is stage + fr_fft_queue_batch + k_qe_lagrange_rows, the quotient is qt_queue with the key's
// forms lent to it (DESIGN.md 5.22).

// The forms, each one exact allocation.  It refers to its context and its verifying key, which must outlive it.
struct h2agg_pk {
    h2agg_ctx* ctx = nullptr;
    const h2agg_vk* vk = nullptr;
    int device = 0;
    unsigned k = 0, e = 0, forms = 0;
    uint32_t F = 0, P = 0;
    DevMem lagrange;   // [F + P][n]: fixed, then sigma, as given
    DevMem coeff;      // [F + P + 3][n]: their coefficient forms, then those of l_0, l_last, l_blind
    DevMem cosets;     // H2AGG_PK_COSETS: [2^e][F + P + 3][n], slab c' = the values of `coeff` on {zeta w_ext^c' w^i}
    size_t col() const { return (size_t)32 << k; }
    size_t key_cols() const { return (size_t)F + P + 3; }
};

namespace {

// 32 (2 (F + P) n + 3 n + [COSETS] (F + P + 3) n 2^e): include/h2agg.h
size_t pk_bytes(const QtLayout& l, unsigned k, unsigned forms) {
    const size_t n = (size_t)1 << k, fp = (size_t)l.F + l.P;
    return 32 * (2 * fp * n + 3 * n + (forms & H2AGG_PK_COSETS ? ((fp + 3) * n) << l.e : 0));
}

QtKeyMode pk_mode(unsigned forms) { return forms & H2AGG_PK_COSETS ? QT_PK_COSETS : QT_PK; }

// Everything behind the copy of the two slabs into o->lagrange: the forms, then the verdict of the device.  Synchronous.
int pk_build(h2agg_ctx* c, h2agg_pk* o) {
    const unsigned k = o->k;
    const size_t n = (size_t)1 << k, col = o->col(), fp = (size_t)o->F + o->P;
    uint8_t* lcoef = o->coeff + fp * col;
    if (fp) {
        const FrFftSeg seg = {o->lagrange, fp};
        TRY(fr_fft_queue_batch(c, &seg, 1, fp, k, 1, nullptr, o->coeff));
    }
    const uint32_t u = (uint32_t)n - o->vk->blinding_factors - 1u;
    hipLaunchKernelGGL(k_qe_lagrange_rows, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream, lcoef, (uint32_t)n, u);
    {
        const FrFftSeg rows3 = {lcoef, 3};
        TRY(fr_fft_queue_batch(c, &rows3, 1, 3, k, 1, nullptr, lcoef));
    }
    if (o->forms & H2AGG_PK_COSETS) {
        const FrFftSeg seg = {o->coeff, fp + 3};
        const ph::HFr w_ext = fft_omega(k + o->e);
        ph::HFr s = qt_zeta();
        for (uint32_t cs = 0; cs < (1u << o->e); ++cs, s = ph::mul(s, w_ext))
            TRY(fr_fft_queue_batch(c, &seg, 1, fp + 3, k, 0, &s, o->cosets + cs * (fp + 3) * col));
    }
    HIP_TRY(c, hipGetLastError());
    return finish(c);
}

// host: the two slabs are the caller's host memory, otherwise device memory
int pk_create(h2agg_ctx* c, const h2agg_vk* vk, const void* fixed, const void* sigma, unsigned forms, h2agg_pk** out, bool host) {
    if (out) *out = nullptr;
    if (c->dbg_phases) c->last_phases.clear();
    if (!vk) return fail(c, H2AGG_ERR_INVALID, "null verifying key");
    if (!out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    if (forms & ~(unsigned)H2AGG_PK_COSETS) return fail(c, H2AGG_ERR_INVALID, "pk_create: unknown bits in forms");
    const QtLayout l = qt_layout(*vk, 0, pk_mode(forms));
    if (const char* why = qt_shape_refusal(*vk, l)) return fail(c, H2AGG_ERR_INVALID, why);
    if ((l.F && !fixed) || (l.P && !sigma)) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    std::unique_ptr<h2agg_pk> o(new h2agg_pk());   // every failure below is a plain return: the owners release what was made
    o->ctx = c;
    o->vk = vk;
    o->device = c->device;
    o->k = vk->k;
    o->e = l.e;
    o->forms = forms;
    o->F = l.F;
    o->P = l.P;
    const size_t col = o->col(), fp = (size_t)l.F + l.P;
    if (fp) TRY(dev_alloc(c, o->lagrange, fp * col, "proving key, Lagrange forms"));
    TRY(dev_alloc(c, o->coeff, o->key_cols() * col, "proving key, coefficient forms"));
    if (forms & H2AGG_PK_COSETS) TRY(dev_alloc(c, o->cosets, (o->key_cols() * col) << l.e, "proving key, coset forms"));
    const hipMemcpyKind kind = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    if (l.F) HIP_TRY(c, hipMemcpyAsync(o->lagrange, fixed, l.F * col, kind, c->stream));
    if (l.P) HIP_TRY(c, hipMemcpyAsync(o->lagrange + l.F * col, sigma, l.P * col, kind, c->stream));
    TRY(clear_flags(c));
    const int rc = pk_build(c, o.get());
    if (rc != H2AGG_OK) {
        (void)hipStreamSynchronize(c->stream);   // nothing queued may still write the forms when their owners go
        return rc;
    }
    *out = o.release();
    return H2AGG_OK;
}

int pk_of(h2agg_ctx* c, const h2agg_pk* pk) {
    if (!pk) return fail(c, H2AGG_ERR_INVALID, "null proving key");
    if (pk->ctx != c) return fail(c, H2AGG_ERR_INVALID, "the proving key belongs to another context");
    return H2AGG_OK;
}

}  // namespace

extern "C" {

int h2agg_pk_create(h2agg_ctx* c, const h2agg_vk* vk, const uint8_t* fixed, const uint8_t* sigma, unsigned forms, h2agg_pk** out) try {
    if (out) *out = nullptr;
    TRY(bind(c));
    return pk_create(c, vk, fixed, sigma, forms, out, true);
} API_CATCH

int h2agg_pk_create_resident(h2agg_ctx* c, const h2agg_vk* vk, const void* d_fixed, const void* d_sigma, unsigned forms,
                             h2agg_pk** out) try {
    if (out) *out = nullptr;
    TRY(bind(c));
    return pk_create(c, vk, d_fixed, d_sigma, forms, out, false);
} API_CATCH

// no context and no device
int h2agg_pk_bytes(const h2agg_vk* vk, unsigned forms, size_t* bytes_out) try {
    if (!vk || !bytes_out || (forms & ~(unsigned)H2AGG_PK_COSETS)) return H2AGG_ERR_INVALID;
    const QtLayout l = qt_layout(*vk, 0, pk_mode(forms));
    if (qt_shape_refusal(*vk, l)) return H2AGG_ERR_INVALID;
    *bytes_out = pk_bytes(l, vk->k, forms);
    return H2AGG_OK;
} API_CATCH

int h2agg_pk_info(const h2agg_pk* pk, unsigned* k_out, unsigned* e_out, size_t* fixed_out, size_t* sigma_out, unsigned* forms_out,
                  size_t* bytes_out) try {
    if (!pk) return H2AGG_ERR_INVALID;
    if (k_out) *k_out = pk->k;
    if (e_out) *e_out = pk->e;
    if (fixed_out) *fixed_out = pk->F;
    if (sigma_out) *sigma_out = pk->P;
    if (forms_out) *forms_out = pk->forms;
    if (bytes_out) *bytes_out = pk_bytes(qt_layout(*pk->vk, 0, pk_mode(pk->forms)), pk->k, pk->forms);
    return H2AGG_OK;
} API_CATCH

int h2agg_pk_ptr(const h2agg_pk* pk, int which, size_t coset, const void** d_ptr_out, size_t* columns_out) try {
    if (d_ptr_out) *d_ptr_out = nullptr;
    if (columns_out) *columns_out = 0;
    if (!pk) return H2AGG_ERR_INVALID;
    h2agg_ctx* c = pk->ctx;
    if (!d_ptr_out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    const size_t col = pk->col();
    const uint8_t* p = nullptr;
    size_t columns = 0;
    switch (which) {
    case H2AGG_PK_FIXED_LAGRANGE: p = pk->lagrange, columns = pk->F; break;
    case H2AGG_PK_SIGMA_LAGRANGE: p = pk->lagrange + pk->F * col, columns = pk->P; break;
    case H2AGG_PK_FIXED_COEFF: p = pk->coeff, columns = pk->F; break;
    case H2AGG_PK_SIGMA_COEFF: p = pk->coeff + pk->F * col, columns = pk->P; break;
    case H2AGG_PK_LAGRANGE_COEFF: p = pk->coeff + ((size_t)pk->F + pk->P) * col, columns = 3; break;
    case H2AGG_PK_COSET:
        if (!(pk->forms & H2AGG_PK_COSETS)) return fail(c, H2AGG_ERR_INVALID, "pk_ptr: the key was built without H2AGG_PK_COSETS");
        if (coset >= ((size_t)1 << pk->e)) return fail(c, H2AGG_ERR_INVALID, "pk_ptr: coset >= 2^e");
        p = pk->cosets + coset * pk->key_cols() * col, columns = pk->key_cols();
        break;
    default:
        return fail(c, H2AGG_ERR_INVALID, "pk_ptr: unknown form");
    }
    *d_ptr_out = columns ? p : nullptr;   // (a form without columns has no address)
    if (columns_out) *columns_out = columns;
    return H2AGG_OK;
} API_CATCH

int h2agg_pk_quotient(h2agg_ctx* c, const h2agg_pk* pk, const void* d_advice, const void* d_instance, const void* d_perm_z,
                      const void* d_lookup_z, const void* d_lookup_ap, const void* d_lookup_sp, const uint8_t* challenges,
                      const uint8_t theta[32], const uint8_t beta[32], const uint8_t gamma[32], const uint8_t y[32],
                      const uint8_t delta[32], void* d_h) try {
    TRY(bind(c));
    TRY(pk_of(c, pk));
    const size_t col = pk->col();
    const uint8_t* coeff = pk->coeff;
    const QtSlabs s = {(const uint8_t*)d_advice,   coeff,                      (const uint8_t*)d_instance,  coeff + pk->F * col,
                       (const uint8_t*)d_perm_z,   (const uint8_t*)d_lookup_z, (const uint8_t*)d_lookup_ap, (const uint8_t*)d_lookup_sp};
    const QtKey key = {coeff + ((size_t)pk->F + pk->P) * col, pk->forms & H2AGG_PK_COSETS ? (const uint8_t*)pk->cosets : nullptr};
    QtLayout l;
    QtScalars sc;
    TRY(qt_check(c, pk->vk, s, challenges, theta, beta, gamma, y, delta, d_h, &l, &sc, pk_mode(pk->forms)));
    return qt_queue(c, *pk->vk, l, sc, s, (uint8_t*)d_h, &key);
} API_CATCH

// no device: the route is the rule's, as for h2agg_quotient_work_bytes
int h2agg_pk_quotient_work_bytes(const h2agg_pk* pk, size_t* bytes_out) try {
    if (!pk || !bytes_out) return H2AGG_ERR_INVALID;
    const QtLayout l = qt_layout(*pk->vk, 0, pk_mode(pk->forms));
    *bytes_out = 32 * l.total + l.fft_work;
    return H2AGG_OK;
} API_CATCH

void h2agg_pk_destroy(h2agg_pk* pk) {
    if (!pk) return;
    (void)hipSetDevice(pk->device);
    (void)join_tails(pk->ctx);
    if (pk->ctx->stream) (void)hipStreamSynchronize(pk->ctx->stream);
    delete pk;   // (hipFree waits for the device once more)
}

}  // extern "C"
