// KZG parameters, host side (included into h2agg.hip: shares the context internals; kernels in g1_fft_kernels.hpp; fft_omega
// in fr_host.inc):
// h2agg_bases_fft, h2agg_params_setup, h2agg_g2_scalar_mul, h2agg_g2_batch_compress.  They stand for halo2_proofs'
// g_to_lagrange / ParamsKZG::downsize, ParamsKZG::setup and the G2 half of ParamsKZG::write — an unvendored git dependency of
// the reference, recalled from upstream (DESIGN.md section 2); the yardstick is the definition in include/h2agg.h.

namespace {

constexpr size_t FRP_CST_BYTES = 32 * (FRP_TABLE + 2);

// d_out[i] = A * base^i + B, i < n (canonical), queued on the context's stream; d_cst: FRP_CST_BYTES of device memory
int fr_affine_powers_launch(h2agg_ctx* c, ph::HFr base, const ph::HFr& A, const ph::HFr& B, size_t n, uint8_t* d_cst, uint8_t* d_out) {
    uint8_t cst[FRP_CST_BYTES];
    for (int j = 0; j < FRP_TABLE; ++j) {
        hfr_bytes(base, cst + 32 * j);
        base = ph::mul(base, base);
    }
    hfr_bytes(A, cst + 32 * FRP_TABLE);
    hfr_bytes(B, cst + 32 * (FRP_TABLE + 1));
    HIP_TRY(c, hipMemcpy(d_cst, cst, FRP_CST_BYTES, hipMemcpyHostToDevice));
    const size_t threads = (n + FRP_CHUNK - 1) / FRP_CHUNK;
    hipLaunchKernelGGL(k_fr_affine_powers, dim3((unsigned)((threads + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream,
                       (const uint8_t*)d_cst, n, d_out);
    return H2AGG_OK;
}

// ladder records of w_k^t (inverse: w_k^-t), t < 2^(k-1), resident in the context
int fft_ensure_twiddles(h2agg_ctx* c, unsigned k, int inv) {
    if (c->fft_tw_k[inv] >= (int)k) return H2AGG_OK;
    const size_t cnt = (size_t)1 << (k - 1);
    DevMem pw, cst;   // for this call (their hipFree synchronises: nothing queued still uses them afterwards)
    TRY(dev_alloc(c, pw, 32 * cnt, "twiddles"));
    TRY(dev_alloc(c, cst, FRP_CST_BYTES, "twiddle constants"));
    c->fft_tw_k[inv] = -1;
    TRY(ensure(c, c->fft_tw[inv], 4 * (size_t)FFT_REC_WORDS * cnt));
    const ph::HFr w = fft_omega(k);
    TRY(fr_affine_powers_launch(c, inv ? ph::inv(w) : w, ph::one(), ph::zero(), cnt, (uint8_t*)cst.p, (uint8_t*)pw.p));
    hipLaunchKernelGGL(k_fft_twiddle_digits, dim3(grid_for(c, cnt)), dim3(BLOCK), 0, c->stream, (const uint8_t*)pw.p, cnt,
                       (uint32_t*)c->fft_tw[inv].p, c->d_flags);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->fft_tw_k[inv] = (int)k;
    return H2AGG_OK;
}

// ladder records of 1 / 2^k, k <= FFT_MAX_K
int fft_ensure_scale(h2agg_ctx* c) {
    if (c->fft_scale_ready) return H2AGG_OK;
    constexpr size_t cnt = FFT_MAX_K + 1;
    uint8_t sc[32 * cnt];
    const ph::HFr half = ph::inv(hfr_u64(2));
    ph::HFr cur = ph::one();
    for (size_t k = 0; k < cnt; ++k) {
        hfr_bytes(cur, sc + 32 * k);
        cur = ph::mul(cur, half);
    }
    DevMem d;
    TRY(dev_alloc(c, d, sizeof sc, "scale"));
    TRY(ensure(c, c->fft_scale, 4 * (size_t)FFT_REC_WORDS * cnt));
    HIP_TRY(c, hipMemcpy(d.p, sc, sizeof sc, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_fft_twiddle_digits, dim3(1), dim3(BLOCK), 0, c->stream, (const uint8_t*)d.p, cnt, (uint32_t*)c->fft_scale.p,
                       c->d_flags);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->fft_scale_ready = true;
    return H2AGG_OK;
}

// the transform of the first 2^k points of d_in (Montgomery affine) into d_out (Montgomery affine); synchronous
int fft_run(h2agg_ctx* c, const uint8_t* d_in, unsigned k, int inv, uint8_t* d_out) {
    const size_t n = (size_t)1 << k;
    DevMem work, jac;
    TRY(dev_alloc(c, work, XYZZ_BYTES * n, "FFT work array"));
    TRY(dev_alloc(c, jac, 96 * n, "FFT result"));
    TRY(clear_flags(c));
    if (k) TRY(fft_ensure_twiddles(c, k, inv));
    const uint32_t* scale = nullptr;
    if (k && inv) {
        TRY(fft_ensure_scale(c));
        scale = (const uint32_t*)c->fft_scale.p + (size_t)FFT_REC_WORDS * k;
    }
    hipStream_t st = c->stream;
    hipLaunchKernelGGL(k_g1_fft_load, dim3((unsigned)((n + SM_GROUPS - 1) / SM_GROUPS)), dim3(SM_THREADS), 0, st, d_in, (uint32_t)k,
                       scale, (uint8_t*)work.p);
    const unsigned grid = (unsigned)((n / 2 + SM_GROUPS - 1) / SM_GROUPS);
    const uint32_t* tw = (const uint32_t*)c->fft_tw[inv].p;
    const uint32_t tw_shift = k ? (uint32_t)(c->fft_tw_k[inv] - (int)k) : 0u;
    for (unsigned s = 1; s <= k; ++s) {
        if (((uint32_t)1 << (k - s)) >= FFT_UNIFORM_MIN)
            hipLaunchKernelGGL(k_g1_fft_stage<true>, dim3(grid), dim3(SM_THREADS), 0, st, (uint8_t*)work.p, (uint32_t)k, (uint32_t)s, tw,
                               tw_shift);
        else
            hipLaunchKernelGGL(k_g1_fft_stage<false>, dim3(grid), dim3(SM_THREADS), 0, st, (uint8_t*)work.p, (uint32_t)k, (uint32_t)s, tw,
                               tw_shift);
    }
    hipLaunchKernelGGL(k_g1_fft_to_jac, dim3(grid_for(c, n)), dim3(BLOCK), 0, st, (const uint8_t*)work.p, n, (uint8_t*)jac.p);
    hipLaunchKernelGGL(k_jac_to_mont_affine, dim3(grid_for(c, n)), dim3(BLOCK), 0, st, (const uint8_t*)jac.p, n, d_out, c->d_flags);
    HIP_TRY(c, hipGetLastError());
    return finish(c);
}

// g = s^i * G and / or g_lagrange = L_i(s) * G, i < 2^k, into d_g / d_gl (either may be null); synchronous
int params_setup_run(h2agg_ctx* c, unsigned k, const ph::HFr& s, const ph::HFr& s_n, uint8_t* d_g, uint8_t* d_gl) {
    const size_t n = (size_t)1 << k;
    DevMem scal, invs, cst;
    TRY(dev_alloc(c, scal, 32 * n, "setup scalars"));
    TRY(dev_alloc(c, cst, 2 * FRP_CST_BYTES, "setup constants"));
    if (d_gl) TRY(dev_alloc(c, invs, 32 * n, "setup scalars"));
    TRY(clear_flags(c));
    if (d_g) {
        TRY(fr_affine_powers_launch(c, s, ph::one(), ph::zero(), n, (uint8_t*)cst.p, (uint8_t*)scal.p));
        TRY(comb_generate_launch(c, (const uint8_t*)scal.p, n, d_g));
    }
    if (d_gl) {
        // L_i(s) = w^i (s^n - 1) / (n (s - w^i)) = 1 / d_i with d_i = (s w^-i - 1) / c, c = (s^n - 1) / n: the d_i are A * (w^-1)^i + B
        // with A = s / c, B = -1 / c; no d_i is zero because s^n != 1.  The inversions: the Fr batch kernel (H2AGG_OP_INV).
        const ph::HFr cinv = ph::inv(ph::mul(ph::sub(s_n, ph::one()), ph::inv(hfr_u64((uint64_t)n))));
        TRY(fr_affine_powers_launch(c, ph::inv(fft_omega(k)), ph::mul(s, cinv), ph::sub(ph::zero(), cinv), n,
                                    (uint8_t*)cst.p + FRP_CST_BYTES, (uint8_t*)scal.p));
        hipLaunchKernelGGL(k_fr_batch_op, dim3(grid_for(c, n)), dim3(BLOCK), 0, c->stream, (int)H2AGG_OP_INV, (const uint8_t*)scal.p,
                           (const uint8_t*)nullptr, n, (uint8_t*)invs.p, c->d_flags);
        TRY(comb_generate_launch(c, (const uint8_t*)invs.p, n, d_gl));
    }
    HIP_TRY(c, hipGetLastError());
    return finish(c);
}

}  // namespace

extern "C" {

int h2agg_bases_fft(h2agg_ctx* c, uint64_t in_handle, unsigned k, int inverse, uint64_t* out_handle) try {
    TRY(bind(c));
    if (!out_handle) return fail(c, H2AGG_ERR_INVALID, "null handle pointer");
    if (k > FFT_MAX_K) return fail(c, H2AGG_ERR_INVALID, "k must be <= 24");
    Table* in = nullptr;
    TRY(find_table(c, in_handle, &in));
    const size_t n = (size_t)1 << k;
    if (n > in->n) return fail(c, H2AGG_ERR_INVALID, "the table has fewer than 2^k points");
    Table t;
    TRY(table_new(c, n, &t));
    TRY(fft_run(c, in->d, k, inverse ? 1 : 0, t.d));
    *out_handle = table_register(c, std::move(t));
    return H2AGG_OK;
} API_CATCH

int h2agg_params_setup(h2agg_ctx* c, unsigned k, const uint8_t s[32], uint64_t* g_handle_out, uint64_t* g_lagrange_handle_out) try {
    TRY(bind(c));
    if (!s) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    if (k > FFT_MAX_K) return fail(c, H2AGG_ERR_INVALID, "k must be <= 24");
    if (!fr_bytes_canonical(s)) return fail(c, H2AGG_ERR_NONCANONICAL, "input integer >= modulus");
    uint64_t sw[4];
    memcpy(sw, s, 32);
    const ph::HFr sm = ph::from_words(sw);
    if (ph::is_zero(sm)) return fail(c, H2AGG_ERR_INVALID, "setup: s == 0 (every g[i], i > 0, would be the identity)");
    ph::HFr s_n = sm;
    for (unsigned i = 0; i < k; ++i) s_n = ph::mul(s_n, s_n);
    if (ph::is_zero(ph::sub(s_n, ph::one())))
        return fail(c, H2AGG_ERR_INVALID, "setup: s^n == 1 (halo2: (s - w^i).invert().unwrap() panics)");
    const size_t n = (size_t)1 << k;
    Table tg, tl;
    if (g_handle_out) TRY(table_new(c, n, &tg));
    if (g_lagrange_handle_out) TRY(table_new(c, n, &tl));
    if (tg.d || tl.d) TRY(params_setup_run(c, k, sm, s_n, tg.d, tl.d));
    // (one word for the two tables of the call: table_register reads it for each)
    if (tg.d) *g_handle_out = table_register(c, std::move(tg));
    if (tl.d) *g_lagrange_handle_out = table_register(c, std::move(tl));
    return H2AGG_OK;
} API_CATCH

// s * Q on the twist: double-and-add over the bits of s through the pairing's projective step functions (line values
// discarded, as g2_in_subgroup does).  For a point of order r and 2 <= s < r no prefix m of s has m * Q == +-Q at an addition.
int h2agg_g2_scalar_mul(const uint8_t g2_aff[128], const uint8_t s[32], uint8_t out_aff[128]) try {
    if (!g2_aff || !s || !out_aff) return H2AGG_ERR_INVALID;
    pairing::G2Affine q;
    const int r = pairing::load_g2(g2_aff, q);
    if (r == 1) return H2AGG_ERR_NONCANONICAL;
    if (r) return H2AGG_ERR_BAD_POINT;
    if (!fr_bytes_canonical(s)) return H2AGG_ERR_NONCANONICAL;
    uint64_t e[4];
    memcpy(e, s, 32);
    int top = 255;
    while (top >= 0 && !((e[top / 64] >> (top % 64)) & 1)) --top;
    if (top < 0 || q.inf) {
        memset(out_aff, 0, 128);
        return H2AGG_OK;
    }
    pairing::G2Proj acc = {q.x, q.y, pairing::f2_one()};
    for (int i = top - 1; i >= 0; --i) {
        pairing::g2_double_step(acc);
        if ((e[i / 64] >> (i % 64)) & 1) pairing::g2_add_step(acc, q);
    }
    const pairing::Fq2 zi = pairing::f2_inv(acc.z);
    const pairing::G2Affine o = {pairing::f2_mul(acc.x, zi), pairing::f2_mul(acc.y, zi), false};
    pairing::g2_to_bytes(o, out_aff);
    return H2AGG_OK;
} API_CATCH

int h2agg_g2_batch_compress(const uint8_t* aff, size_t n, uint8_t* out) try {
    if (n && (!aff || !out)) return H2AGG_ERR_INVALID;
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* b = aff + 128 * i;
        pairing::G2Affine q;
        bool zero = true;
        for (int j = 0; j < 128; ++j) zero &= b[j] == 0;
        q.inf = zero;
        if (!pairing::fq_from_bytes(b, q.x.c0) || !pairing::fq_from_bytes(b + 32, q.x.c1) || !pairing::fq_from_bytes(b + 64, q.y.c0) ||
            !pairing::fq_from_bytes(b + 96, q.y.c1))
            return H2AGG_ERR_NONCANONICAL;
        if (!pairing::g2_on_curve(q)) return H2AGG_ERR_BAD_POINT;
        memcpy(out + 64 * i, b, 64);
        if (!zero) out[64 * i + 63] |= (uint8_t)((b[64] & 1) << 7);   // parity of y.c0 (`y.to_bytes()[0] & 1`)
    }
    return H2AGG_OK;
} API_CATCH

}  // extern "C"
