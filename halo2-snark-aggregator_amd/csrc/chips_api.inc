// The chips' batch calls over host buffers (included into h2agg.hip behind msm_run.inc: shares the context internals; kernels in
// batch_kernels.hpp and scalar_mul_kernels.hpp): h2agg_fr_batch_op, _batch_pow_constant, _mul_add_accumulate,
// _sum_with_coeff_and_constant and h2agg_g1_batch_add, _batch_scalar_mul, _batch_to_affine (and _device), _batch_decompress,
// _batch_compress, h2agg_g1_sum.  Each one is ensure / stage_in / clear_flags / one launch / stage_out (csrc/host.inc).

extern "C" {

// ---------------------------------------------------------------- Fr
int h2agg_fr_batch_op(h2agg_ctx* c, int op, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out) try {
    TRY(bind(c));
    if (op < H2AGG_OP_ADD || op > H2AGG_OP_DIV) return fail(c, H2AGG_ERR_INVALID, "unknown field op");
    if (n == 0) return H2AGG_OK;
    const bool binary = op <= H2AGG_OP_MUL || op == H2AGG_OP_DIV;
    if (!a || !out || (binary && !b)) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_a, 32 * n));
    TRY(ensure(c, c->out, 32 * n));
    TRY(stage_in(c, c->in_a, a, 32 * n));
    if (binary) {
        TRY(ensure(c, c->in_b, 32 * n));
        TRY(stage_in(c, c->in_b, b, 32 * n));
    }
    TRY(clear_flags(c));
    hipLaunchKernelGGL(k_fr_batch_op, dim3(grid_for(c, n)), dim3(BLOCK), 0, c->stream, op, (const uint8_t*)c->in_a.p,
                       (const uint8_t*)c->in_b.p, n, (uint8_t*)c->out.p, c->d_flags);
    return stage_out(c, out, c->out.p, 32 * n);
} API_CATCH

int h2agg_fr_batch_pow_constant(h2agg_ctx* c, const uint8_t* a, size_t n, uint64_t exponent, uint8_t* out) try {
    TRY(bind(c));
    if (exponent < 1) return fail(c, H2AGG_ERR_INVALID, "assert!(exponent >= 1) failed (arith/field.rs:89)");
    if (n == 0) return H2AGG_OK;
    if (!a || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_a, 32 * n));
    TRY(ensure(c, c->out, 32 * n));
    TRY(stage_in(c, c->in_a, a, 32 * n));
    TRY(clear_flags(c));
    hipLaunchKernelGGL(k_fr_batch_pow, dim3(grid_for(c, n)), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->in_a.p, n,
                       exponent, (uint8_t*)c->out.p, c->d_flags);
    return stage_out(c, out, c->out.p, 32 * n);
} API_CATCH

int h2agg_fr_mul_add_accumulate(h2agg_ctx* c, const uint8_t* v, size_t n, const uint8_t b[32], uint8_t out[32]) try {
    TRY(bind(c));
    if ((n && !v) || !b || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_a, 32 * n + 32));
    TRY(ensure(c, c->in_b, 32));
    TRY(ensure(c, c->out, 32));
    TRY(stage_in(c, c->in_a, v, 32 * n));
    TRY(stage_in(c, c->in_b, b, 32));
    TRY(clear_flags(c));
    hipLaunchKernelGGL(k_fr_horner, dim3(1), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->in_a.p, n,
                       (const uint8_t*)c->in_b.p, (uint8_t*)c->out.p, c->d_flags);
    return stage_out(c, out, c->out.p, 32);
} API_CATCH

int h2agg_fr_sum_with_coeff_and_constant(h2agg_ctx* c, const uint8_t* x, const uint8_t* coeff, size_t n,
                                         const uint8_t b[32], uint8_t out[32]) try {
    TRY(bind(c));
    if ((n && (!x || !coeff)) || !b || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_a, 32 * n + 32));
    TRY(ensure(c, c->in_b, 32 * n + 32));
    TRY(ensure(c, c->in_c, 32));
    TRY(ensure(c, c->out, 32));
    TRY(stage_in(c, c->in_a, x, 32 * n));
    TRY(stage_in(c, c->in_b, coeff, 32 * n));
    TRY(stage_in(c, c->in_c, b, 32));
    TRY(clear_flags(c));
    hipLaunchKernelGGL(k_fr_sum_coeff, dim3(1), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->in_a.p,
                       (const uint8_t*)c->in_b.p, n, (const uint8_t*)c->in_c.p, (uint8_t*)c->out.p, c->d_flags);
    return stage_out(c, out, c->out.p, 32);
} API_CATCH

// ---------------------------------------------------------------- G1 batch
int h2agg_g1_batch_add(h2agg_ctx* c, const uint8_t* a, const uint8_t* b, size_t n, int subtract, uint8_t* out) try {
    TRY(bind(c));
    if (n == 0) return H2AGG_OK;
    if (!a || !b || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_a, 96 * n));
    TRY(ensure(c, c->in_b, 96 * n));
    TRY(ensure(c, c->out, 96 * n));
    TRY(stage_in(c, c->in_a, a, 96 * n));
    TRY(stage_in(c, c->in_b, b, 96 * n));
    TRY(clear_flags(c));
    hipLaunchKernelGGL(k_g1_batch_add, dim3(grid_for(c, n)), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->in_a.p,
                       (const uint8_t*)c->in_b.p, n, subtract, (uint8_t*)c->out.p, c->d_flags);
    return stage_out(c, out, c->out.p, 96 * n);
} API_CATCH

int h2agg_g1_batch_scalar_mul(h2agg_ctx* c, const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t* out) try {
    TRY(bind(c));
    if (n == 0) return H2AGG_OK;
    if (!bases || !scalars || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_a, 64 * n));
    TRY(ensure(c, c->in_b, 32 * n));
    TRY(ensure(c, c->out, 96 * n));
    TRY(stage_in(c, c->in_a, bases, 64 * n));
    TRY(stage_in(c, c->in_b, scalars, 32 * n));
    TRY(clear_flags(c));
    // GLV + signed window-4 ladder, four lanes per point (csrc/scalar_mul_kernels.hpp); H2AGG_SCALAR_MUL=ladder selects the
    // round-1 bit-serial kernel for A/B measurements
    static const bool ladder = knob("H2AGG_SCALAR_MUL") && !strcmp(knob("H2AGG_SCALAR_MUL"), "ladder");
    if (ladder) {
        hipLaunchKernelGGL(k_g1_batch_scalar_mul, dim3(grid_for(c, n)), dim3(BLOCK), 0, c->stream,
                           (const uint8_t*)c->in_a.p, (const uint8_t*)c->in_b.p, n, (uint8_t*)c->out.p, c->d_flags);
    } else {
        size_t groups = (n + SM_GROUPS - 1) / SM_GROUPS;
        const size_t cap = launch_cap(c, 16);
        if (groups > cap) groups = cap;
        hipLaunchKernelGGL(k_g1_batch_scalar_mul_w4, dim3((unsigned)groups), dim3(SM_THREADS), 0, c->stream,
                           (const uint8_t*)c->in_a.p, (const uint8_t*)c->in_b.p, n, (uint8_t*)c->out.p, c->d_flags);
    }
    return stage_out(c, out, c->out.p, 96 * n);
} API_CATCH

int h2agg_g1_batch_to_affine(h2agg_ctx* c, const uint8_t* in, size_t n, uint8_t* out) try {
    TRY(bind(c));
    if (n == 0) return H2AGG_OK;
    if (!in || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_a, 96 * n));
    TRY(ensure(c, c->out, 64 * n));
    TRY(stage_in(c, c->in_a, in, 96 * n));
    TRY(clear_flags(c));
    hipLaunchKernelGGL(k_g1_batch_to_affine, dim3(grid_for(c, n)), dim3(BLOCK), 0, c->stream,
                       (const uint8_t*)c->in_a.p, n, (uint8_t*)c->out.p, c->d_flags);
    return stage_out(c, out, c->out.p, 64 * n);
} API_CATCH

int h2agg_g1_batch_to_affine_device(h2agg_ctx* c, const uint8_t* d_in_jac, size_t n, uint8_t* out) try {
    TRY(bind(c));
    if (n == 0) return H2AGG_OK;
    if (!d_in_jac || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(join_tails(c));   // the inputs are typically results of h2agg_g1_msm_device_async
    TRY(ensure(c, c->out, 64 * n));
    TRY(clear_flags(c));
    hipLaunchKernelGGL(k_g1_batch_to_affine, dim3(grid_for(c, n)), dim3(BLOCK), 0, c->stream, d_in_jac, n,
                       (uint8_t*)c->out.p, c->d_flags);
    return stage_out(c, out, c->out.p, 64 * n);
} API_CATCH

int h2agg_g1_batch_decompress(h2agg_ctx* c, const uint8_t* in, size_t n, uint8_t* out_aff, uint8_t* ok) try {
    TRY(bind(c));
    if (n == 0) return H2AGG_OK;
    if (!in || !out_aff) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_a, 32 * n));
    TRY(ensure(c, c->out, 64 * n));
    TRY(ensure(c, c->in_b, n + 16));
    TRY(stage_in(c, c->in_a, in, 32 * n));
    TRY(clear_flags(c));
    hipLaunchKernelGGL(k_g1_batch_decompress, dim3(grid_for(c, n)), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->in_a.p, n,
                       (uint8_t*)c->out.p, (uint8_t*)c->in_b.p, c->d_flags);
    HIP_TRY(c, hipMemcpyAsync(out_aff, c->out.p, 64 * n, hipMemcpyDeviceToHost, c->stream));
    if (ok) return stage_out(c, ok, c->in_b.p, n);
    return finish(c);
} API_CATCH
int h2agg_g1_batch_compress(h2agg_ctx* c, const uint8_t* aff, size_t n, uint8_t* out) try {
    TRY(bind(c));
    if (n == 0) return H2AGG_OK;
    if (!aff || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_a, 64 * n));
    TRY(ensure(c, c->out, 32 * n));
    TRY(stage_in(c, c->in_a, aff, 64 * n));
    TRY(clear_flags(c));
    hipLaunchKernelGGL(k_g1_batch_compress, dim3(grid_for(c, n)), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->in_a.p, n,
                       (uint8_t*)c->out.p, c->d_flags);
    return stage_out(c, out, c->out.p, 32 * n);
} API_CATCH

int h2agg_g1_sum(h2agg_ctx* c, const uint8_t* in, size_t n, uint8_t out[96]) try {
    TRY(bind(c));
    if (!out || (n && !in)) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_a, 96 * n + 96));
    TRY(stage_in(c, c->in_a, in, 96 * n));
    TRY(clear_flags(c));
    hipLaunchKernelGGL(k_g1_sum, dim3(1), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->in_a.p, n, c->d_res_jac,
                       c->d_flags);
    return fetch_result_jac(c, out);
} API_CATCH

}  // extern "C"
