// The multi_exp entry points (included into h2agg.hip behind bases_api.inc: shares the context internals; every MSM runs through
// msm_run, csrc/msm_run.inc): over a resident table h2agg_g1_msm_device_async / _batch_async / _device / _preloaded and
// h2agg_instance_commitment; over host buffers h2agg_g1_msm / _jac (msm_host) and h2agg_eval_flat; h2agg_host_alloc / _free for
// the page-locked buffers they like to be handed.

namespace {

// h2agg_g1_msm / h2agg_g1_msm_jac: host buffers in.  stride = 64: canonical affine bases; 96: canonical Jacobian points,
// normalised on the device (k_jac_to_mont_affine) where the affine entry point converts to Montgomery form (k_bases_to_mont)
int msm_host(h2agg_ctx* c, const uint8_t* bases, size_t stride, const uint8_t* scalars, size_t n, uint8_t out[96]) {
    TRY(bind(c));
    if (!out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    set_identity_jac(out);
    if (n == 0) return fail(c, H2AGG_ERR_EMPTY, "multi_exp of zero pairs (reference panics: mock/arith/ecc.rs:128)");
    if (!bases || !scalars) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_a, stride * n));
    TRY(ensure(c, c->in_b, 32 * n));
    TRY(ensure(c, c->tmp_bases, 64 * n));
    TRY(clear_flags(c));
    // Large inputs are cut into slices that cross PCIe on a copy stream while the previous slice is being computed
    // (an MSM is a sum over points, so the slices' results just add up): 96 B/point of transfer hide under ~1.7 ns/point
    // of arithmetic, instead of preceding it.  Slices of >= 2^19 points keep the per-MSM efficiency (2^18-point slices lose more than the overlap gains).
    const bool chained = c->dbg_pcie_chain != 0;
    // chained slices (below) of ~200 K points: the transfer (1.73 ns/point) and the slice's sort + accumulation (~90 us +
    // 1.3 ns/point) then take turns of equal length — measured, profiles/r03_sweeps.txt section 10: 2^20 points 3.03 / 2.97 /
    // 2.92 / 2.96 / 3.15 ms with 3 / 4 / 5 / 6 / 8 slices
    const size_t MIN_SLICE = chained ? (size_t)200 << 10 : (size_t)1 << 19;
    size_t nslices = chained ? (n + MIN_SLICE / 2) / MIN_SLICE : n / MIN_SLICE;
    if (nslices > MSM_MAX_SLICES) nslices = MSM_MAX_SLICES;
    // (h2agg_debug_configure "pcie_slices": tests vary it per call)
    if (c->dbg_pcie_slices >= 1 && c->dbg_pcie_slices <= MSM_MAX_SLICES && n >= ((size_t)1 << 10) * (size_t)c->dbg_pcie_slices)
        nslices = (size_t)c->dbg_pcie_slices;
    if (nslices < 2) {
        TRY(stage_in(c, c->in_a, bases, stride * n));
        TRY(stage_in(c, c->in_b, scalars, 32 * n));
        if (stride == 96)
            hipLaunchKernelGGL(k_jac_to_mont_affine, dim3(grid_for(c, (n + TA_K - 1) / TA_K)), dim3(BLOCK), 0, c->stream,
                               (const uint8_t*)c->in_a.p, n, (uint8_t*)c->tmp_bases.p, c->d_flags);
        else
            hipLaunchKernelGGL(k_bases_to_mont, dim3(grid_for(c, n)), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->in_a.p, n,
                               (uint8_t*)c->tmp_bases.p, c->d_flags);
        TRY(msm_run(c, MsmCall{(const uint8_t*)c->tmp_bases.p, (const uint8_t*)c->in_b.p, n, c->d_res_jac}));
        return fetch_result_jac(c, out);
    }
    TRY(ensure(c, c->out, 96 * MSM_MAX_SLICES));
    // the copy stream must not overwrite in_a / in_b while earlier work on the main stream still reads them
    HIP_TRY(c, hipEventRecord(c->ev_ready, c->stream));
    HIP_TRY(c, hipStreamWaitEvent(c->copy_stream, c->ev_ready, 0));
    const size_t per = (n + nslices - 1) / nslices;
    // The slices share one bucket set (chain modes of msm_run): slice k only sorts its keys and adds its points to the bucket
    // sums; ONE reduction / window-sum / Horner chain follows the last slice — that chain (0.6-0.9 ms of pure latency) is what
    // is left exposed behind the last byte of the transfer, so the slices can be small.  debug key "pcie_chain" 0: the earlier
    // scheme (every slice a whole MSM, results added) for A/B runs.
    MsmCall call;
    if (chained) {
        call.chain_n = n;
        call.chain_glv = c->dbg_pcie_glv ? c->dbg_pcie_glv > 0 : (c->cfg_glv >= 0 && n < ((size_t)1 << 22));
    }
    int rc = H2AGG_OK;
    size_t done = 0, k = 0;
    OverlapScope overlap(c);
    for (; done < n && rc == H2AGG_OK; done += per, ++k) {
        const size_t m = n - done < per ? n - done : per;
        chaos_wait(16, c->copy_stream);
        hipError_t e = hipMemcpyAsync((uint8_t*)c->in_b.p + 32 * done, scalars + 32 * done, 32 * m, hipMemcpyHostToDevice,
                                      c->copy_stream);
        if (e == hipSuccess) e = hipEventRecord(c->ev_copy_s[k], c->copy_stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync((uint8_t*)c->in_a.p + stride * done, bases + stride * done, stride * m, hipMemcpyHostToDevice,
                               c->copy_stream);
        if (e == hipSuccess) e = hipEventRecord(c->ev_copy[k], c->copy_stream);
        // the sort of a slice only reads its scalars: it runs while the slice's bases are still on their way (chained
        // slices; the earlier scheme waits for both, as it always did)
        if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, chained ? c->ev_copy_s[k] : c->ev_copy[k], 0);
        if (e != hipSuccess) {
            rc = fail(c, H2AGG_ERR_HIP, hipGetErrorString(e));
            break;
        }
        auto convert = [=](hipStream_t st) {
            if (stride == 96)
                hipLaunchKernelGGL(k_jac_to_mont_affine, dim3(grid_for(c, (m + TA_K - 1) / TA_K)), dim3(BLOCK), 0, st,
                                   (const uint8_t*)c->in_a.p + 96 * done, m, (uint8_t*)c->tmp_bases.p + 64 * done, c->d_flags);
            else
                hipLaunchKernelGGL(k_bases_to_mont, dim3(grid_for(c, m)), dim3(BLOCK), 0, st,
                                   (const uint8_t*)c->in_a.p + 64 * done, m, (uint8_t*)c->tmp_bases.p + 64 * done, c->d_flags);
        };
        if (chained) {
            call.chain = done == 0 ? CHAIN_FIRST : (done + per >= n ? CHAIN_LAST : CHAIN_MID);
            hipEvent_t ev_bases = c->ev_copy[k];
            c->bases_hook = [=](hipStream_t st) -> int {
                HIP_TRY(c, hipStreamWaitEvent(st, ev_bases, 0));
                convert(st);
                return H2AGG_OK;
            };
        } else {
            convert(c->stream);
        }
        call.d_bases = (const uint8_t*)c->tmp_bases.p + 64 * done;
        call.d_scalars = (const uint8_t*)c->in_b.p + 32 * done;
        call.n_base = m;
        call.d_out_jac = chained ? c->d_res_jac : (uint8_t*)c->out.p + 96 * k;
        rc = msm_run(c, call);
        c->bases_hook = nullptr;
    }
    overlap.restore();
    TRY(rc);
    TRY(join_tails(c));
    if (!chained)
        hipLaunchKernelGGL(k_g1_sum, dim3(1), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->out.p, k, c->d_res_jac, c->d_flags);
    return fetch_result_jac(c, out);
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- MSM
int h2agg_g1_msm_device_async(h2agg_ctx* c, uint64_t handle, const void* d_scalars, size_t n, void* d_out_jac) try {
    TRY(bind(c));
    Table* tp = nullptr;
    TRY(find_table(c, handle, &tp));
    Table& t = *tp;
    if (!d_scalars || !d_out_jac) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    if (n == 0) return fail(c, H2AGG_ERR_EMPTY, "multi_exp of zero pairs (reference panics: mock/arith/ecc.rs:128)");
    if (n > t.n) return fail(c, H2AGG_ERR_INVALID, "more scalars than bases in the table");
    if (comb_msm_applies(c, t, n)) {
        bool done = false;
        TRY(comb_msm_run(c, t, (const uint8_t*)d_scalars, n, 1, (uint8_t*)d_out_jac, &done));
        if (done) return H2AGG_OK;
    }
    const uint8_t* endo = nullptr;
    TRY(table_endo(c, t, &endo));
    // Beyond 2^22 points the packed (index | sub-bucket) sort item no longer fits 32 bits and the sort would fall back to
    // its slower two-array kernels: cut the MSM into slices of <= 2^22 points instead (their tails overlap the next
    // slice's bulk) and add the slices' results.
    if (t.pre && !c->cfg_c) {   // fixed-base levels (h2agg_bases_precompute); an explicit window_bits overrides
        const PreTable pt{t.pre, t.n, t.pre_c, t.pre_W};
        if ((size_t)pt.W * n < ((size_t)1 << 32)) {
            MsmCall call{t.d, (const uint8_t*)d_scalars, n, (uint8_t*)d_out_jac};
            call.pre = &pt;
            return msm_run(c, call);
        }
    }
    const size_t SLICE = (size_t)1 << 22;
    MsmCall call{t.d, (const uint8_t*)d_scalars, n, (uint8_t*)d_out_jac};
    call.d_endo_x = endo;
    call.no_identity = t.no_identity;
    if (n <= SLICE) return msm_run(c, call);
    // The slices share ONE bucket set (chain modes of msm_run): every slice adds its points to the sums the buckets already
    // hold, and only the last one is followed by the bucket reduction / window sums / Horner tail.
    const size_t nsl = (n + SLICE - 1) / SLICE;
    const bool was_overlap = c->tail_overlap;
    {
        OverlapScope overlap(c);
        call.chain_n = n;
        call.chain_glv = false;
        for (size_t k = 0; k < nsl; ++k) {
            const size_t off = k * SLICE;
            call.d_bases = t.d + 64 * off;
            call.d_scalars = (const uint8_t*)d_scalars + 32 * off;
            call.d_endo_x = endo + 32 * off;
            call.n_base = n - off < SLICE ? n - off : SLICE;
            call.chain = k == 0 ? CHAIN_FIRST : (k + 1 == nsl ? CHAIN_LAST : CHAIN_MID);
            TRY(msm_run(c, call));
        }
    }
    if (!was_overlap) TRY(join_tails(c));   // without overlap mode the caller's stream orders the result
    return H2AGG_OK;
} API_CATCH

int h2agg_g1_msm_device_batch_async(h2agg_ctx* c, uint64_t handle, const void* d_scalars, size_t n, size_t batch,
                                    void* d_out_jac) try {
    TRY(bind(c));
    Table* tp = nullptr;
    TRY(find_table(c, handle, &tp));
    Table& t = *tp;
    if (!d_scalars || !d_out_jac) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    if (n == 0 || batch == 0)
        return fail(c, H2AGG_ERR_EMPTY, "multi_exp of zero pairs (reference panics: mock/arith/ecc.rs:128)");
    if (n > t.n) return fail(c, H2AGG_ERR_INVALID, "more scalars than bases in the table");
    if (comb_msm_applies(c, t, n)) {
        bool done = false;
        TRY(comb_msm_run(c, t, (const uint8_t*)d_scalars, n, batch, (uint8_t*)d_out_jac, &done));
        if (done) return H2AGG_OK;
    }
    // MSMs per set of launches: the level-1 sort partitions (batch * W * NB >> sub_bits, sub_bits <= 11) must fit its
    // LDS counters, and the entry count its 32-bit offsets
    // fixed-base levels (h2agg_bases_precompute).  Levels at c = 20 pay only through their own sort, which takes one MSM at
    // a time and no sort knobs: where it does not apply (a configured context; a batch of short columns over a big table, which
    // would also want batch x 2^19 buckets) the levels are left alone and the ordinary path runs over the table — the two-array
    // sort over c = 20 levels measured 113 ms against the ordinary path's 74 (16 MSMs, 2^22 points; ADVICE r5).
    const bool fb_table = t.pre && t.pre_c == FB_C && !c->dbg_pre_big;
    const bool use_pre = t.pre && !c->cfg_c && (!fb_table || (fb_sort_knobs_clear(c) && (batch == 1 || n >= ((size_t)1 << 18))));
    const PreTable pt{t.pre, t.n, t.pre_c, t.pre_W};
    const MsmPlan p1 = make_plan(c, n, 1);
    const uint32_t nb1 = use_pre ? (1u << (pt.c - 1)) : p1.NB;
    const size_t sets1 = use_pre ? 1 : (size_t)p1.W;                               // bucket sets per MSM
    uint32_t ppw_min = nb1 >> 11;
    if (ppw_min < 1) ppw_min = 1;
    size_t per = (size_t)SORT_MAX_PW / (sets1 * ppw_min);
    const size_t ent1 = use_pre ? n * (size_t)pt.W : n * (size_t)p1.W * (p1.glv ? 2 : 1);
    if (per * ent1 >= ((size_t)1 << 31)) per = (((size_t)1 << 31) - 1) / ent1;
    if (per * n >= ((size_t)1 << 29)) per = (((size_t)1 << 29) - 1) / n;
    if (per < 1) per = 1;
    // From 2^20 points on an MSM fills the chip by itself and takes the digit-major sort / two-dimensional reduction, which
    // batches do not: one MSM after another, each one's tail under the next one's bulk (2^22 points: 6.1 -> 5.4 ms each)
    const bool one_by_one = use_pre ? (pt.c == FB_C && n >= ((size_t)1 << 18)) : n >= ((size_t)1 << 20);
    if (one_by_one) per = 1;
    const uint8_t* endo = nullptr;
    TRY(table_endo(c, t, &endo));
    const bool was_overlap = c->tail_overlap;
    {
        OverlapScope overlap(c, one_by_one && batch > 1);
        MsmCall call;
        call.d_bases = t.d;
        call.n_base = n;
        call.d_endo_x = use_pre ? nullptr : endo;
        call.pre = use_pre ? &pt : nullptr;
        call.no_identity = !use_pre && t.no_identity;
        for (size_t q = 0; q < batch; q += per) {
            call.d_scalars = (const uint8_t*)d_scalars + 32 * n * q;
            call.d_out_jac = (uint8_t*)d_out_jac + 96 * q;
            call.batch = (uint32_t)(batch - q < per ? batch - q : per);
            TRY(msm_run(c, call));
        }
    }
    if (one_by_one && batch > 1 && !was_overlap) TRY(join_tails(c));   // without overlap mode the caller's stream orders the results
    return H2AGG_OK;
} API_CATCH

int h2agg_g1_msm_device(h2agg_ctx* c, uint64_t handle, const void* d_scalars, size_t n, uint8_t out[96]) try {
    TRY(bind(c));
    if (!out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    set_identity_jac(out);
    TRY(clear_flags(c));
    TRY(h2agg_g1_msm_device_async(c, handle, d_scalars, n, c->d_res_jac));
    return fetch_result_jac(c, out);
} API_CATCH

int h2agg_g1_msm_preloaded(h2agg_ctx* c, uint64_t handle, const uint8_t* scalars, size_t n, uint8_t out[96]) try {
    TRY(bind(c));
    if (!out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    set_identity_jac(out);
    if (n == 0) return fail(c, H2AGG_ERR_EMPTY, "multi_exp of zero pairs (reference panics: mock/arith/ecc.rs:128)");
    if (!scalars) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(ensure(c, c->in_b, 32 * n));
    TRY(stage_in(c, c->in_b, scalars, 32 * n));
    return h2agg_g1_msm_device(c, handle, c->in_b.p, n, out);
} API_CATCH

// assign_instance_commitment for one instance column (verify.rs:601-603, 623-639)
int h2agg_instance_commitment(h2agg_ctx* c, uint64_t g_lagrange_handle, const uint8_t* instance, size_t len,
                              size_t max_len, uint8_t out_jac[96]) try {
    TRY(bind(c));
    if (!out_jac) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    set_identity_jac(out_jac);
    if (len > max_len)
        return fail(c, H2AGG_ERR_INVALID, "assert!(instance.len() <= params.n() - (blinding_factors + 1)) failed (verify.rs:601-603)");
    if (len == 0) return H2AGG_OK;  // None => pchip.assign_const(identity)  (verify.rs:638)
    return h2agg_g1_msm_preloaded(c, g_lagrange_handle, instance, len, out_jac);
} API_CATCH

int h2agg_host_alloc(h2agg_ctx* c, size_t bytes, void** out) try {
    TRY(bind(c));
    if (!out || bytes == 0) return fail(c, H2AGG_ERR_INVALID, "null out or zero size");
    hipError_t e = hipHostMalloc(out, bytes, hipHostMallocDefault);
    if (e != hipSuccess) return fail(c, H2AGG_ERR_NOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    return H2AGG_OK;
} API_CATCH
int h2agg_host_free(h2agg_ctx* c, void* p) try {
    TRY(bind(c));
    if (p) HIP_TRY(c, hipHostFree(p));
    return H2AGG_OK;
} API_CATCH

int h2agg_g1_msm(h2agg_ctx* c, const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t out[96]) try {
    return msm_host(c, bases, 64, scalars, n, out);
} API_CATCH
int h2agg_g1_msm_jac(h2agg_ctx* c, const uint8_t* points_jac, const uint8_t* scalars, size_t n, uint8_t out[96]) try {
    return msm_host(c, points_jac, 96, scalars, n, out);
} API_CATCH

int h2agg_eval_flat(h2agg_ctx* c, const uint8_t* pts, const uint8_t* scalars, const uint8_t* has_scalar, size_t n,
                    uint8_t out[96]) try {
    TRY(bind(c));
    if (!out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    set_identity_jac(out);
    if (n && (!pts || !scalars || !has_scalar)) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    // host-side partition of the flat list (evaluation.rs:189-196): entries with / without a scalar
    std::vector<uint8_t> ps, ss, pn;
    for (size_t i = 0; i < n; ++i) {
        if (has_scalar[i]) {
            ps.insert(ps.end(), pts + 64 * i, pts + 64 * i + 64);
            ss.insert(ss.end(), scalars + 32 * i, scalars + 32 * i + 32);
        } else {
            pn.insert(pn.end(), pts + 64 * i, pts + 64 * i + 64);
        }
    }
    const size_t m = ss.size() / 32, k = pn.size() / 64;
    if (m == 0) return fail(c, H2AGG_ERR_EMPTY, "multi_exp of zero pairs (reference panics: mock/arith/ecc.rs:128)");
    TRY(ensure(c, c->in_a, 64 * m));
    TRY(ensure(c, c->in_b, 32 * m));
    TRY(ensure(c, c->in_c, 64 * k + 64));
    TRY(ensure(c, c->tmp_bases, 64 * m));
    TRY(stage_in(c, c->in_a, ps.data(), 64 * m));
    TRY(stage_in(c, c->in_b, ss.data(), 32 * m));
    TRY(stage_in(c, c->in_c, pn.data(), 64 * k));
    // pageable-host sources must stay alive until the copies are done
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    TRY(clear_flags(c));
    hipLaunchKernelGGL(k_bases_to_mont, dim3(grid_for(c, m)), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->in_a.p, m,
                       (uint8_t*)c->tmp_bases.p, c->d_flags);
    TRY(msm_run(c, MsmCall{(const uint8_t*)c->tmp_bases.p, (const uint8_t*)c->in_b.p, m, nullptr}));
    TRY(join_tails(c));
    hipLaunchKernelGGL(k_eval_tail, dim3(1), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->d_res_xyzz,
                       (const uint8_t*)c->in_c.p, k, c->d_res_jac, c->d_flags);
    return fetch_result_jac(c, out);
} API_CATCH

}  // extern "C"
