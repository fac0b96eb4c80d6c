// Segmented multi_exp, host side (included into h2agg.hip: shares the context internals; kernels in seg_msm_kernels.hpp):
// seg_msm_run and h2agg_g1_msm_segmented.  (Its other caller, the 2N-side evaluation of h2agg_verify_proofs: schema_api.inc.)

namespace {

constexpr int SEG_C_DEFAULT = 5;             // DESIGN.md: the segmented multi_exp's window width
constexpr size_t SEG_CHUNK_AUTO = 16384;     // points per set of launches (SMALL_SORT_N, the one-launch sort's range)

template <int C>
void seg_window_launch(hipStream_t st, const uint8_t* bases, const uint8_t* scalars, const uint32_t* d_seg, uint32_t first,
                       uint32_t count, uint32_t maxlen, uint8_t* wsum) {
    const int W = window_count(C, false);
    hipLaunchKernelGGL(k_seg_window<C>, dim3((unsigned)W, count), dim3(SegCfg<C>::T), seg_window_lds<C>(maxlen), st, bases,
                       scalars, d_seg, first, W, wsum);
}

// S multi_exps over the segments seg[s] .. seg[s + 1] of d_bases (Montgomery affine) / d_scalars (canonical): canonical Jacobian
// to d_out_jac[96 s].  d_seg: the same offsets on the device (32-bit).  Segments are taken in groups of whole segments of at
// most `seg_chunk` points (h2agg_debug_configure "seg_chunk"; 0 = SEG_CHUNK_AUTO), each group one window launch + one Horner
// launch, all queued back to back on the context's stream; a segment longer than that range (or than SEG_MAX_LEN) is an
// ordinary msm_run of its own.  The caller joins the tail streams before reading the results.
int seg_msm_run(h2agg_ctx* c, const uint8_t* d_bases, const uint8_t* d_scalars, const uint64_t* seg, size_t S,
                const uint32_t* d_seg, uint8_t* d_out_jac) {
    const int C = c->dbg_seg_c ? c->dbg_seg_c : SEG_C_DEFAULT;
    if (C < 4 || C > 8) return fail(c, H2AGG_ERR_INVALID, "seg_c must be 4 .. 8");
    const int W = window_count(C, false);
    size_t chunk = c->dbg_seg_chunk > 0 ? (size_t)c->dbg_seg_chunk : SEG_CHUNK_AUTO;
    const size_t longest = chunk < SEG_MAX_LEN ? chunk : SEG_MAX_LEN;
    TRY(ensure(c, c->seg_wsum, S * (size_t)W * XYZZ_BYTES + 256));
    hipStream_t st = c->stream;
    size_t s = 0;
    while (s < S) {
        const size_t len = (size_t)(seg[s + 1] - seg[s]);
        if (len > longest) {
            TRY(msm_run(c, MsmCall{d_bases + 64 * seg[s], d_scalars + 32 * seg[s], len, d_out_jac + 96 * s}));
            ++s;
            continue;
        }
        size_t e = s, pts = 0;
        uint32_t maxlen = 0;
        while (e < S && e - s < 65535) {   // (grid y)
            const size_t l = (size_t)(seg[e + 1] - seg[e]);
            if (l > longest || pts + l > chunk) break;
            pts += l;
            if (l > maxlen) maxlen = (uint32_t)l;
            ++e;
        }
        const uint32_t count = (uint32_t)(e - s);
        uint8_t* wsum = (uint8_t*)c->seg_wsum.p + XYZZ_BYTES * (size_t)W * s;
        switch (C) {
            case 4: seg_window_launch<4>(st, d_bases, d_scalars, d_seg, (uint32_t)s, count, maxlen, wsum); break;
            case 5: seg_window_launch<5>(st, d_bases, d_scalars, d_seg, (uint32_t)s, count, maxlen, wsum); break;
            case 6: seg_window_launch<6>(st, d_bases, d_scalars, d_seg, (uint32_t)s, count, maxlen, wsum); break;
            case 7: seg_window_launch<7>(st, d_bases, d_scalars, d_seg, (uint32_t)s, count, maxlen, wsum); break;
            default: seg_window_launch<8>(st, d_bases, d_scalars, d_seg, (uint32_t)s, count, maxlen, wsum); break;
        }
        hipLaunchKernelGGL(k_msm_final_lp, dim3(count), dim3(64), 0, st, (const uint8_t*)wsum, C, W, (uint8_t*)nullptr,
                           d_out_jac + 96 * s);
        s = e;
    }
    HIP_TRY(c, hipGetLastError());
    return H2AGG_OK;
}

bool fr_bytes_canonical(const uint8_t* b) {   // little-endian integer < r
    uint64_t w[4];
    memcpy(w, b, 32);
    return !poseidon_host::geq_mod(w);
}

}  // namespace

extern "C" {

int h2agg_g1_msm_segmented(h2agg_ctx* c, const uint8_t* bases_aff, const uint8_t* scalars, size_t n, const uint64_t* seg_start,
                           size_t nseg, uint8_t* out_jac) try {
    TRY(bind(c));
    if (!out_jac || !seg_start || nseg == 0) return fail(c, H2AGG_ERR_INVALID, "null buffer or no segments");
    for (size_t s = 0; s < nseg; ++s) set_identity_jac(out_jac + 96 * s);
    if (seg_start[0] != 0 || seg_start[nseg] != n) return fail(c, H2AGG_ERR_INVALID, "seg_start must run from 0 to n");
    for (size_t s = 0; s < nseg; ++s) {
        if (seg_start[s + 1] < seg_start[s]) return fail(c, H2AGG_ERR_INVALID, "seg_start must not decrease");
        if (seg_start[s + 1] == seg_start[s])
            return fail(c, H2AGG_ERR_EMPTY, "multi_exp of zero pairs (reference panics: mock/arith/ecc.rs:128)");
    }
    if (!bases_aff || !scalars) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    if (n >= ((size_t)1 << 30)) return fail(c, H2AGG_ERR_INVALID, "n must be < 2^30");
    for (size_t i = 0; i < n; ++i)
        if (!fr_bytes_canonical(scalars + 32 * i)) return fail(c, H2AGG_ERR_NONCANONICAL, "input integer >= modulus");
    std::vector<uint32_t> seg32(nseg + 1);
    for (size_t s = 0; s <= nseg; ++s) seg32[s] = (uint32_t)seg_start[s];
    TRY(ensure(c, c->in_a, 64 * n));
    TRY(ensure(c, c->in_b, 32 * n));
    TRY(ensure(c, c->tmp_bases, 64 * n));
    TRY(ensure(c, c->seg_dev, 4 * (nseg + 1)));
    TRY(ensure(c, c->seg_out, 96 * nseg));
    hipStream_t st = c->stream;
    TRY(clear_flags(c));
    HIP_TRY(c, hipMemcpyAsync(c->in_a.p, bases_aff, 64 * n, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->in_b.p, scalars, 32 * n, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->seg_dev.p, seg32.data(), 4 * (nseg + 1), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_bases_to_mont, dim3(grid_for(c, n)), dim3(BLOCK), 0, st, (const uint8_t*)c->in_a.p, n,
                       (uint8_t*)c->tmp_bases.p, c->d_flags);
    TRY(seg_msm_run(c, (const uint8_t*)c->tmp_bases.p, (const uint8_t*)c->in_b.p, seg_start, nseg, (const uint32_t*)c->seg_dev.p,
                    (uint8_t*)c->seg_out.p));
    TRY(join_tails(c));
    HIP_TRY(c, hipMemcpyAsync(out_jac, c->seg_out.p, 96 * nseg, hipMemcpyDeviceToHost, st));
    const int rc = finish(c);
    if (rc != H2AGG_OK)
        for (size_t s = 0; s < nseg; ++s) set_identity_jac(out_jac + 96 * s);
    return rc;
} API_CATCH

}  // extern "C"
