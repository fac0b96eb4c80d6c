// Segmented multi_exp, host side (included into h2agg.hip: shares the context internals; kernels in seg_msm_kernels.hpp):
// h2agg_g1_msm_segmented and the 2N-side evaluation of h2agg_verify_proofs.

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
            TRY(msm_run(c, d_bases + 64 * seg[s], d_scalars + 32 * seg[s], len, d_out_jac + 96 * s));
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
    static const uint64_t R[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
    for (int i = 3; i >= 0; --i) {
        uint64_t w;
        memcpy(&w, b + 8 * i, 8);
        if (w != R[i]) return w < R[i];
    }
    return false;
}

// evaluate_multiopen_proof (verify.rs:690-745) for many (w_x, w_g) pairs of one schema at once: every side's eval_prepare walk
// recorded on the tape, ONE tape run, the 2N multi_exps as ONE segmented multi_exp (the (G, +/- e) pair folded into each side
// as in eval_launch_sides), the scalar-less points, and one field inversion for all sides (Montgomery's trick).
// out_aff: 128 B per pair (left, right), canonical affine.
int evaluate_multiopen_many(h2agg_schema* sc, const std::vector<std::pair<uint32_t, uint32_t>>& roots, uint8_t* out_aff) {
    h2agg_ctx* c = sc->ctx;
    Schema& S = sc->s;
    Tape& t = S.tape;
    const size_t nsides = 2 * roots.size();
    std::vector<EvalLists> L(nsides);
    std::vector<int64_t> extra(nsides, -1);
    std::vector<uint32_t> names;
    for (size_t p = 0; p < roots.size(); ++p) TRY(multiopen_lists(sc, roots[p].first, roots[p].second, &L[2 * p], &extra[2 * p], names));
    // ---- the tape is final: its dependency levels
    const uint32_t nconst = t.nconst, nops = (uint32_t)t.ops.size(), nreg = nconst + nops;
    std::vector<TapeOp> sorted;
    std::vector<uint32_t> lstart, cslot;
    uint32_t maxlevel = 0;
    bool tape_lds = false;
    if (nops) {
        std::vector<TapeOp> ops(nops);
        for (uint32_t k = 0; k < nops; ++k) {
            TapeOp o = t.ops[k];
            o.dst = t.resolve(o.dst);
            o.a = t.resolve(o.a);
            if (o.op != TAPE_SQRN) o.b = t.resolve(o.b);   // (SQRN: b is an immediate count, not a register)
            ops[k] = o;
        }
        if (!schedule_levels(ops, nreg, sorted, lstart, maxlevel)) return fail(c, H2AGG_ERR_INVALID, "tape: operand not yet defined");
        tape_lds = c->dbg_tape_lds && tape_lds_assign(sorted, lstart, nconst, nreg, cslot);
    }
    // ---- one staging block: tape, then per side (in side order) the (register, point) pairs, the scalar-less points, and
    // both segmentations
    std::vector<uint64_t> seg(nsides + 1, 0);
    std::vector<uint32_t> seg32(nsides + 1, 0), pseg(nsides + 1, 0);
    for (size_t s = 0; s < nsides; ++s) {
        seg[s + 1] = seg[s] + L[s].regs_s.size() + (extra[s] >= 0 ? 1 : 0);
        pseg[s + 1] = pseg[s] + (uint32_t)(L[s].pts_ns.size() / 64);
    }
    const size_t M = seg[nsides], K = pseg[nsides];
    if (M >= ((size_t)1 << 30)) return fail(c, H2AGG_ERR_INVALID, "too many evaluation pairs");
    for (size_t s = 0; s <= nsides; ++s) seg32[s] = (uint32_t)seg[s];
    auto align = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t off = 0;
    const size_t off_consts = off;  off = align(off + (size_t)nconst * 32);
    const size_t off_ops = off;     off = align(off + sorted.size() * sizeof(TapeOp));
    const size_t off_lvl = off;     off = align(off + lstart.size() * 4);
    const size_t off_cslot = off;   off = align(off + (tape_lds ? (size_t)nconst * 4 : 0));
    const size_t off_idx = off;     off = align(off + M * 4);
    const size_t off_pts = off;     off = align(off + M * 64);
    const size_t off_pns = off;     off = align(off + K * 64);
    const size_t off_seg = off;     off = align(off + (nsides + 1) * 4);
    const size_t off_pseg = off;    off = align(off + (nsides + 1) * 4);
    const size_t total = off;
    TRY(ensure_stage(c, total));
    TRY(ensure(c, c->sch_in, total));
    TRY(ensure(c, c->sch_regs, (size_t)nreg * REG_WORDS * 4 + 64));
    TRY(ensure(c, c->sch_scalars[0], M * 32 + 32));
    TRY(ensure(c, c->sch_bases[0], M * 64 + 64));
    TRY(ensure(c, c->seg_out, nsides * (96 + 128) + 256));
    uint8_t gen[64] = {0};
    gen[0] = 1;
    gen[32] = 2;   // pchip.assign_one = generator (1, 2)   verify.rs:714
    uint8_t* h = c->h_stage;
    if (nconst) memcpy(h + off_consts, t.consts.data(), (size_t)nconst * 32);
    if (!sorted.empty()) memcpy(h + off_ops, sorted.data(), sorted.size() * sizeof(TapeOp));
    if (!lstart.empty()) memcpy(h + off_lvl, lstart.data(), lstart.size() * 4);
    if (tape_lds && nconst) memcpy(h + off_cslot, cslot.data(), (size_t)nconst * 4);
    uint32_t* idx = (uint32_t*)(h + off_idx);
    for (size_t s = 0; s < nsides; ++s) {
        const size_t m = L[s].regs_s.size(), o = seg[s];
        for (size_t i = 0; i < m; ++i) idx[o + i] = t.resolve(L[s].regs_s[i]);
        memcpy(h + off_pts + 64 * o, L[s].pts_s.data(), m * 64);
        if (extra[s] >= 0) {
            idx[o + m] = t.resolve((uint32_t)extra[s]);
            memcpy(h + off_pts + 64 * (o + m), gen, 64);
        }
        if (!L[s].pts_ns.empty()) memcpy(h + off_pns + 64 * (size_t)pseg[s], L[s].pts_ns.data(), L[s].pts_ns.size());
    }
    memcpy(h + off_seg, seg32.data(), (nsides + 1) * 4);
    memcpy(h + off_pseg, pseg.data(), (nsides + 1) * 4);
    hipStream_t st = c->stream;
    uint8_t* d = (uint8_t*)c->sch_in.p;
    TRY(clear_flags(c));
    HIP_TRY(c, hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, st));
    if (tape_lds) {   // constants + every level in one launch, the register file in LDS (schema.hpp)
        hipLaunchKernelGGL(k_tape_run_lds, dim3(1), dim3(TAPE_THREADS), 0, st, (const uint8_t*)(d + off_consts),
                           (const uint32_t*)(d + off_cslot), nconst, (const TapeOp*)(d + off_ops), (const uint32_t*)(d + off_lvl),
                           maxlevel, (uint32_t*)c->sch_regs.p, c->d_flags);
    } else {
        if (nconst)
            hipLaunchKernelGGL(k_tape_load_consts, dim3((nconst + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st,
                               (const uint8_t*)(d + off_consts), nconst, (uint32_t*)c->sch_regs.p, c->d_flags);
        if (nops)
            hipLaunchKernelGGL(k_tape_run, dim3(1), dim3(TAPE_THREADS), 0, st, (const TapeOp*)(d + off_ops),
                               (const uint32_t*)(d + off_lvl), maxlevel, (uint32_t*)c->sch_regs.p, c->d_flags);
    }
    c->sch_owner = sc;
    sc->tape_done_ops = nops;
    sc->tape_done_consts = nconst;
    // gather + Montgomery form of every side's pairs in one launch, then the segmented multi_exp
    hipLaunchKernelGGL(k_eval_prep<false>, dim3((unsigned)((M + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, (const uint32_t*)c->sch_regs.p,
                       (const uint32_t*)(d + off_idx), (const uint8_t*)(d + off_pts), (uint32_t)M, (uint8_t*)c->sch_scalars[0].p,
                       (uint8_t*)c->sch_bases[0].p, (uint8_t*)nullptr, c->d_flags);
    uint8_t* d_jac = (uint8_t*)c->seg_out.p;
    uint8_t* d_tail = d_jac + 96 * nsides;
    TRY(seg_msm_run(c, (const uint8_t*)c->sch_bases[0].p, (const uint8_t*)c->sch_scalars[0].p, seg.data(), nsides,
                    (const uint32_t*)(d + off_seg), d_jac));
    TRY(join_tails(c));
    hipLaunchKernelGGL(k_seg_tail, dim3((unsigned)nsides), dim3(64), 0, st, (const uint8_t*)d_jac, (const uint8_t*)(d + off_pns),
                       (const uint32_t*)(d + off_pseg), d_tail, c->d_flags);
    std::vector<uint8_t> xyzz(nsides * 128);
    HIP_TRY(c, hipMemcpyAsync(xyzz.data(), d_tail, xyzz.size(), hipMemcpyDeviceToHost, st));
    TRY(finish(c));
    S.point_list_len = L[nsides - 1].regs_s.size();
    S.names = names;
    // ---- x = X / ZZ, y = Y / ZZZ for every side with ONE inversion
    namespace pr = h2agg::pairing;
    std::vector<pr::Fq> X(nsides), Y(nsides), ZZ(nsides), ZZZ(nsides), pre(nsides + 1);
    std::vector<char> inf(nsides);
    pre[0] = pr::fq_one();
    for (size_t s = 0; s < nsides; ++s) {
        const uint8_t* o = xyzz.data() + 128 * s;
        if (!pr::fq_from_bytes(o, X[s]) || !pr::fq_from_bytes(o + 32, Y[s]) || !pr::fq_from_bytes(o + 64, ZZ[s]) ||
            !pr::fq_from_bytes(o + 96, ZZZ[s]))
            return fail(c, H2AGG_ERR_HIP, "evaluate_multiopen_proof: the device returned a non-canonical coordinate");
        inf[s] = pr::fq_is_zero(ZZ[s]);
        pre[s + 1] = inf[s] ? pre[s] : pr::fq_mul(pre[s], pr::fq_mul(ZZ[s], ZZZ[s]));
    }
    pr::Fq inv = pr::fq_inv(pre[nsides]);   // 1 / prod(ZZ ZZZ)
    memset(out_aff, 0, 64 * nsides);        // the identity: zeros (as the device's affine store writes it)
    for (size_t s = nsides; s-- > 0;) {
        if (inf[s]) continue;
        const pr::Fq dinv = pr::fq_mul(inv, pre[s]);                      // 1 / (ZZ_s ZZZ_s)
        inv = pr::fq_mul(inv, pr::fq_mul(ZZ[s], ZZZ[s]));
        pr::fq_to_bytes(pr::fq_mul(X[s], pr::fq_mul(dinv, ZZZ[s])), out_aff + 64 * s);        // X / ZZ
        pr::fq_to_bytes(pr::fq_mul(Y[s], pr::fq_mul(dinv, ZZ[s])), out_aff + 64 * s + 32);   // Y / ZZZ
    }
    return H2AGG_OK;
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
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

}  // extern "C"
