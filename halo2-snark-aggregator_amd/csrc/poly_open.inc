// KZG openings, host side (included into h2agg.hip: shares the context internals; kernels and bounds in poly_kernels.hpp,
// level plan and checks in fr_host.inc, staging in host.inc, power tables in fr_fft.inc): h2agg_fr_poly_eval[_device],
// h2agg_fr_poly_divide[_device], h2agg_kzg_multiopen[_device].  They stand for halo2_proofs' eval_polynomial, kate_division and
// the GWC multiopen prover — an unvendored git dependency of the reference, recalled from upstream (DESIGN.md section 2); the
// yardstick is the definition in include/h2agg.h.  Which W a verifier accepts is pinned by
// halo2-snark-aggregator-api/src/systems/halo2/multiopen.rs:23-69.

namespace {

constexpr size_t POLY_MAX_QUERIES = 65535;   // a grid dimension of the linear combination; chunks * queries stays < 2^31

// the levels of one call: 2^k coefficients per query; the top level is the nq values a(z)
FrLevelPlan poly_plan(const h2agg_ctx* c, unsigned k, size_t nq) {
    return fr_level_plan(c->dbg_fr_poly_chunk ? (unsigned)c->dbg_fr_poly_chunk : FR_CHUNK_LOG, (size_t)1 << k, nq);
}

// tab[l][p]: the powers (z_p^(T^l))^(2^j), j < t (and j = t where the table has room), as the device's Montgomery form
void poly_point_tables(const std::vector<ph::HFr>& pts, const FrLevelPlan& plan, std::vector<std::vector<FrPolyPoint>>& tab) {
    tab.assign(plan.launches(), std::vector<FrPolyPoint>(pts.size()));
    for (size_t p = 0; p < pts.size(); ++p) {
        ph::HFr b = pts[p];
        for (size_t l = 0; l < plan.launches(); ++l) {
            memset(&tab[l][p], 0, sizeof(FrPolyPoint));
            for (unsigned j = 0; j < plan.t; ++j) {
                hfr_words(ph::mul(b, fr_radix()), tab[l][p].pw[j]);
                b = ph::mul(b, b);
            }
            // (the carry fold reads z^8 = pw[3]: at t = 3 that is the next level's base)
            if (plan.t < FR_CHUNK_LOG) hfr_words(ph::mul(b, fr_radix()), tab[l][p].pw[plan.t]);
        }
    }
}

// one level of either sweep: a launch per FR_POLY_POINTS points of `pts`, every launch over all queries.  `pts` holds only
// points that a query of the call names (poly_eval_run compacts the caller's array, multiopen_run passes its groups')
template <class Kernel>
void poly_level_launch(h2agg_ctx* c, Kernel kernel, FrPolyArgs& a, const std::vector<FrPolyPoint>& pts, size_t nq) {
    for (size_t p0 = 0; p0 < pts.size(); p0 += FR_POLY_POINTS) {
        memset(a.pt, 0, sizeof(a.pt));
        for (size_t s = 0; s < FR_POLY_POINTS && p0 + s < pts.size(); ++s) a.pt[s] = pts[p0 + s];
        a.pt0 = (uint32_t)p0;
        hipLaunchKernelGGL(kernel, dim3((unsigned)(nq * a.chunks)), dim3(FR_CHUNK_THREADS), 0, c->stream, a);
    }
}

// Queues the up-sweep: the values a_q(z_q) end up at poly_top(c, plan).  d_desc: null (query q = polynomial q of the slab at
// point q) or nq x {polynomial, point} in device memory.
void poly_eval_queue(h2agg_ctx* c, const uint8_t* d_slab, const uint32_t* d_desc, const FrLevelPlan& plan,
                     const std::vector<std::vector<FrPolyPoint>>& tab) {
    uint8_t* work = (uint8_t*)c->poly_work.p;
    for (size_t l = 0; l < plan.launches(); ++l) {
        FrPolyArgs a;
        a.src = l == 0 ? d_slab : work + 32 * plan.off[l];
        a.dst = work + 32 * plan.off[l + 1];
        a.carry = nullptr;
        a.desc = d_desc;
        a.flags = c->d_flags;
        a.n = plan.cnt[l];
        a.chunks = plan.cnt[l + 1];
        a.t = plan.t;
        a.level0 = l == 0;
        poly_level_launch(c, k_fr_poly_chunk_eval, a, tab[l], plan.nq);
    }
}
const uint8_t* poly_top(const h2agg_ctx* c, const FrLevelPlan& plan) { return (const uint8_t*)c->poly_work.p + 32 * plan.off.back(); }
// the carries into the chunks of the coefficients, [query][plan.cnt[1]], once the levels above are divided; null: one chunk
const uint8_t* poly_carries(const h2agg_ctx* c, const FrLevelPlan& plan) {
    return plan.launches() > 1 ? (const uint8_t*)c->poly_work.p + 32 * plan.off[1] : nullptr;
}

// Queues the down-sweep behind poly_eval_queue of the same plan: the quotients go to d_quot, [query][2^k] (d_quot == d_slab
// allowed when query q is polynomial q: poly_kernels.hpp says why).  The levels above the coefficients are divided in place.
// lowest = 1 stops above the coefficients (shplonk.inc: its leaf kernel takes the carries at poly_carries from there).
void poly_divide_queue(h2agg_ctx* c, const uint8_t* d_slab, const uint32_t* d_desc, const FrLevelPlan& plan,
                       const std::vector<std::vector<FrPolyPoint>>& tab, uint8_t* d_quot, size_t lowest = 0) {
    uint8_t* work = (uint8_t*)c->poly_work.p;
    for (size_t l = plan.launches(); l-- > lowest;) {
        FrPolyArgs a;
        a.src = l == 0 ? d_slab : work + 32 * plan.off[l];
        a.dst = l == 0 ? d_quot : work + 32 * plan.off[l];
        a.carry = l + 1 == plan.launches() ? nullptr : work + 32 * plan.off[l + 1];
        a.desc = d_desc;
        a.flags = c->d_flags;
        a.n = plan.cnt[l];
        a.chunks = plan.cnt[l + 1];
        a.t = plan.t;
        a.level0 = l == 0;
        poly_level_launch(c, k_fr_poly_chunk_divide, a, tab[l], plan.nq);
    }
}

// what every entry point with a query list refuses; on success the points as field elements
int poly_check_queries(h2agg_ctx* c, unsigned k, size_t npoly, const uint32_t* queries, size_t nq, const uint8_t* points,
                       size_t npoints, std::vector<ph::HFr>* pts) {
    TRY(fr_check_k(c, k));
    if (!queries || !points) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    if (nq == 0) return fail(c, H2AGG_ERR_INVALID, "no queries");
    if (nq > POLY_MAX_QUERIES) return fail(c, H2AGG_ERR_INVALID, "more than 65535 queries in one call");
    if (npoly > ((size_t)1 << 32) - 1 || npoints > ((size_t)1 << 32) - 1) return fail(c, H2AGG_ERR_INVALID, "count out of range");
    for (size_t q = 0; q < nq; ++q) {
        if (queries[2 * q] >= npoly) return fail(c, H2AGG_ERR_INVALID, "query names a polynomial index >= npoly");
        if (queries[2 * q + 1] >= npoints) return fail(c, H2AGG_ERR_INVALID, "query names a point index >= npoints");
    }
    pts->resize(npoints);
    for (size_t p = 0; p < npoints; ++p) TRY(fr_parse(c, points + 32 * p, &(*pts)[p]));
    return H2AGG_OK;
}

int poly_eval_run(h2agg_ctx* c, const uint8_t* d_polys, unsigned k, const uint32_t* queries, size_t nq,
                  const std::vector<ph::HFr>& pts, uint8_t* out) {
    // Points that no query names get no power table and no launch: the queries go to the device with the point's rank
    // among the named ones (first seen first) in the point index's place.  `desc` lives until finish() has synchronised.
    std::vector<uint32_t> desc(queries, queries + 2 * nq);
    std::vector<int64_t> rank(pts.size(), -1);
    std::vector<ph::HFr> named;
    for (size_t q = 0; q < nq; ++q) {
        int64_t& r = rank[desc[2 * q + 1]];
        if (r < 0) {
            r = (int64_t)named.size();
            named.push_back(pts[desc[2 * q + 1]]);
        }
        desc[2 * q + 1] = (uint32_t)r;
    }
    const FrLevelPlan plan = poly_plan(c, k, nq);
    std::vector<std::vector<FrPolyPoint>> tab;
    poly_point_tables(named, plan, tab);
    TRY(ensure(c, c->poly_work, 32 * plan.total));
    TRY(ensure(c, c->poly_desc, 8 * nq));
    HIP_TRY(c, hipMemcpyAsync(c->poly_desc.p, desc.data(), 8 * nq, hipMemcpyHostToDevice, c->stream));
    poly_eval_queue(c, d_polys, (const uint32_t*)c->poly_desc.p, plan, tab);
    HIP_TRY(c, hipGetLastError());
    return stage_out(c, out, poly_top(c, plan), 32 * nq);
}

// up-sweep, down-sweep and the remainder of ONE polynomial; nothing synchronises unless the work buffer has to grow
int poly_divide_queue_one(h2agg_ctx* c, const uint8_t* d_poly, unsigned k, const ph::HFr& z, uint8_t* d_quot, uint8_t* d_rem) {
    const FrLevelPlan plan = poly_plan(c, k, 1);
    std::vector<std::vector<FrPolyPoint>> tab;
    poly_point_tables(std::vector<ph::HFr>(1, z), plan, tab);
    TRY(ensure(c, c->poly_work, 32 * plan.total));
    poly_eval_queue(c, d_poly, nullptr, plan, tab);
    poly_divide_queue(c, d_poly, nullptr, plan, tab, d_quot);
    HIP_TRY(c, hipGetLastError());
    if (d_rem) HIP_TRY(c, hipMemcpyAsync(d_rem, poly_top(c, plan), 32, hipMemcpyDeviceToDevice, c->stream));
    return H2AGG_OK;
}

int poly_divide_check(h2agg_ctx* c, unsigned k, const uint8_t* z, ph::HFr* zf) {
    TRY(fr_check_k(c, k));
    if (!z) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    return fr_parse(c, z, zf);
}

int multiopen_run(h2agg_ctx* c, uint64_t g_handle, const uint8_t* d_polys, unsigned k, const uint32_t* queries, size_t nq,
                  const std::vector<ph::HFr>& pts, const ph::HFr& v, uint8_t* w_aff, uint32_t* group_points, size_t* ngroups) {
    const size_t n = (size_t)1 << k;
    // grouping (multiopen.rs:31-43 with the point index in the rotation's role): one group per distinct point, first seen first
    std::vector<uint32_t> gpoint;
    std::vector<std::vector<uint32_t>> members;
    std::vector<int64_t> group_of(pts.size(), -1);
    for (size_t q = 0; q < nq; ++q) {
        const uint32_t pt = queries[2 * q + 1];
        if (group_of[pt] < 0) {
            group_of[pt] = (int64_t)gpoint.size();
            gpoint.push_back(pt);
            members.emplace_back();
        }
        members[(size_t)group_of[pt]].push_back(queries[2 * q]);
    }
    const size_t groups = gpoint.size();
    // device lists: the members of every group, highest power of v first, then the group offsets
    std::vector<uint32_t> lists;
    std::vector<uint32_t> goff(1, 0);
    std::vector<ph::HFr> gz(groups);
    for (size_t g = 0; g < groups; ++g) {
        lists.insert(lists.end(), members[g].rbegin(), members[g].rend());
        goff.push_back((uint32_t)lists.size());
        gz[g] = pts[gpoint[g]];
    }
    lists.insert(lists.end(), goff.begin(), goff.end());
    const FrLevelPlan plan = poly_plan(c, k, groups);
    std::vector<std::vector<FrPolyPoint>> tab;
    poly_point_tables(gz, plan, tab);
    TRY(ensure(c, c->poly_work, 32 * plan.total));
    TRY(ensure(c, c->poly_desc, 4 * lists.size()));
    TRY(ensure(c, c->poly_slab, 32 * n * groups));
    TRY(ensure(c, c->poly_jac, 96 * groups));
    HIP_TRY(c, hipMemcpyAsync(c->poly_desc.p, lists.data(), 4 * lists.size(), hipMemcpyHostToDevice, c->stream));
    enum { COMBINE, DIVIDE, COMMIT };
    PhaseClock phases(c);
    phases.mark(COMBINE);
    FrLincombArgs la;
    hfr_words(ph::mul(v, fr_radix()), la.v);
    la.polys = d_polys;
    la.dst = (uint8_t*)c->poly_slab.p;
    la.list = (const uint32_t*)c->poly_desc.p;
    la.goff = la.list + nq;
    la.flags = c->d_flags;
    la.n = (uint32_t)n;
    hipLaunchKernelGGL(k_fr_poly_lincomb, dim3((unsigned)((n + BLOCK - 1) / BLOCK), (unsigned)groups), dim3(BLOCK), 0, c->stream, la);
    phases.mark(DIVIDE);
    poly_eval_queue(c, la.dst, nullptr, plan, tab);
    poly_divide_queue(c, la.dst, nullptr, plan, tab, la.dst);
    phases.mark(COMMIT);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // `lists` has crossed: pageable memory may still be read until here
    TRY(h2agg_g1_msm_device_batch_async(c, g_handle, c->poly_slab.p, n, groups, c->poly_jac.p));
    TRY(h2agg_g1_batch_to_affine_device(c, (const uint8_t*)c->poly_jac.p, groups, w_aff));   // joins, synchronises, reports the flags
    phases.mark(PhaseClock::END);
    static const char* const names[3] = {"combine", "divide", "commit"};
    phases.report(names, 3);
    for (size_t g = 0; g < groups; ++g) group_points[g] = gpoint[g];
    *ngroups = groups;
    return H2AGG_OK;
}

int multiopen_check(h2agg_ctx* c, uint64_t g_handle, unsigned k, size_t npoly, const uint32_t* queries, size_t nq,
                    const uint8_t* points, size_t npoints, const uint8_t* v, const void* w_aff, const void* group_points,
                    const void* ngroups, std::vector<ph::HFr>* pts, ph::HFr* vf) {
    if (!v || !w_aff || !group_points || !ngroups) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(poly_check_queries(c, k, npoly, queries, nq, points, npoints, pts));
    TRY(fr_parse(c, v, vf));
    Table* g = nullptr;
    TRY(find_table(c, g_handle, &g));
    if (g->n < ((size_t)1 << k)) return fail(c, H2AGG_ERR_INVALID, "the base table is shorter than 2^k");
    return H2AGG_OK;
}

}  // namespace

extern "C" {

int h2agg_fr_poly_eval_device(h2agg_ctx* c, const void* d_polys, size_t npoly, unsigned k, const uint32_t* queries, size_t nq,
                              const uint8_t* points, size_t npoints, uint8_t* out) try {
    TRY(bind(c));
    if (!d_polys || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    std::vector<ph::HFr> pts;
    TRY(poly_check_queries(c, k, npoly, queries, nq, points, npoints, &pts));
    TRY(clear_flags(c));
    return poly_eval_run(c, (const uint8_t*)d_polys, k, queries, nq, pts, out);
} API_CATCH

int h2agg_fr_poly_eval(h2agg_ctx* c, const uint8_t* polys, size_t npoly, unsigned k, const uint32_t* queries, size_t nq,
                       const uint8_t* points, size_t npoints, uint8_t* out) try {
    TRY(bind(c));
    if (!polys || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    std::vector<ph::HFr> pts;
    TRY(poly_check_queries(c, k, npoly, queries, nq, points, npoints, &pts));
    const size_t bytes = ((size_t)32 << k) * npoly;
    TRY(ensure(c, c->in_a, bytes));
    TRY(stage_in(c, c->in_a, polys, bytes));
    TRY(clear_flags(c));
    return poly_eval_run(c, (const uint8_t*)c->in_a.p, k, queries, nq, pts, out);
} API_CATCH

int h2agg_fr_poly_divide_device(h2agg_ctx* c, const void* d_poly, unsigned k, const uint8_t z[32], void* d_quot, void* d_rem) try {
    TRY(bind(c));
    if (!d_poly || !d_quot) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    ph::HFr zf;
    TRY(poly_divide_check(c, k, z, &zf));
    return poly_divide_queue_one(c, (const uint8_t*)d_poly, k, zf, (uint8_t*)d_quot, (uint8_t*)d_rem);
} API_CATCH

int h2agg_fr_poly_divide(h2agg_ctx* c, const uint8_t* in, unsigned k, const uint8_t z[32], uint8_t* out, uint8_t rem[32]) try {
    TRY(bind(c));
    if (!in || !out || !rem) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    ph::HFr zf;
    TRY(poly_divide_check(c, k, z, &zf));
    const size_t bytes = (size_t)32 << k;
    TRY(ensure(c, c->in_a, bytes + 32));
    uint8_t* d = (uint8_t*)c->in_a.p;
    TRY(stage_in(c, c->in_a, in, bytes));
    TRY(clear_flags(c));
    TRY(poly_divide_queue_one(c, d, k, zf, d, d + bytes));
    HIP_TRY(c, hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, c->stream));
    return stage_out(c, rem, d + bytes, 32);
} API_CATCH

int h2agg_kzg_multiopen_device(h2agg_ctx* c, uint64_t g_handle, const void* d_polys, size_t npoly, unsigned k,
                               const uint32_t* queries, size_t nq, const uint8_t* points, size_t npoints, const uint8_t v[32],
                               uint8_t* w_aff, uint32_t* group_points, size_t* ngroups) try {
    TRY(bind(c));
    if (!d_polys) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    std::vector<ph::HFr> pts;
    ph::HFr vf;
    TRY(multiopen_check(c, g_handle, k, npoly, queries, nq, points, npoints, v, w_aff, group_points, ngroups, &pts, &vf));
    TRY(clear_flags(c));
    return multiopen_run(c, g_handle, (const uint8_t*)d_polys, k, queries, nq, pts, vf, w_aff, group_points, ngroups);
} API_CATCH

int h2agg_kzg_multiopen(h2agg_ctx* c, uint64_t g_handle, const uint8_t* polys, size_t npoly, unsigned k, const uint32_t* queries,
                        size_t nq, const uint8_t* points, size_t npoints, const uint8_t v[32], uint8_t* w_aff,
                        uint32_t* group_points, size_t* ngroups) try {
    TRY(bind(c));
    if (!polys) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    std::vector<ph::HFr> pts;
    ph::HFr vf;
    TRY(multiopen_check(c, g_handle, k, npoly, queries, nq, points, npoints, v, w_aff, group_points, ngroups, &pts, &vf));
    const size_t bytes = ((size_t)32 << k) * npoly;
    TRY(ensure(c, c->in_a, bytes));
    TRY(stage_in(c, c->in_a, polys, bytes));
    TRY(clear_flags(c));
    return multiopen_run(c, g_handle, (const uint8_t*)c->in_a.p, k, queries, nq, pts, vf, w_aff, group_points, ngroups);
} API_CATCH

}  // extern "C"
