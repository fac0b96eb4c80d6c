// The Shplonk (BDFG20) multiopen prover, host side (included into h2agg.hip behind poly_open.inc: shares the context internals
// and that family's level plan, power tables and sweeps; kernels and bounds in shplonk_kernels.hpp; checks, growing buffers
// and staging in host.inc / fr_host.inc): h2agg_kzg_shplonk_begin / _finish / _destroy.  They stand for halo2_proofs'
// poly/kzg/multiopen/shplonk/prover.rs and construct_intermediate_sets — an unvendored git dependency of the reference,
// recalled from upstream (DESIGN.md section 2); the yardstick is the definition in include/h2agg.h.

namespace {

struct ShplonkSet {
    std::vector<uint32_t> points;   // S_i: point indices, in the order the set's first polynomial first names them
    std::vector<uint32_t> polys;    // p_{i,0}, p_{i,1}, ...: in the order of their first queries
    std::vector<std::vector<ph::HFr>> evals;   // [j][s]: the value of p_{i,j} at points[s]
    std::vector<uint32_t> first_query;         // [j]: the first query that names p_{i,j} (for messages)
    std::vector<ph::HFr> corr;      // sum_j y^j r_{i,j}: |S_i| coefficients
    std::vector<ph::HFr> omega;     // [s]: 1 / prod_{s' != s} (z_s - z_s')
};

}  // namespace

// What begin keeps for finish: the resident slab with h(X) behind it, one more array, the sets.  It refers to its context,
// which must outlive it.
struct h2agg_shplonk {
    h2agg_ctx* ctx = nullptr;
    int device = 0;
    uint64_t g_handle = 0;
    unsigned k = 0;
    size_t npoly = 0;
    DevBuf slab;    // [npoly + 1][2^k]: the polynomials, then h
    DevBuf num;     // [2^k]: N_i of the set in work; L of round 2, then its quotient
    DevBuf lists;   // the call's lists, weights, corrections and small results (ShplonkBlob)
    std::vector<ShplonkSet> sets;
    std::vector<ph::HFr> pts;       // the caller's points
    std::vector<uint32_t> named;    // T: the point indices some query names, first seen first
    ph::HFr y, v;
    uint8_t* h() const { return (uint8_t*)slab.p + ((size_t)32 << k) * npoly; }
};

namespace {

// One host block per call, copied to the device once: u32 words; the kernels' arguments point into its device copy.
struct ShplonkBlob {
    std::vector<uint32_t> w;
    size_t words(size_t n) {   // reserves n words, 8-word aligned -> their offset
        const size_t at = w.size();
        w.resize(at + ((n + 7) & ~(size_t)7), 0);
        return at;
    }
    void put(size_t at, const ph::HFr& x) { hfr_words(x, &w[at]); }
    void put_mont(size_t at, const ph::HFr& x) { hfr_words(ph::mul(x, fr_radix()), &w[at]); }
};

bool hfr_less(const ph::HFr& a, const ph::HFr& b) {   // any total order: equal values end up adjacent
    for (int i = 3; i >= 0; --i)
        if (a.l[i] != b.l[i]) return a.l[i] < b.l[i];
    return false;
}
bool hfr_eq(const ph::HFr& a, const ph::HFr& b) { return !memcmp(a.l, b.l, 32); }

ph::HFr hfr_horner(const std::vector<ph::HFr>& a, const ph::HFr& x) {
    ph::HFr r = ph::zero();
    for (size_t i = a.size(); i-- > 0;) r = ph::add(ph::mul(r, x), a[i]);
    return r;
}

// The sets of include/h2agg.h from the queries and their values.  Refuses a repeated pair with two values, equal values
// under two named point indices, a set of more than SHPLONK_MAX_SET points.
int shplonk_sets(h2agg_ctx* c, h2agg_shplonk* o, size_t npoly, const uint32_t* queries, size_t nq, const std::vector<ph::HFr>& ev) {
    std::vector<int64_t> slot(npoly, -1);   // polynomial -> its place in `order`
    std::vector<uint32_t> order;            // polynomials, first seen first
    std::vector<std::vector<uint32_t>> ppts;
    std::vector<std::vector<ph::HFr>> pev;
    std::vector<uint32_t> pfirst;
    std::vector<bool> seen(o->pts.size(), false);
    for (size_t q = 0; q < nq; ++q) {
        const uint32_t m = queries[2 * q], pt = queries[2 * q + 1];
        if (!seen[pt]) {
            seen[pt] = true;
            o->named.push_back(pt);
        }
        if (slot[m] < 0) {
            slot[m] = (int64_t)order.size();
            order.push_back(m);
            ppts.emplace_back();
            pev.emplace_back();
            pfirst.push_back((uint32_t)q);
        }
        std::vector<uint32_t>& mine = ppts[(size_t)slot[m]];
        const auto at = std::find(mine.begin(), mine.end(), pt);
        if (at != mine.end()) {
            if (!hfr_eq(pev[(size_t)slot[m]][(size_t)(at - mine.begin())], ev[q]))
                return fail(c, H2AGG_ERR_INVALID, "shplonk: query " + std::to_string(q) + " repeats a (polynomial, point) pair with another value");
            continue;
        }
        if (mine.size() == SHPLONK_MAX_SET) return fail(c, H2AGG_ERR_INVALID, "shplonk: a polynomial is opened at more than 32 points");
        mine.push_back(pt);
        pev[(size_t)slot[m]].push_back(ev[q]);
    }
    std::vector<uint32_t> byval(o->named);
    std::sort(byval.begin(), byval.end(), [&](uint32_t a, uint32_t b) { return hfr_less(o->pts[a], o->pts[b]); });
    for (size_t i = 1; i < byval.size(); ++i)
        if (hfr_eq(o->pts[byval[i - 1]], o->pts[byval[i]]))
            return fail(c, H2AGG_ERR_INVALID, "shplonk: point indices " + std::to_string(std::min(byval[i - 1], byval[i])) + " and " +
                                                  std::to_string(std::max(byval[i - 1], byval[i])) + " hold one value");
    std::map<std::vector<uint32_t>, size_t> by_points;   // the sorted point indices -> the set
    for (size_t a = 0; a < order.size(); ++a) {
        std::vector<uint32_t> key(ppts[a]);
        std::sort(key.begin(), key.end());
        auto it = by_points.find(key);
        if (it == by_points.end()) {
            it = by_points.emplace(key, o->sets.size()).first;
            o->sets.emplace_back();
            o->sets.back().points = ppts[a];
        }
        ShplonkSet& s = o->sets[it->second];
        std::vector<ph::HFr> e(s.points.size());   // in the set's order of points
        for (size_t i = 0; i < s.points.size(); ++i)
            e[i] = pev[a][(size_t)(std::find(ppts[a].begin(), ppts[a].end(), s.points[i]) - ppts[a].begin())];
        s.polys.push_back(order[a]);
        s.evals.push_back(std::move(e));
        s.first_query.push_back(pfirst[a]);
    }
    return H2AGG_OK;
}

// omega_s and corr = sum_j y^j r_{i,j} of every set: r is interpolated once per set, over the y-combination of the values
void shplonk_interpolate(h2agg_shplonk* o) {
    for (ShplonkSet& s : o->sets) {
        const size_t m = s.points.size();
        std::vector<ph::HFr> z(m), e(m, ph::zero());
        for (size_t i = 0; i < m; ++i) z[i] = o->pts[s.points[i]];
        ph::HFr yj = ph::one();
        for (size_t j = 0; j < s.polys.size(); ++j) {
            for (size_t i = 0; i < m; ++i) e[i] = ph::add(e[i], ph::mul(yj, s.evals[j][i]));
            yj = ph::mul(yj, o->y);
        }
        std::vector<ph::HFr> zs(m + 1, ph::zero());   // Z_S(X)
        zs[0] = ph::one();
        for (size_t i = 0; i < m; ++i) {   // times (X - z_i), in place from the top
            for (size_t d = i + 1; d > 0; --d) zs[d] = ph::sub(zs[d - 1], ph::mul(zs[d], z[i]));
            zs[0] = ph::sub(ph::zero(), ph::mul(zs[0], z[i]));
        }
        s.omega.assign(m, ph::one());
        s.corr.assign(m, ph::zero());
        for (size_t i = 0; i < m; ++i) {
            ph::HFr den = ph::one();
            for (size_t b = 0; b < m; ++b)
                if (b != i) den = ph::mul(den, ph::sub(z[i], z[b]));
            s.omega[i] = ph::inv(den);   // the named points are distinct: den != 0
            const ph::HFr f = ph::mul(e[i], s.omega[i]);
            ph::HFr hi = ph::zero();     // Z_S / (X - z_i), top down
            for (size_t d = m; d-- > 0;) {
                hi = ph::add(zs[d + 1], ph::mul(hi, z[i]));
                s.corr[d] = ph::add(s.corr[d], ph::mul(f, hi));
            }
        }
    }
}

void shplonk_wsum_launch(h2agg_ctx* c, h2agg_shplonk* o, size_t idx_at, size_t w_at, size_t ncorr_at, size_t nterms) {
    const size_t n = (size_t)1 << o->k;
    const uint32_t* d = (const uint32_t*)o->lists.p;
    FrWsumArgs a;
    a.polys = (const uint8_t*)o->slab.p;
    a.dst = (uint8_t*)o->num.p;
    a.idx = d + idx_at;
    a.w = d + w_at;
    a.ncorr = d + ncorr_at;
    a.flags = c->d_flags;
    a.nterms = (uint32_t)nterms;
    a.n = (uint32_t)n;
    hipLaunchKernelGGL(k_fr_poly_wsum, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream, a);
}

// the commitment of n coefficients at d_coeffs, as a canonical affine point; synchronises and reports the flags
int shplonk_commit(h2agg_ctx* c, h2agg_shplonk* o, const void* d_coeffs, uint8_t aff[64]) {
    TRY(ensure(c, c->poly_jac, 96));
    TRY(h2agg_g1_msm_device_batch_async(c, o->g_handle, d_coeffs, (size_t)1 << o->k, 1, c->poly_jac.p));
    return h2agg_g1_batch_to_affine_device(c, (const uint8_t*)c->poly_jac.p, 1, aff);
}

// Some N_i(z) != 0: which query's value is not its polynomial's?  (The slow way, on the refusal only: every query evaluated.)
int shplonk_name_mismatch(h2agg_ctx* c, h2agg_shplonk* o, const uint32_t* queries, size_t nq, const uint8_t* evals) {
    std::vector<uint8_t> got(32 * nq);
    TRY(clear_flags(c));
    TRY(poly_eval_run(c, (const uint8_t*)o->slab.p, o->k, queries, nq, o->pts, got.data()));
    for (size_t q = 0; q < nq; ++q)
        if (memcmp(&got[32 * q], evals + 32 * q, 32))
            return fail(c, H2AGG_ERR_INVALID, "shplonk: the value of query " + std::to_string(q) + " (polynomial " + std::to_string(queries[2 * q]) +
                                                  ", point " + std::to_string(queries[2 * q + 1]) + ") is not its polynomial's");
    return fail(c, H2AGG_ERR_INVALID, "shplonk: a numerator does not vanish on its point set");
}

// polys: the slab [npoly][2^k] on the host, or with `resident` in device memory (a column store's columns): the object's own
// slab is filled by stage_in or by a device copy, so the source is free once the call has returned
int shplonk_begin_run(h2agg_ctx* c, h2agg_shplonk* o, const uint8_t* polys, bool resident, const uint32_t* queries, size_t nq,
                      const uint8_t* evals, uint8_t* h1_aff) {
    const size_t n = (size_t)1 << o->k, bytes = 32 * n;
    shplonk_interpolate(o);
    // the call's block: per set the list and weights of N_i, -corr, the queries (N_i, z) of the sweeps; the top values
    struct At {
        size_t idx, w, ncorr, desc, top;
    };
    ShplonkBlob blob;
    std::vector<At> at(o->sets.size());
    size_t most_points = 0, tops = 0;
    for (size_t i = 0; i < o->sets.size(); ++i) {
        const ShplonkSet& s = o->sets[i];
        const size_t np = s.polys.size(), m = s.points.size();
        at[i] = {blob.words(np), blob.words(8 * np), blob.words(8 * SHPLONK_MAX_SET), blob.words(2 * m), tops};
        ph::HFr yj = ph::one();
        for (size_t j = 0; j < np; ++j) {
            blob.w[at[i].idx + j] = s.polys[j];
            blob.put_mont(at[i].w + 8 * j, yj);
            yj = ph::mul(yj, o->y);
        }
        for (size_t d = 0; d < m; ++d) blob.put(at[i].ncorr + 8 * d, ph::sub(ph::zero(), s.corr[d]));
        for (size_t q = 0; q < m; ++q) blob.w[at[i].desc + 2 * q + 1] = (uint32_t)q;   // {polynomial 0 = N_i, point q of the set}
        most_points = std::max(most_points, m);
        tops += m;
    }
    const size_t top_at = blob.words(8 * tops);
    TRY(ensure(c, o->slab, bytes * (o->npoly + 1)));
    TRY(ensure(c, o->num, bytes));
    TRY(ensure(c, o->lists, 4 * blob.w.size()));
    TRY(ensure(c, c->poly_work, 32 * poly_plan(c, o->k, most_points).total));
    enum { STAGE, NUMERATORS, DIVIDE, COMMIT };
    PhaseClock phases(c);
    phases.mark(STAGE);
    if (resident)
        HIP_TRY(c, hipMemcpyAsync(o->slab.p, polys, bytes * o->npoly, hipMemcpyDeviceToDevice, c->stream));
    else
        TRY(stage_in(c, o->slab, polys, bytes * o->npoly));
    TRY(stage_in(c, o->lists, (const uint8_t*)blob.w.data(), 4 * blob.w.size()));
    TRY(clear_flags(c));
    const uint32_t* d_lists = (const uint32_t*)o->lists.p;
    ph::HFr vi = ph::one();
    for (size_t i = 0; i < o->sets.size(); ++i) {
        const ShplonkSet& s = o->sets[i];
        const size_t m = s.points.size();
        phases.mark(NUMERATORS);
        shplonk_wsum_launch(c, o, at[i].idx, at[i].w, at[i].ncorr, s.polys.size());
        phases.mark(DIVIDE);
        const FrLevelPlan plan = poly_plan(c, o->k, m);
        std::vector<ph::HFr> z(m);
        for (size_t q = 0; q < m; ++q) z[q] = o->pts[s.points[q]];
        std::vector<std::vector<FrPolyPoint>> tab;
        poly_point_tables(z, plan, tab);
        const uint32_t* d_desc = d_lists + at[i].desc;
        poly_eval_queue(c, (const uint8_t*)o->num.p, d_desc, plan, tab);
        HIP_TRY(c, hipMemcpyAsync((uint8_t*)o->lists.p + 4 * top_at + 32 * at[i].top, poly_top(c, plan), 32 * m, hipMemcpyDeviceToDevice,
                                  c->stream));
        poly_divide_queue(c, (const uint8_t*)o->num.p, d_desc, plan, tab, nullptr, 1);
        for (size_t q0 = 0; q0 < m; q0 += SHPLONK_CHAINS) {
            FrShplonkLeafArgs a;
            memset(&a, 0, sizeof a);
            a.npts = (uint32_t)std::min<size_t>(SHPLONK_CHAINS, m - q0);
            for (uint32_t r = 0; r < a.npts; ++r) {
                a.pt[r] = tab[0][q0 + r];
                hfr_words(ph::mul(ph::mul(s.omega[q0 + r], vi), fr_radix()), a.wz[r]);
            }
            a.src = (const uint8_t*)o->num.p;
            a.dst = o->h();
            a.carry = poly_carries(c, plan);
            a.q0 = (uint32_t)q0;
            a.n = (uint32_t)n;
            a.chunks = plan.cnt[1];
            a.t = plan.t;
            a.accumulate = i > 0 || q0 > 0;   // the first launch of the call writes h
            hipLaunchKernelGGL(k_fr_shplonk_leaf, dim3(a.chunks), dim3(FR_CHUNK_THREADS), 0, c->stream, a);
        }
        vi = ph::mul(vi, o->v);
    }
    phases.mark(COMMIT);   // (with the read-back of the divisions' remainders)
    HIP_TRY(c, hipGetLastError());
    std::vector<uint8_t> top(32 * tops);
    TRY(stage_out(c, top.data(), (const uint8_t*)o->lists.p + 4 * top_at, 32 * tops));   // synchronises: `blob` has crossed
    for (uint8_t b : top)
        if (b) return shplonk_name_mismatch(c, o, queries, nq, evals);
    TRY(shplonk_commit(c, o, o->h(), h1_aff));
    phases.mark(PhaseClock::END);
    static const char* const names[4] = {"stage", "numerators", "divide", "commit"};
    phases.report(names, 4);
    return H2AGG_OK;
}

int shplonk_finish_run(h2agg_ctx* c, h2agg_shplonk* o, const ph::HFr& u, uint8_t* h2_aff) {
    // d_i = Z_{T \ S_i}(u); c_i = d_i / d_0; t = Z_T(u) / d_0
    std::vector<ph::HFr> d(o->sets.size());
    std::vector<bool> in_set(o->pts.size());
    ph::HFr zt = ph::one();
    for (uint32_t p : o->named) zt = ph::mul(zt, ph::sub(u, o->pts[p]));
    for (size_t i = 0; i < o->sets.size(); ++i) {
        in_set.assign(o->pts.size(), false);
        for (uint32_t p : o->sets[i].points) in_set[p] = true;
        d[i] = ph::one();
        for (uint32_t p : o->named)
            if (!in_set[p]) d[i] = ph::mul(d[i], ph::sub(u, o->pts[p]));
    }
    if (ph::is_zero(d[0])) return fail(c, H2AGG_ERR_INVALID, "shplonk: u is a point of another set than the first (d_0 == 0)");
    const ph::HFr d0_inv = ph::inv(d[0]);
    // L + t h = sum_i v^i c_i (sum_j y^j p_{i,j} - corr_i(u)): the list, with h under -t at its end, and the constant
    ShplonkBlob blob;
    size_t nterms = 1;
    for (const ShplonkSet& s : o->sets) nterms += s.polys.size();
    const size_t idx_at = blob.words(nterms), w_at = blob.words(8 * nterms), ncorr_at = blob.words(8 * SHPLONK_MAX_SET),
                 rem_at = blob.words(8);
    ph::HFr vi = ph::one(), constant = ph::zero();
    size_t term = 0;
    for (size_t i = 0; i < o->sets.size(); ++i) {
        const ShplonkSet& s = o->sets[i];
        ph::HFr wj = ph::mul(vi, ph::mul(d[i], d0_inv));
        constant = ph::add(constant, ph::mul(wj, hfr_horner(s.corr, u)));
        for (size_t j = 0; j < s.polys.size(); ++j, ++term) {
            blob.w[idx_at + term] = s.polys[j];
            blob.put_mont(w_at + 8 * term, wj);
            wj = ph::mul(wj, o->y);
        }
        vi = ph::mul(vi, o->v);
    }
    blob.w[idx_at + term] = (uint32_t)o->npoly;   // h, the row behind the polynomials
    blob.put_mont(w_at + 8 * term, ph::sub(ph::zero(), ph::mul(zt, d0_inv)));
    blob.put(ncorr_at, ph::sub(ph::zero(), constant));
    TRY(ensure(c, o->lists, 4 * blob.w.size()));
    enum { COMBINE, DIVIDE, COMMIT };
    PhaseClock phases(c);
    TRY(stage_in(c, o->lists, (const uint8_t*)blob.w.data(), 4 * blob.w.size()));
    TRY(clear_flags(c));
    phases.mark(COMBINE);
    shplonk_wsum_launch(c, o, idx_at, w_at, ncorr_at, nterms);
    phases.mark(DIVIDE);
    uint8_t* d_rem = (uint8_t*)o->lists.p + 4 * rem_at;
    TRY(poly_divide_queue_one(c, (const uint8_t*)o->num.p, o->k, u, (uint8_t*)o->num.p, d_rem));
    phases.mark(COMMIT);
    uint8_t rem[32];
    TRY(stage_out(c, rem, d_rem, 32));   // synchronises: `blob` has crossed
    for (uint8_t b : rem)
        if (b) return fail(c, H2AGG_ERR_HIP, "shplonk: internal: L(u) != 0 for values that begin accepted");
    TRY(shplonk_commit(c, o, o->num.p, h2_aff));
    phases.mark(PhaseClock::END);
    static const char* const names[3] = {"combine", "divide", "commit"};
    phases.report(names, 3);
    return H2AGG_OK;
}

// h2agg_kzg_shplonk_begin behind bind(), over a host slab or (resident) a slab in device memory: h2agg_columns_shplonk_begin
int shplonk_begin(h2agg_ctx* c, uint64_t g_handle, const uint8_t* polys, bool resident, size_t npoly, unsigned k, const uint32_t* queries,
                  size_t nq, const uint8_t* points, size_t npoints, const uint8_t* evals, const uint8_t* y, const uint8_t* v,
                  uint8_t* h1_aff, h2agg_shplonk** out) {
    if (out) *out = nullptr;
    if (!polys || !evals || !y || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    std::unique_ptr<h2agg_shplonk> o(new h2agg_shplonk());
    size_t ngroups_unused = 0;
    // (the GWC call's checks: v, the queries, the points, the table; its three outputs stand in as non-null)
    TRY(multiopen_check(c, g_handle, k, npoly, queries, nq, points, npoints, v, h1_aff, &ngroups_unused, &ngroups_unused, &o->pts, &o->v));
    TRY(fr_parse(c, y, &o->y));
    std::vector<ph::HFr> ev(nq);
    for (size_t q = 0; q < nq; ++q) TRY(fr_parse(c, evals + 32 * q, &ev[q]));
    o->ctx = c;
    o->device = c->device;
    o->g_handle = g_handle;
    o->k = k;
    o->npoly = npoly;
    TRY(shplonk_sets(c, o.get(), npoly, queries, nq, ev));
    if (c->dbg_phases) c->last_phases.clear();
    TRY(shplonk_begin_run(c, o.get(), polys, resident, queries, nq, evals, h1_aff));
    *out = o.release();
    return H2AGG_OK;
}

}  // namespace

extern "C" {

int h2agg_kzg_shplonk_begin(h2agg_ctx* c, uint64_t g_handle, const uint8_t* polys, size_t npoly, unsigned k, const uint32_t* queries,
                            size_t nq, const uint8_t* points, size_t npoints, const uint8_t* evals, const uint8_t y[32],
                            const uint8_t v[32], uint8_t h1_aff[64], h2agg_shplonk** out) try {
    TRY(bind(c));
    return shplonk_begin(c, g_handle, polys, false, npoly, k, queries, nq, points, npoints, evals, y, v, h1_aff, out);
} API_CATCH

int h2agg_kzg_shplonk_finish(h2agg_shplonk* o, const uint8_t u[32], uint8_t h2_aff[64]) try {
    if (!o) return H2AGG_ERR_INVALID;
    h2agg_ctx* c = o->ctx;
    TRY(bind(c));
    if (!u || !h2_aff) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    ph::HFr uf;
    TRY(fr_parse(c, u, &uf));
    Table* g = nullptr;
    TRY(find_table(c, o->g_handle, &g));   // (it may have been freed since begin)
    if (c->dbg_phases) c->last_phases.clear();
    return shplonk_finish_run(c, o, uf, h2_aff);
} API_CATCH

void h2agg_kzg_shplonk_destroy(h2agg_shplonk* o) {
    if (!o) return;
    (void)hipSetDevice(o->device);
    delete o;   // hipFree waits for whatever still reads the buffers
}

}  // extern "C"
