// The witness check, host side (included into h2agg.hip behind keygen.inc: shares the context internals, the expression
// compiler of quotient.inc and the sort of lookup.inc; kernels, flag layout and bounds in witness_kernels.hpp, checks in
// fr_host.inc, staging in host.inc): h2agg_witness_check_layout, h2agg_witness_check.  They stand for the gate, lookup and
// permutation checks of halo2_proofs' dev::MockProver::verify — an unvendored git dependency of the reference, recalled from
// upstream (DESIGN.md section 2 and 5.17); the yardstick is the definition in include/h2agg.h.  The order of the constraints
// is pinned by halo2-snark-aggregator-api/src/systems/halo2/params.rs:74-224.
//
// There is no _device twin: the resident form runs over column stores (h2agg_columns_witness_check in csrc/columns.inc,
// DESIGN.md 5.20), on top of wc_check, wc_queue and wc_report_out below.

namespace {

// Flag words of one chunk of constraints: 2^24 words = 64 MiB.  A line is n / 32 words, so at k = 24 a chunk is 32
// constraints, at k <= 19 it is 1024 or more; a key with more gate polynomials or permutation columns than that runs them in
// chunks (one program, one launch and one report per chunk), a lookup is a chunk of its own.
// (The measure build takes another bound from H2AGG_WC_FLAG_WORDS, so that a small key crosses the chunk boundary:
// tools/witness_check_time.py --chunks.)
constexpr size_t WC_FLAG_WORDS = (size_t)1 << 24;

size_t wc_flag_words() {
    const char* v = knob("H2AGG_WC_FLAG_WORDS");
    return v && atoll(v) > 0 ? (size_t)atoll(v) : WC_FLAG_WORDS;
}

// The work memory of one call, cut out of the context's wc_work (offsets in bytes, multiples of 256): the flag lines of a
// chunk, the tile sums and minima of its report, the two theta-folds of a lookup, the report itself.
struct WcLayout {
    uint32_t n, u, zwords, tiles, chunk;   // chunk: most constraints per set of launches
    size_t G, P, L, C, max_rows;
    size_t zflags, sums, mins, fold_a, fold_s, counts, first_rows, total_at, rows, total;
};

WcLayout wc_layout(const h2agg_vk& vk, unsigned what, size_t max_rows) {
    WcLayout l;
    l.n = 1u << vk.k;
    l.u = l.n - vk.blinding_factors - 1u;   // >= 1: h2agg_vk_create refuses blinding_factors + 1 >= n
    l.zwords = 2u * ((l.n + 63u) / 64u);
    l.tiles = (l.zwords + WC_WAVE - 1) / WC_WAVE;
    l.G = 0;
    for (const auto& g : vk.gates) l.G += g.size();
    l.P = vk.perm_cols.size();
    l.L = vk.lookups.size();
    l.C = l.G + l.P + l.L;
    l.max_rows = std::min<size_t>(max_rows, l.n);   // a line never holds more than n rows: the device array is no wider
    size_t most = 0;
    if (what & H2AGG_WC_GATES) most = std::max(most, l.G);
    if (what & H2AGG_WC_PERMUTATION) most = std::max(most, l.P);
    if ((what & H2AGG_WC_LOOKUPS) && l.L) most = std::max<size_t>(most, 1);
    l.chunk = (uint32_t)std::min<size_t>(std::max<size_t>(1, wc_flag_words() / l.zwords), std::max<size_t>(most, 1));
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    };
    l.zflags = take(4 * (size_t)l.chunk * l.zwords);
    l.sums = take(4 * (size_t)l.chunk * l.tiles);
    l.mins = take(4 * (size_t)l.chunk * l.tiles);
    const bool folds = (what & H2AGG_WC_LOOKUPS) && l.L;
    l.fold_a = take(folds ? 32 * (size_t)l.n : 0);
    l.fold_s = take(folds ? 32 * (size_t)l.n : 0);
    l.counts = take(4 * l.C);
    l.first_rows = take(4 * l.C);
    l.total_at = take(8);
    l.rows = take(4 * l.C * l.max_rows);
    l.total = at;
    return l;
}

// everything a call needs that does not depend on where the buffers live: the compiled programs and the parsed scalars
struct WcCall {
    WcLayout l;
    std::vector<QeProgram> gate_progs;     // one per chunk of gate polynomials
    std::vector<QeProgram> lookup_progs;   // per lookup: inputs, tables
    ph::HFr theta;
    bool gates, permutation, lookups;
};

// every refusal of h2agg_witness_check but the mapping's range (the caller scans it where it can read it)
int wc_check(h2agg_ctx* c, const h2agg_vk* vk, unsigned what, const void* advice, const void* fixed, const void* instance,
             const uint8_t* challenges, const uint8_t* theta, const void* mapping, size_t max_rows, const void* counts,
             const void* first_rows, const void* total, WcCall* call) {
    if (!vk) return fail(c, H2AGG_ERR_INVALID, "null verifying key");
    if (what == 0 || (what & ~(unsigned)(H2AGG_WC_GATES | H2AGG_WC_PERMUTATION | H2AGG_WC_LOOKUPS)))
        return fail(c, H2AGG_ERR_INVALID, "what must be a non-empty set of H2AGG_WC_GATES, H2AGG_WC_PERMUTATION, H2AGG_WC_LOOKUPS");
    TRY(fr_check_k(c, vk->k));
    WcLayout& l = call->l;
    l = wc_layout(*vk, what, max_rows);
    call->gates = (what & H2AGG_WC_GATES) && l.G;
    call->permutation = (what & H2AGG_WC_PERMUTATION) && l.P;
    call->lookups = (what & H2AGG_WC_LOOKUPS) && l.L;
    if ((vk->num_advice && !advice) || (qe_nfixed(*vk) && !fixed) || (vk->num_instance && !instance) || !total ||
        (l.C && (!counts || !first_rows)) || (call->lookups && !theta) || (call->permutation && !mapping))
        return fail(c, H2AGG_ERR_INVALID, "null buffer");
    if (l.C > UINT32_MAX || l.C * l.max_rows > (SIZE_MAX >> 4)) return fail(c, H2AGG_ERR_NOMEM, "witness_check: the report does not fit the address space");
    std::vector<ph::HFr> chal;
    TRY(qe_challenges(c, *vk, challenges, &chal));
    if (call->lookups) TRY(fr_parse(c, theta, &call->theta));
    std::vector<const h2agg_vk::Expr*> list, part;
    if (call->gates) {
        TRY(qe_list(c, *vk, 0, 0, &list));
        for (size_t e0 = 0; e0 < list.size(); e0 += l.chunk) {
            part.assign(list.begin() + e0, list.begin() + std::min(list.size(), e0 + l.chunk));
            call->gate_progs.emplace_back();
            TRY(qe_compile(c, *vk, part, chal, &call->gate_progs.back()));
        }
    }
    if (call->lookups)
        for (size_t j = 0; j < l.L; ++j)
            for (int t = 0; t < 2; ++t) {
                list.clear();
                TRY(qe_list(c, *vk, 1 + t, j, &list));
                if (list.empty()) return fail(c, H2AGG_ERR_INVALID, "a lookup without expressions");
                call->lookup_progs.emplace_back();
                TRY(qe_compile(c, *vk, list, chal, &call->lookup_progs.back()));
            }
    return H2AGG_OK;
}

// counts, first rows and the lowest rows of the `lines` flag lines in the work memory: constraints c0 .. c0 + lines - 1
void wc_report_queue(h2agg_ctx* c, const WcLayout& l, uint8_t* w, uint32_t c0, uint32_t lines) {
    WcReportArgs a;
    a.zflags = (const uint32_t*)(w + l.zflags);
    a.sums = (uint32_t*)(w + l.sums);
    a.mins = (uint32_t*)(w + l.mins);
    a.counts = (uint32_t*)(w + l.counts);
    a.first_rows = (uint32_t*)(w + l.first_rows);
    a.rows = (uint32_t*)(w + l.rows);
    a.zwords = l.zwords;
    a.tiles = l.tiles;
    a.c0 = c0;
    a.lines = lines;
    a.max_rows = (uint32_t)l.max_rows;
    hipLaunchKernelGGL(k_wc_tile_count, dim3(l.tiles, lines), dim3(WC_WAVE), 0, c->stream, a);
    hipLaunchKernelGGL(k_wc_line, dim3(lines), dim3(WC_WAVE), 0, c->stream, a);
    if (l.max_rows) hipLaunchKernelGGL(k_wc_place, dim3(l.tiles, lines), dim3(WC_WAVE), 0, c->stream, a);
}

// Queues the whole check over device slabs: behind it the report (counts, first rows, total, rows — WcLayout) stands in
// wc_work.  Nothing synchronises unless a workspace has to grow (all of them grow before the first launch).
int wc_queue(h2agg_ctx* c, const h2agg_vk& vk, const WcCall& call, const uint8_t* d_advice, const uint8_t* d_fixed,
             const uint8_t* d_instance, const void* d_mapping) {
    const WcLayout& l = call.l;
    const unsigned k = vk.k;
    const uint32_t n = l.n;
    std::vector<size_t> gate_at, lookup_at;
    size_t prog_words = 0;
    for (const QeProgram& p : call.gate_progs) {
        gate_at.push_back(prog_words);
        prog_words += p.words();
    }
    for (const QeProgram& p : call.lookup_progs) {
        lookup_at.push_back(prog_words);
        prog_words += p.words();
    }
    const size_t cols_at = prog_words;
    if (call.permutation) prog_words += 2 * l.P;
    // ---- everything that may have to grow, before the first launch
    const LkGeom geom = lk_geom(c);
    const LkLayout sort = lk_layout(l.u, geom.t);
    TRY(ensure(c, c->wc_work, l.total));
    TRY(ensure(c, c->qt_prog, 4 * prog_words + 4));
    if (call.lookups) TRY(ensure(c, c->lk_work, sort.total));
    uint8_t* w = (uint8_t*)c->wc_work.p;
    uint32_t* d_prog = (uint32_t*)c->qt_prog.p;
    uint32_t* zflags = (uint32_t*)(w + l.zflags);
    enum { GATES, PERMUTATION, LOOKUPS, REPORT, PHASES };   // of h2agg_last_phases (debug key phases)
    PhaseClock phases(c);
    // ---- the report of a constraint nobody checks: 0 failing rows, no first row, no rows
    HIP_TRY(c, hipMemsetAsync(w + l.counts, 0, l.first_rows - l.counts, c->stream));
    HIP_TRY(c, hipMemsetAsync(w + l.first_rows, 0xFF, l.total_at - l.first_rows, c->stream));
    HIP_TRY(c, hipMemsetAsync(w + l.total_at, 0, l.rows - l.total_at, c->stream));
    if (l.total > l.rows) HIP_TRY(c, hipMemsetAsync(w + l.rows, 0xFF, l.total - l.rows, c->stream));
    // ---- the programs and the permutation columns' places
    for (size_t p = 0; p < call.gate_progs.size(); ++p) {
        qe_put_queue(c, call.gate_progs[p].code.data(), call.gate_progs[p].code.size(), d_prog + gate_at[p]);
        qe_put_queue(c, call.gate_progs[p].pool.data(), call.gate_progs[p].pool.size(), d_prog + gate_at[p] + call.gate_progs[p].code.size());
    }
    for (size_t p = 0; p < call.lookup_progs.size(); ++p) {
        qe_put_queue(c, call.lookup_progs[p].code.data(), call.lookup_progs[p].code.size(), d_prog + lookup_at[p]);
        qe_put_queue(c, call.lookup_progs[p].pool.data(), call.lookup_progs[p].pool.size(), d_prog + lookup_at[p] + call.lookup_progs[p].code.size());
    }
    if (call.permutation) {
        std::vector<uint32_t> cols(2 * l.P);
        for (size_t g = 0; g < l.P; ++g) {
            cols[2 * g] = vk.perm_cols[g].kind;
            cols[2 * g + 1] = vk.perm_cols[g].index;
        }
        qe_put_queue(c, cols.data(), cols.size(), d_prog + cols_at);
    }
    // ---- gates: the interpreter with the zero test as its ending, a chunk of polynomials per launch
    phases.mark(GATES);
    uint32_t c0 = 0;
    for (size_t p = 0; p < call.gate_progs.size(); ++p) {
        const QeProgram& prog = call.gate_progs[p];
        QeArgs a;
        memset(&a, 0, sizeof a);
        a.prog = d_prog + gate_at[p];
        a.consts = a.prog + prog.code.size();
        a.advice = d_advice;
        a.fixed = d_fixed;
        a.instance = d_instance;
        a.flags = c->d_flags;
        a.ninstr = (uint32_t)(prog.code.size() / 3);
        a.n = n;
        a.check = 1;
        a.zflags = zflags;
        a.zwords = l.zwords;
        a.u = l.u;
        hipLaunchKernelGGL(k_qe_eval<true>, dim3((n + QE_THREADS - 1) / QE_THREADS), dim3(QE_THREADS), 0, c->stream, a);
        phases.mark(REPORT);
        wc_report_queue(c, l, w, c0, prog.m);
        phases.mark(GATES);
        c0 += prog.m;
    }
    // ---- permutation: a chunk of columns per launch
    phases.mark(PERMUTATION);
    if (call.permutation)
        for (size_t g0 = 0; g0 < l.P; g0 += l.chunk) {
            const uint32_t lines = (uint32_t)std::min<size_t>(l.chunk, l.P - g0);
            WcPermArgs a;
            a.advice = d_advice;
            a.fixed = d_fixed;
            a.instance = d_instance;
            a.cols = d_prog + cols_at;
            a.mapping = (const uint2*)d_mapping;
            a.zflags = zflags;
            a.flags = c->d_flags;
            a.n = n;
            a.P = (uint32_t)l.P;
            a.g0 = (uint32_t)g0;
            a.zwords = l.zwords;
            hipLaunchKernelGGL(k_wc_permutation, dim3((n + BLOCK - 1) / BLOCK, lines), dim3(BLOCK), 0, c->stream, a);
            phases.mark(REPORT);
            wc_report_queue(c, l, w, (uint32_t)(l.G + g0), lines);
            phases.mark(PERMUTATION);
        }
    // ---- lookups: the two theta-folds, the sort of the table's usable rows, a search per input row
    phases.mark(LOOKUPS);
    if (call.lookups)
        for (size_t j = 0; j < l.L; ++j) {
            uint8_t* fold[2] = {w + l.fold_a, w + l.fold_s};
            for (int t = 0; t < 2; ++t)
                qe_eval_queue(c, call.lookup_progs[2 * j + t], d_prog + lookup_at[2 * j + t], false, k, d_advice, d_fixed, d_instance,
                              &call.theta, nullptr, true, fold[t]);
            TRY(lk_sort_queue(c, fold[1], sort, l.u, geom));
            const uint8_t* lw = (const uint8_t*)c->lk_work.p;
            WcLookupArgs a;
            a.a = fold[0];
            a.s_in = fold[1];
            a.s_w0 = lw + sort.w0;
            a.s_w1 = lw + sort.w1;
            a.s_plan = (const uint32_t*)(lw + sort.plan);
            a.zflags = zflags;
            a.n = n;
            a.u = l.u;
            hipLaunchKernelGGL(k_wc_lookup, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, a);
            phases.mark(REPORT);
            wc_report_queue(c, l, w, (uint32_t)(l.G + l.P + j), 1);
            phases.mark(LOOKUPS);
        }
    phases.mark(REPORT);
    hipLaunchKernelGGL(k_wc_total, dim3(1), dim3(WC_WAVE), 0, c->stream, (const uint32_t*)(w + l.counts), (uint32_t)l.C,
                       (uint32_t*)(w + l.total_at));
    phases.mark(PhaseClock::END);
    HIP_TRY(c, hipGetLastError());
    static const char* const names[PHASES] = {"gates", "permutation", "lookups", "report"};
    phases.report(names, PHASES);   // (waits for the last event)
    return H2AGG_OK;
}

// The report of the check wc_queue queued, from wc_work to the caller's host arrays; synchronises and reports the flags.
int wc_report_out(h2agg_ctx* c, const WcLayout& l, size_t max_rows, uint32_t* counts, uint32_t* first_rows, uint32_t* rows, uint64_t* total) {
    const uint8_t* w = (const uint8_t*)c->wc_work.p;
    HIP_TRY(c, hipMemcpyAsync(counts, w + l.counts, 4 * l.C, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(first_rows, w + l.first_rows, 4 * l.C, hipMemcpyDeviceToHost, c->stream));
    if (max_rows) {
        if (l.max_rows == max_rows) {
            HIP_TRY(c, hipMemcpyAsync(rows, w + l.rows, 4 * l.C * max_rows, hipMemcpyDeviceToHost, c->stream));
        } else {   // max_rows > n: the device lines are n wide, the tail of every line of the caller's is "no row"
            memset(rows, 0xFF, 4 * l.C * max_rows);
            HIP_TRY(c, hipMemcpy2DAsync(rows, 4 * max_rows, w + l.rows, 4 * l.max_rows, 4 * l.max_rows, l.C, hipMemcpyDeviceToHost, c->stream));
        }
    }
    return stage_out(c, (uint8_t*)total, w + l.total_at, 8);
}

}  // namespace

extern "C" {

int h2agg_witness_check_layout(const h2agg_vk* vk, size_t* n_gate_polys, size_t* n_perm_columns, size_t* n_lookups) try {
    if (!vk) return H2AGG_ERR_INVALID;
    size_t G = 0;
    for (const auto& g : vk->gates) G += g.size();
    if (n_gate_polys) *n_gate_polys = G;
    if (n_perm_columns) *n_perm_columns = vk->perm_cols.size();
    if (n_lookups) *n_lookups = vk->lookups.size();
    return H2AGG_OK;
} API_CATCH

int h2agg_witness_check(h2agg_ctx* c, const h2agg_vk* vk, unsigned what, const uint8_t* advice, const uint8_t* fixed,
                        const uint8_t* instance, const uint8_t* challenges, const uint8_t theta[32], const uint32_t* mapping,
                        size_t max_rows, uint32_t* counts, uint32_t* first_rows, uint32_t* rows, uint64_t* total) try {
    TRY(bind(c));
    if (c->dbg_phases) c->last_phases.clear();
    if (!rows) max_rows = 0;
    WcCall call;
    TRY(wc_check(c, vk, what, advice, fixed, instance, challenges, theta, mapping, max_rows, counts, first_rows, total, &call));
    const WcLayout& l = call.l;
    const size_t n = l.n, col = 32 * n;
    // the range of every entry of the mapping, on the host: one pass over memory the copy is about to read
    if (call.permutation)
        for (size_t x = 0; x < l.P * n; ++x)
            if (mapping[2 * x] >= l.P || mapping[2 * x + 1] >= n)
                return fail(c, H2AGG_ERR_INVALID, "witness_check: a mapping entry is outside the P x 2^k cells");
    if (l.C == 0) {
        *total = 0;
        return H2AGG_OK;
    }
    const size_t A = vk->num_advice, F = qe_nfixed(*vk), I = vk->num_instance;
    TRY(ensure(c, c->in_a, (A + F + I) * col));
    if (call.permutation) TRY(ensure(c, c->in_b, 8 * l.P * n));
    TRY(stage_in(c, c->in_a, advice, A * col));
    TRY(stage_in(c, c->in_a, fixed, F * col, A * col));
    TRY(stage_in(c, c->in_a, instance, I * col, (A + F) * col));
    if (call.permutation) TRY(stage_in(c, c->in_b, (const uint8_t*)mapping, 8 * l.P * n));
    TRY(clear_flags(c));
    const uint8_t* d = (const uint8_t*)c->in_a.p;
    TRY(wc_queue(c, *vk, call, d, d + A * col, d + (A + F) * col, c->in_b.p));
    return wc_report_out(c, l, max_rows, counts, first_rows, rows, total);
} API_CATCH

}  // extern "C"
