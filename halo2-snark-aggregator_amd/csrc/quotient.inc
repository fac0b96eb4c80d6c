// The quotient polynomial h(X), host side (included into h2agg.hip behind lookup.inc: shares the context internals and reads
// h2agg_vk, which is verifier.inc's; kernels, number forms and bounds in quotient_kernels.hpp, checks in
// fr_host.inc, staging in host.inc, transforms and power tables in fr_fft.inc): h2agg_vk_expressions_eval[_device],
// h2agg_quotient[_device], h2agg_quotient_configure, h2agg_quotient_work_bytes.
// They stand for the evaluation of h(X) in halo2_proofs' create_proof — an unvendored git dependency of the reference, recalled
// from upstream (DESIGN.md section 2); the yardstick is the definition in include/h2agg.h.  Which expressions h has to satisfy,
// and in which order, is pinned by halo2-snark-aggregator-api/src/systems/halo2/params.rs:74-224 and vanish.rs:18-72.

namespace {

static_assert(QE_DEPTH == H2AGG_EXPR_MAX_DEPTH, "the header states the depth the kernel supports");

// A list of expressions compiled for k_qe_eval: `code` (three words per instruction), then the constant pool.
struct QeProgram {
    std::vector<uint32_t> code, pool;
    uint32_t m = 0;   // expressions
    size_t words() const { return code.size() + pool.size(); }
};

// Postfix bytecode of the key -> instructions.  Leaves become (slab, column, rotation mod n); constants, scale factors and
// challenges go to the pool in Montgomery form.  The key's own checks (expr_valid) hold; what is new here is the depth.
int qe_compile(h2agg_ctx* c, const h2agg_vk& vk, const std::vector<const h2agg_vk::Expr*>& list, const std::vector<ph::HFr>& chal,
               QeProgram* p) {
    const int64_t n = (int64_t)1 << vk.k;
    auto constant = [&](const ph::HFr& v) {
        uint32_t w[8];
        hfr_words(ph::mul(v, fr_radix()), w);
        p->pool.insert(p->pool.end(), w, w + 8);
        return (uint32_t)(p->pool.size() / 8 - 1);
    };
    auto emit = [&](uint32_t op, uint32_t a, uint32_t b) {
        p->code.push_back(op);
        p->code.push_back(a);
        p->code.push_back(b);
    };
    for (const h2agg_vk::Expr* ep : list) {
        const h2agg_vk::Expr& e = *ep;
        unsigned depth = 0;
        size_t i = 0;
        while (i < e.size()) {
            const uint8_t op = e[i++];
            uint32_t idx = 0;
            ph::HFr v;
            switch (op) {
            case EX_CONST:
                TRY(fr_parse(c, e.data() + i, &v));
                i += 32;
                emit(QE_CONST, constant(v), 0);
                ++depth;
                break;
            case EX_FIXED: case EX_ADVICE: case EX_INSTANCE: {
                memcpy(&idx, e.data() + i, 4);
                i += 4;
                const h2agg_vk::Query& q = op == EX_FIXED ? vk.fixed_q[idx] : op == EX_ADVICE ? vk.advice_q[idx] : vk.instance_q[idx];
                const uint32_t slab = op == EX_ADVICE ? 0u : op == EX_FIXED ? 1u : 2u;
                emit(QE_COLUMN | slab << 8, q.column, (uint32_t)((((int64_t)q.rotation % n) + n) % n));
                ++depth;
                break;
            }
            case EX_CHALLENGE:
                memcpy(&idx, e.data() + i, 4);
                i += 4;
                emit(QE_CONST, constant(chal[idx]), 0);
                ++depth;
                break;
            case EX_NEG:
                emit(QE_NEG, 0, 0);
                break;
            case EX_SUM: case EX_PRODUCT:
                emit(op == EX_SUM ? QE_SUM : QE_PRODUCT, 0, 0);
                --depth;
                break;
            case EX_SCALED:
                TRY(fr_parse(c, e.data() + i, &v));
                i += 32;
                emit(QE_SCALED, constant(v), 0);
                break;
            default:
                return fail(c, H2AGG_ERR_INVALID, "malformed expression");
            }
            if (depth > QE_DEPTH)
                return fail(c, H2AGG_ERR_INVALID, "an expression needs an operand stack deeper than H2AGG_EXPR_MAX_DEPTH (16)");
        }
        if (depth != 1) return fail(c, H2AGG_ERR_INVALID, "malformed expression");
        emit(QE_END, 0, 0);
        ++p->m;
    }
    return H2AGG_OK;
}

// the list `which` / `j` of the key (include/h2agg.h)
int qe_list(h2agg_ctx* c, const h2agg_vk& vk, int which, size_t j, std::vector<const h2agg_vk::Expr*>* list) {
    if (which == 0) {
        for (const auto& g : vk.gates)
            for (const auto& e : g) list->push_back(&e);
        return H2AGG_OK;
    }
    if (which != 1 && which != 2) return fail(c, H2AGG_ERR_INVALID, "which must be 0 (gates), 1 (lookup inputs) or 2 (lookup tables)");
    if (j >= vk.lookups.size()) return fail(c, H2AGG_ERR_INVALID, "no such lookup");
    for (const auto& e : which == 1 ? vk.lookups[j].inputs : vk.lookups[j].tables) list->push_back(&e);
    return H2AGG_OK;
}

int qe_challenges(h2agg_ctx* c, const h2agg_vk& vk, const uint8_t* challenges, std::vector<ph::HFr>* chal) {
    if (vk.num_challenges && !challenges) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    chal->resize(vk.num_challenges);
    for (uint32_t i = 0; i < vk.num_challenges; ++i) TRY(fr_parse(c, challenges + 32 * (size_t)i, &(*chal)[i]));
    return H2AGG_OK;
}

size_t qe_nfixed(const h2agg_vk& vk) { return vk.fixed_commitments.size() / 64; }

// `words` to d_dst, by kernels that carry them in their arguments (quotient_kernels.hpp)
void qe_put_queue(h2agg_ctx* c, const uint32_t* words, size_t count, uint32_t* d_dst) {
    for (size_t at = 0; at < count; at += QE_PUT_WORDS) {
        const uint32_t now = (uint32_t)std::min<size_t>(QE_PUT_WORDS, count - at);
        QePutArgs a;
        memcpy(a.w, words + at, 4 * (size_t)now);
        hipLaunchKernelGGL(k_qe_put, dim3((now + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, a, d_dst + at, now);
    }
}

// The program to d_prog (code, then pool), then the evaluation.  fold null: out is [m][n].  d_prog holds p.words() words.
void qe_eval_queue(h2agg_ctx* c, const QeProgram& p, uint32_t* d_prog, bool upload, unsigned k, const uint8_t* d_advice,
                   const uint8_t* d_fixed, const uint8_t* d_instance, const ph::HFr* fold, const uint8_t* d_acc_in, bool check,
                   uint8_t* d_out) {
    if (upload) {
        qe_put_queue(c, p.code.data(), p.code.size(), d_prog);
        qe_put_queue(c, p.pool.data(), p.pool.size(), d_prog + p.code.size());
    }
    const uint32_t n = 1u << k;
    QeArgs a;
    memset(a.fold, 0, sizeof a.fold);
    if (fold) hfr_words(ph::mul(*fold, fr_radix()), a.fold);
    a.prog = d_prog;
    a.consts = d_prog + p.code.size();
    a.advice = d_advice;
    a.fixed = d_fixed;
    a.instance = d_instance;
    a.acc_in = d_acc_in;
    a.out = d_out;
    a.flags = c->d_flags;
    a.ninstr = (uint32_t)(p.code.size() / 3);
    a.n = n;
    a.folded = fold != nullptr;
    a.check = check;
    a.zflags = nullptr;
    a.zwords = a.u = 0;
    hipLaunchKernelGGL(k_qe_eval<false>, dim3((n + QE_THREADS - 1) / QE_THREADS), dim3(QE_THREADS), 0, c->stream, a);
}

struct QeEvalCall {
    QeProgram prog;
    ph::HFr fold;
    bool folded = false;
    size_t nfixed = 0;
};

// every refusal of h2agg_vk_expressions_eval that does not depend on where the buffers live
int qe_eval_check(h2agg_ctx* c, const h2agg_vk* vk, int which, size_t j, unsigned k, const void* advice, const void* fixed,
                  const void* instance, const uint8_t* challenges, const uint8_t* fold, const void* out, QeEvalCall* call) {
    if (!vk) return fail(c, H2AGG_ERR_INVALID, "null verifying key");
    TRY(fr_check_k(c, k));
    if (k != vk->k) return fail(c, H2AGG_ERR_INVALID, "k differs from the key's");
    std::vector<const h2agg_vk::Expr*> list;
    TRY(qe_list(c, *vk, which, j, &list));
    if (list.empty()) return fail(c, H2AGG_ERR_INVALID, "the list holds no expression");
    call->nfixed = qe_nfixed(*vk);
    if ((vk->num_advice && !advice) || (call->nfixed && !fixed) || (vk->num_instance && !instance) || !out)
        return fail(c, H2AGG_ERR_INVALID, "null buffer");
    std::vector<ph::HFr> chal;
    TRY(qe_challenges(c, *vk, challenges, &chal));
    call->folded = fold != nullptr;
    if (fold) TRY(fr_parse(c, fold, &call->fold));
    return qe_compile(c, *vk, list, chal, &call->prog);
}

// ---- the quotient ------------------------------------------------------------------------------------------------------

// bn256::Fr::ZETA from the GLV basis, as poly.py derives it: a1 + b1 zeta = 0 mod r, b1 = -B1N
const ph::HFr& qt_zeta() {
    static const ph::HFr z = [] {
        const uint64_t a1[4] = {(uint64_t)GlvConst::A1[0] | (uint64_t)GlvConst::A1[1] << 32,
                                (uint64_t)GlvConst::A1[2] | (uint64_t)GlvConst::A1[3] << 32, 0, 0};
        const uint64_t b1n[4] = {(uint64_t)GlvConst::B1N[0] | (uint64_t)GlvConst::B1N[1] << 32, 0, 0, 0};
        return ph::mul(ph::from_words(a1), ph::inv(ph::from_words(b1n)));
    }();
    return z;
}

// Where every polynomial sits in a coset's value slab [polys][n], and the work memory of a call in elements of 32 bytes:
// the slab, the coefficients of l_0 / l_last / l_blind, the fold column, a lookup's two theta-folds, and `ext`: the extended
// evaluations [n][2^e], or on the split route the per-coset inverse transforms u[2^e][n] (the same size).  fft_work: the bytes
// of the transforms' work array.  Only the existing route has a transform of size 2^(k + e), so only there the work array (and
// the twiddle and shift tables, qt_queue) go by k + e.
constexpr unsigned QT_MAX_K = FR_S;   // k + e: the two-adicity of Fr, 28 (w_ext = fft_omega(k + e) is a host scalar)
// Who holds the key's columns (fixed, sigma, l_0 / l_last / l_blind).  QT_CALLER: the call — it builds the three Lagrange
// columns and transforms all of them per coset into the one slab.  QT_PK: a proving key (pk.inc) holds the coefficients of the
// three columns; the slab is as before, `lcoef` is gone.  QT_PK_COSETS: the proving key holds every coset's values, the slab
// is the witness alone ([A + I + sets + 3 L][n]) and the fixed-form kernels read two bases (quotient_kernels.hpp).
enum QtKeyMode { QT_CALLER = 0, QT_PK = 1, QT_PK_COSETS = 2 };
struct QtLayout {
    uint32_t A, F, I, P, sets, L;
    // columns of the slab; with QT_PK_COSETS fixed0, sigma0 and l0 are columns of the key's coset slab [F + P + 3][n] instead
    uint32_t fixed0, instance0, sigma0, z0, lz0, lap0, lsp0, l0, polys;
    size_t lcoef, acc, lin, ltab, ext, total, fft_work;
    unsigned e;
    bool split;
    QtKeyMode mode;
};
// what a proving key lends to a call: the coefficients of l_0 / l_last / l_blind [3][n], and with QT_PK_COSETS the slabs
// [2^e][F + P + 3][n]
struct QtKey {
    const uint8_t* lcoef;
    const uint8_t* cosets;
};

// k + e <= 24: one inverse transform of size 2^(k + e) ends the call; above that, or after h2agg_quotient_configure(ctx, 1), the
// coset-split ending, which transforms nothing larger than 2^k
bool qt_split_route(unsigned k, unsigned e, int forced) { return forced != 0 || k + e > FFT_MAX_K; }

QtLayout qt_layout(const h2agg_vk& vk, int forced_split, QtKeyMode mode = QT_CALLER) {
    QtLayout l;
    l.mode = mode;
    l.A = vk.num_advice;
    l.F = (uint32_t)qe_nfixed(vk);
    l.I = vk.num_instance;
    l.P = (uint32_t)vk.perm_cols.size();
    l.sets = vk.n_sets;
    l.L = (uint32_t)vk.lookups.size();
    if (mode == QT_PK_COSETS) {   // the slab: advice, instance, the Z of the sets, every lookup's Z, a', s'
        l.instance0 = l.A;
        l.z0 = l.instance0 + l.I;
        l.lz0 = l.z0 + l.sets;
        l.lap0 = l.lz0 + l.L;
        l.lsp0 = l.lap0 + l.L;
        l.polys = l.lsp0 + l.L;
        l.fixed0 = 0;   // the key's coset slab: fixed, sigma, the three
        l.sigma0 = l.F;
        l.l0 = l.F + l.P;
    } else {
        l.fixed0 = l.A;
        l.instance0 = l.fixed0 + l.F;
        l.sigma0 = l.instance0 + l.I;
        l.z0 = l.sigma0 + l.P;
        l.lz0 = l.z0 + l.sets;
        l.lap0 = l.lz0 + l.L;
        l.lsp0 = l.lap0 + l.L;
        l.l0 = l.lsp0 + l.L;
        l.polys = l.l0 + 3;
    }
    l.e = 0;
    while (((uint64_t)1 << l.e) < (uint64_t)vk.degree - 1) ++l.e;
    const size_t n = (size_t)1 << vk.k;
    l.lcoef = (size_t)l.polys * n;
    l.acc = l.lcoef + (mode == QT_CALLER ? 3 * n : 0);
    l.lin = l.acc + n;
    l.ltab = l.lin + n;
    l.ext = l.ltab + n;
    l.total = l.ext + (n << l.e);
    l.split = qt_split_route(vk.k, l.e, forced_split);
    l.fft_work = fr_fft_batch_work_bytes(l.polys, vk.k);
    if (!l.split) l.fft_work = std::max(l.fft_work, (size_t)32 << (vk.k + l.e));
    return l;
}

// what both h2agg_quotient* and h2agg_quotient_work_bytes refuse by the key's shape alone; null: the key is taken
const char* qt_shape_refusal(const h2agg_vk& vk, const QtLayout& l) {
    if (vk.k > FFT_MAX_K || vk.k + l.e > QT_MAX_K) return "the extended domain 2^(k + e) must be <= 2^28, and k <= 24";
    if (l.P && vk.degree < 3) return "permutation columns need degree >= 3";
    return nullptr;
}

struct QtScalars {
    std::vector<ph::HFr> chal;
    ph::HFr theta, beta, gamma, y, delta;
};

struct QtSlabs {
    const uint8_t *advice, *fixed, *instance, *sigma, *perm_z, *lookup_z, *lookup_ap, *lookup_sp;
};

int qt_check(h2agg_ctx* c, const h2agg_vk* vk, const QtSlabs& s, const uint8_t* challenges, const uint8_t* theta, const uint8_t* beta,
             const uint8_t* gamma, const uint8_t* y, const uint8_t* delta, const void* h, QtLayout* l, QtScalars* sc,
             QtKeyMode mode = QT_CALLER) {
    if (!vk) return fail(c, H2AGG_ERR_INVALID, "null verifying key");
    *l = qt_layout(*vk, c->cfg_quotient_split, mode);
    if (const char* why = qt_shape_refusal(*vk, *l)) return fail(c, H2AGG_ERR_INVALID, why);
    if ((l->A && !s.advice) || (l->F && !s.fixed) || (l->I && !s.instance) || (l->P && (!s.sigma || !s.perm_z)) ||
        (l->L && (!s.lookup_z || !s.lookup_ap || !s.lookup_sp)) || !theta || !beta || !gamma || !y || !delta || !h)
        return fail(c, H2AGG_ERR_INVALID, "null buffer");
    TRY(qe_challenges(c, *vk, challenges, &sc->chal));
    TRY(fr_parse(c, theta, &sc->theta));
    TRY(fr_parse(c, beta, &sc->beta));
    TRY(fr_parse(c, gamma, &sc->gamma));
    TRY(fr_parse(c, y, &sc->y));
    return fr_parse(c, delta, &sc->delta);
}

// Queues the whole quotient: nothing synchronises unless a workspace has to grow (all of them grow before the first launch).
// key: null (l.mode QT_CALLER), or what the proving key of the call lends (in.fixed and in.sigma are then its coefficient
// forms; with QT_PK_COSETS nothing reads them).
int qt_queue(h2agg_ctx* c, const h2agg_vk& vk, const QtLayout& l, const QtScalars& sc, const QtSlabs& in, uint8_t* d_h,
             const QtKey* key = nullptr) {
    const bool two = l.mode == QT_PK_COSETS;
    const unsigned k = vk.k, K = k + l.e;
    const size_t n = (size_t)1 << k, col = 32 * n;
    const uint32_t cosets = 1u << l.e;
    // programs: the gates under y, every lookup's two lists under theta
    std::vector<QeProgram> progs(1 + 2 * (size_t)l.L);
    {
        std::vector<const h2agg_vk::Expr*> list;
        TRY(qe_list(c, vk, 0, 0, &list));
        TRY(qe_compile(c, vk, list, sc.chal, &progs[0]));
        for (uint32_t j = 0; j < l.L; ++j)
            for (int t = 0; t < 2; ++t) {
                list.clear();
                TRY(qe_list(c, vk, 1 + t, j, &list));
                if (list.empty()) return fail(c, H2AGG_ERR_INVALID, "a lookup without expressions");
                TRY(qe_compile(c, vk, list, sc.chal, &progs[1 + 2 * j + t]));
            }
    }
    std::vector<size_t> prog_at;
    size_t prog_words = 0;
    for (const QeProgram& p : progs) {
        prog_at.push_back(prog_words);
        prog_words += p.words();
    }
    const size_t cols_at = prog_words;
    prog_words += l.P;
    const uint32_t pieces = vk.degree - 1;
    const size_t cross_at = prog_words;   // the split ending's constants, behind the permutation columns' places
    if (l.split) prog_words += 8 * (size_t)pieces * cosets;
    const size_t m = progs[0].m + (l.sets ? 2 * (size_t)l.sets + 1 : 0) + 5 * (size_t)l.L;
    if (m == 0) {   // no expression at all: N = 0
        HIP_TRY(c, hipMemsetAsync(d_h, 0, col * (vk.degree - 1), c->stream));
        return H2AGG_OK;
    }
    // ---- everything that may have to grow, before the first launch
    TRY(ensure(c, c->qt_work, 32 * l.total));
    TRY(ensure(c, c->qt_prog, 4 * prog_words + 4));
    TRY(ensure(c, c->qt_tab, fr_table_bytes(k)));
    const unsigned Kt = l.split ? k : K;   // the largest transform of the call: its work array, shift table and twiddles
    TRY(ensure(c, c->frfft_work, l.fft_work));
    TRY(ensure(c, c->frfft_shift, fr_table_bytes(Kt)));
    if (Kt) {
        TRY(fr_fft_ensure_twiddles(c, Kt, 0));
        TRY(fr_fft_ensure_twiddles(c, Kt, 1));
    }
    uint8_t* w = (uint8_t*)c->qt_work.p;
    uint8_t* cos = w;
    const uint8_t* lcoef = key ? key->lcoef : w + 32 * l.lcoef;
    uint8_t* acc = w + 32 * l.acc;
    uint8_t* lin = w + 32 * l.lin;
    uint8_t* ltab = w + 32 * l.ltab;
    uint8_t* ext = w + 32 * l.ext;
    uint32_t* d_prog = (uint32_t*)c->qt_prog.p;
    enum { FORWARD, GATES, PERMUTATION, LOOKUPS, INVERSE, PHASES };   // of h2agg_last_phases (debug key phases)
    PhaseClock phases(c);
    // ---- once per call: the programs, the permutation columns' places, w^i, the coefficients of l_0 / l_last / l_blind
    for (size_t p = 0; p < progs.size(); ++p) {
        qe_put_queue(c, progs[p].code.data(), progs[p].code.size(), d_prog + prog_at[p]);
        qe_put_queue(c, progs[p].pool.data(), progs[p].pool.size(), d_prog + prog_at[p] + progs[p].code.size());
    }
    if (l.P) {
        std::vector<uint32_t> cols(l.P);
        for (uint32_t g = 0; g < l.P; ++g)
            cols[g] = (vk.perm_cols[g].kind == 0 ? 0u : vk.perm_cols[g].kind == 1 ? l.fixed0 | (two ? QE_IN_KEY : 0u) : l.instance0) +
                      vk.perm_cols[g].index;
        qe_put_queue(c, cols.data(), cols.size(), d_prog + cols_at);
        fr_table_launch(c, fft_omega(k), k, (uint8_t*)c->qt_tab.p);
    }
    const ph::HFr w_ext = fft_omega(K), zeta = qt_zeta();
    if (l.split) {
        // T[i][c'] R, T[i][c'] = zeta^(-n i) w_E^(-c' i) / (2^e (s_c'^n - 1)): s_c'^n = zeta^n w_E^c', w_E = w_ext^n a primitive
        // 2^e-th root of unity.  They depend on k, e and degree alone.
        const ph::HFr zn = hfr_pow(zeta, n), w_E = hfr_pow(w_ext, n), zn_inv = ph::inv(zn), scale = ph::inv(hfr_u64(cosets));
        std::vector<ph::HFr> w_pow(cosets), per_coset(cosets);   // w_E^-j; 1 / (2^e (s_c'^n - 1))
        ph::HFr wp = ph::one(), sn = zn;
        const ph::HFr w_E_inv = ph::inv(w_E);
        for (uint32_t cs = 0; cs < cosets; ++cs, wp = ph::mul(wp, w_E_inv), sn = ph::mul(sn, w_E)) {
            w_pow[cs] = wp;
            per_coset[cs] = ph::mul(scale, ph::inv(ph::sub(sn, ph::one())));   // s^n - 1 != 0: see below
        }
        std::vector<uint32_t> tab(8 * (size_t)pieces * cosets);
        ph::HFr zi = fr_radix();   // zeta^(-n i) R
        for (uint32_t i = 0; i < pieces; ++i, zi = ph::mul(zi, zn_inv))
            for (uint32_t cs = 0; cs < cosets; ++cs)
                hfr_words(ph::mul(ph::mul(zi, w_pow[(uint32_t)(((uint64_t)cs * i) & (cosets - 1u))]), per_coset[cs]),
                          tab.data() + 8 * ((size_t)i * cosets + cs));
        qe_put_queue(c, tab.data(), tab.size(), d_prog + cross_at);
    }
    phases.mark(FORWARD);
    const uint32_t u = (uint32_t)n - vk.blinding_factors - 1u;
    if (!key) {
        uint8_t* rows = w + 32 * l.lcoef;
        hipLaunchKernelGGL(k_qe_lagrange_rows, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream, rows, (uint32_t)n, u);
        const FrFftSeg rows3 = {rows, 3};
        TRY(fr_fft_queue_batch(c, &rows3, 1, 3, k, 1, nullptr, rows));
    }
    // ---- the sources of the slab's columns, in QtLayout's order: one transform launch per pass takes them all.  (A key with
    // cosets: the witness alone — its segments without columns take no part.)
    const FrFftSeg src[FR_FFT_SEGS] = {{in.advice, l.A},           {in.fixed, two ? 0 : l.F}, {in.instance, l.I},
                                       {in.sigma, two ? 0 : l.P},  {in.perm_z, l.sets},       {in.lookup_z, l.L},
                                       {in.lookup_ap, l.L},        {in.lookup_sp, l.L},       {lcoef, two ? 0u : 3u}};
    const size_t key_slab = two ? col * ((size_t)l.F + l.P + 3) : 0;
    const dim3 rows((unsigned)((n + BLOCK - 1) / BLOCK)), block(BLOCK);
    ph::HFr s = zeta;
    for (uint32_t cs = 0; cs < cosets; ++cs, s = ph::mul(s, w_ext)) {
        if (cs) phases.mark(FORWARD);
        if (l.polys) TRY(fr_fft_queue_batch(c, src, FR_FFT_SEGS, l.polys, k, 0, &s, cos));
        const uint8_t* kcos = two ? key->cosets + cs * key_slab : cos;   // the base of the key's columns on this coset
        QeCoset q;
        q.cos = cos;
        q.key = kcos;
        q.acc_out = acc;
        hfr_words(ph::mul(sc.y, fr_radix()), q.yM);
        q.n = (uint32_t)n;
        q.l0 = l.l0;
        const uint8_t* acc_in = nullptr;
        phases.mark(GATES);
        if (progs[0].m) {
            qe_eval_queue(c, progs[0], d_prog + prog_at[0], false, k, cos, kcos + l.fixed0 * col, cos + l.instance0 * col, &sc.y, nullptr,
                          false, acc);
            acc_in = acc;
        }
        phases.mark(PERMUTATION);
        if (l.sets) {
            QePermArgs a;
            a.q = q;
            a.q.acc_in = acc_in;
            hfr_words(ph::mul(sc.beta, ph::mul(fr_radix(), fr_radix())), a.betaR2);
            hfr_words(ph::mul(sc.gamma, fr_radix()), a.gammaM);
            hfr_words(ph::mul(sc.delta, fr_radix()), a.deltaM);
            hfr_words(ph::mul(ph::mul(sc.beta, s), fr_radix()), a.bsM);
            a.cols = d_prog + cols_at;
            a.wT = fr_table_split(k);
            a.w_lo = (const uint8_t*)c->qt_tab.p;
            a.w_hi = a.w_lo + ((size_t)32 << a.wT);
            a.P = l.P;
            a.chunk = vk.chunk_len;
            a.n_sets = l.sets;
            a.sigma0 = l.sigma0;
            a.z0 = l.z0;
            a.rot_last = u;   // n - (blinding_factors + 1)
            hipLaunchKernelGGL(k_qe_permutation, rows, block, 0, c->stream, a);
            acc_in = acc;
        }
        phases.mark(LOOKUPS);
        for (uint32_t j = 0; j < l.L; ++j) {
            for (int t = 0; t < 2; ++t)
                qe_eval_queue(c, progs[1 + 2 * j + t], d_prog + prog_at[1 + 2 * j + t], false, k, cos, kcos + l.fixed0 * col,
                              cos + l.instance0 * col, &sc.theta, nullptr, false, t ? ltab : lin);
            QeLookupArgs a;
            a.q = q;
            a.q.acc_in = acc_in;
            hfr_words(ph::mul(sc.beta, fr_radix()), a.betaM);
            hfr_words(ph::mul(sc.gamma, fr_radix()), a.gammaM);
            a.in = lin;
            a.table = ltab;
            a.z = l.lz0 + j;
            a.ap = l.lap0 + j;
            a.sp = l.lsp0 + j;
            hipLaunchKernelGGL(k_qe_lookup, rows, block, 0, c->stream, a);
            acc_in = acc;
        }
        // s^n - 1 != 0: s = zeta w_ext^c' is outside the domain of n-th roots (zeta^n is a primitive cube root of unity)
        if (l.split) {
            // row c' of u = the size-n inverse transform of the fold column at shift s; the division by s^n - 1 is a scalar
            // per coset and waits in the constants of k_qe_cross_cosets
            phases.mark(INVERSE);
            TRY(fr_fft_queue(c, acc, k, 1, &s, ext + cs * col));
            continue;
        }
        QeScalar inv;
        hfr_words(ph::mul(ph::inv(ph::sub(hfr_pow(s, n), ph::one())), fr_radix()), inv.w);
        hipLaunchKernelGGL(k_qe_store_extended, rows, block, 0, c->stream, (const uint8_t*)acc, inv, (uint32_t)n, (uint32_t)l.e, cs, ext);
    }
    phases.mark(INVERSE);
    if (l.split) {
        QeCrossArgs a;
        a.u = ext;
        a.tab = d_prog + cross_at;
        a.h = d_h;
        a.n = (uint32_t)n;
        a.cosets = cosets;
        a.pieces = pieces;
        a.first = 0;
        const uint32_t full = pieces / QX_PIECES, rest = pieces % QX_PIECES;   // groups of QX_PIECES, then one smaller group
        if (full) hipLaunchKernelGGL(k_qe_cross_cosets<QX_PIECES>, dim3(rows.x, full), block, 0, c->stream, a);
        a.first = full * QX_PIECES;
        static_assert(QX_PIECES == 4, "one case per smaller group");
        if (rest == 1) hipLaunchKernelGGL(k_qe_cross_cosets<1>, dim3(rows.x, 1), block, 0, c->stream, a);
        if (rest == 2) hipLaunchKernelGGL(k_qe_cross_cosets<2>, dim3(rows.x, 1), block, 0, c->stream, a);
        if (rest == 3) hipLaunchKernelGGL(k_qe_cross_cosets<3>, dim3(rows.x, 1), block, 0, c->stream, a);
    } else {
        TRY(fr_fft_queue(c, ext, K, 1, &zeta, ext));
        HIP_TRY(c, hipMemcpyAsync(d_h, ext, col * pieces, hipMemcpyDeviceToDevice, c->stream));
    }
    phases.mark(PhaseClock::END);
    HIP_TRY(c, hipGetLastError());
    static const char* const names[PHASES] = {"forward", "gates", "permutation", "lookups", "inverse"};
    phases.report(names, PHASES);   // (waits for the last event: with the key set the queued form is not asynchronous)
    return H2AGG_OK;
}

}  // namespace

extern "C" {

int h2agg_vk_expressions_eval_device(h2agg_ctx* c, const h2agg_vk* vk, int which, size_t j, unsigned k, const void* d_advice,
                                     const void* d_fixed, const void* d_instance, const uint8_t* challenges, const uint8_t fold[32],
                                     void* d_out) try {
    TRY(bind(c));
    QeEvalCall call;
    TRY(qe_eval_check(c, vk, which, j, k, d_advice, d_fixed, d_instance, challenges, fold, d_out, &call));
    TRY(ensure(c, c->qt_prog, 4 * call.prog.words()));
    qe_eval_queue(c, call.prog, (uint32_t*)c->qt_prog.p, true, k, (const uint8_t*)d_advice, (const uint8_t*)d_fixed,
                  (const uint8_t*)d_instance, call.folded ? &call.fold : nullptr, nullptr, true, (uint8_t*)d_out);
    HIP_TRY(c, hipGetLastError());
    return H2AGG_OK;
} API_CATCH

int h2agg_vk_expressions_eval(h2agg_ctx* c, const h2agg_vk* vk, int which, size_t j, unsigned k, const uint8_t* advice,
                              const uint8_t* fixed, const uint8_t* instance, const uint8_t* challenges, const uint8_t fold[32],
                              uint8_t* out) try {
    TRY(bind(c));
    QeEvalCall call;
    TRY(qe_eval_check(c, vk, which, j, k, advice, fixed, instance, challenges, fold, out, &call));
    const size_t col = (size_t)32 << k;
    const size_t A = vk->num_advice, F = call.nfixed, I = vk->num_instance, outs = call.folded ? 1 : call.prog.m;
    TRY(ensure(c, c->in_a, (A + F + I) * col));
    TRY(ensure(c, c->out, outs * col));
    TRY(ensure(c, c->qt_prog, 4 * call.prog.words()));
    TRY(stage_in(c, c->in_a, advice, A * col));
    TRY(stage_in(c, c->in_a, fixed, F * col, A * col));
    TRY(stage_in(c, c->in_a, instance, I * col, (A + F) * col));
    TRY(clear_flags(c));
    const uint8_t* d = (const uint8_t*)c->in_a.p;
    qe_eval_queue(c, call.prog, (uint32_t*)c->qt_prog.p, true, k, d, d + A * col, d + (A + F) * col, call.folded ? &call.fold : nullptr,
                  nullptr, true, (uint8_t*)c->out.p);
    HIP_TRY(c, hipGetLastError());
    return stage_out(c, out, c->out.p, outs * col);
} API_CATCH

int h2agg_quotient_device(h2agg_ctx* c, const h2agg_vk* vk, const void* d_advice, const void* d_fixed, const void* d_instance,
                          const void* d_sigma, const void* d_perm_z, const void* d_lookup_z, const void* d_lookup_ap,
                          const void* d_lookup_sp, const uint8_t* challenges, const uint8_t theta[32], const uint8_t beta[32],
                          const uint8_t gamma[32], const uint8_t y[32], const uint8_t delta[32], void* d_h) try {
    TRY(bind(c));
    const QtSlabs s = {(const uint8_t*)d_advice,   (const uint8_t*)d_fixed,    (const uint8_t*)d_instance,  (const uint8_t*)d_sigma,
                       (const uint8_t*)d_perm_z,   (const uint8_t*)d_lookup_z, (const uint8_t*)d_lookup_ap, (const uint8_t*)d_lookup_sp};
    QtLayout l;
    QtScalars sc;
    TRY(qt_check(c, vk, s, challenges, theta, beta, gamma, y, delta, d_h, &l, &sc));
    return qt_queue(c, *vk, l, sc, s, (uint8_t*)d_h);
} API_CATCH

int h2agg_quotient(h2agg_ctx* c, const h2agg_vk* vk, const uint8_t* advice, const uint8_t* fixed, const uint8_t* instance,
                   const uint8_t* sigma, const uint8_t* perm_z, const uint8_t* lookup_z, const uint8_t* lookup_ap,
                   const uint8_t* lookup_sp, const uint8_t* challenges, const uint8_t theta[32], const uint8_t beta[32],
                   const uint8_t gamma[32], const uint8_t y[32], const uint8_t delta[32], uint8_t* h) try {
    TRY(bind(c));
    const QtSlabs s = {advice, fixed, instance, sigma, perm_z, lookup_z, lookup_ap, lookup_sp};
    QtLayout l;
    QtScalars sc;
    TRY(qt_check(c, vk, s, challenges, theta, beta, gamma, y, delta, h, &l, &sc));
    // the host form stages every slab whole: it keeps the bound it had (the resident form takes the larger keys)
    if (vk->k + l.e > FFT_MAX_K)
        return fail(c, H2AGG_ERR_INVALID, "the host-buffer form takes extended domains 2^(k + e) <= 2^24 (h2agg_quotient_device: <= 2^28)");
    const size_t col = (size_t)32 << vk->k;
    const uint8_t* host[8] = {advice, fixed, instance, sigma, perm_z, lookup_z, lookup_ap, lookup_sp};
    const size_t count[8] = {l.A, l.F, l.I, l.P, l.sets, l.L, l.L, l.L};
    size_t at[9] = {0};
    for (int i = 0; i < 8; ++i) at[i + 1] = at[i] + count[i] * col;
    const size_t out_bytes = col * (vk->degree - 1);
    TRY(ensure(c, c->in_a, at[8]));
    TRY(ensure(c, c->out, out_bytes));
    for (int i = 0; i < 8; ++i) TRY(stage_in(c, c->in_a, host[i], count[i] * col, at[i]));
    TRY(clear_flags(c));
    const uint8_t* d = (const uint8_t*)c->in_a.p;
    const QtSlabs ds = {d + at[0], d + at[1], d + at[2], d + at[3], d + at[4], d + at[5], d + at[6], d + at[7]};
    TRY(qt_queue(c, *vk, l, sc, ds, (uint8_t*)c->out.p));
    return stage_out(c, h, c->out.p, out_bytes);
} API_CATCH

int h2agg_quotient_configure(h2agg_ctx* c, int split) try {
    if (!c) return H2AGG_ERR_INVALID;
    if (split != 0 && split != 1) return fail(c, H2AGG_ERR_INVALID, "h2agg_quotient_configure: split must be 0 (by size) or 1 (always)");
    c->cfg_quotient_split = split;
    return H2AGG_OK;
} API_CATCH

// no context: the route is the rule's (h2agg_quotient_configure belongs to a context)
int h2agg_quotient_work_bytes(const h2agg_vk* vk, size_t* bytes_out) try {
    if (!vk || !bytes_out) return H2AGG_ERR_INVALID;
    const QtLayout l = qt_layout(*vk, 0);
    if (qt_shape_refusal(*vk, l)) return H2AGG_ERR_INVALID;
    *bytes_out = 32 * l.total + l.fft_work;
    return H2AGG_OK;
} API_CATCH

}  // extern "C"
