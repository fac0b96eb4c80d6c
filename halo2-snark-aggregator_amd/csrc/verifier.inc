// The verifier-params pipeline on the GPU backend (included into h2agg.hip): the verifying key, the recording helpers,
// build_queries and the plan types.  The aggregation call that drives them, stage by stage, is csrc/verify_run.inc.
// SURVEY.md 8(f) row 1 (+ the callers of the hot path): everything between the proof bytes and the final pair.
//
//   VerifierParamsBuilder::build_params       halo2-snark-aggregator-api/src/systems/halo2/verify.rs:342-571
//   VerifierParams::queries                   .../params.rs:74-224
//   get_lagrange_commits                      .../lagrange.rs:17-39
//   Evaluable::chip_evaluate                  .../expression.rs:19-113
//   permutation::Evaluated::{expressions, queries}, CommonEvaluated::queries   .../permutation.rs:34-201
//   lookup::Evaluated::{expressions, queries} .../lookup.rs:34-182
//   vanish::Evaluated::{new, queries}         .../vanish.rs:18-92
//   assign_instance_commitment                .../verify.rs:574-649
//   verify_aggregation_proofs_in_chip         .../verify.rs:835-942
//   calc_verify_circuit_final_pair            halo2-snark-aggregator-circuit/src/verify_circuit.rs:114-201
//
// Division of labour: the host (this file) does the reference's CONTROL FLOW — it knows from the verifying key how a proof
// is laid out, which expression uses which evaluation, which queries exist — and records every `schip` call as an
// operation on the schema's Fr tape (csrc/schema.hpp); the device does the arithmetic: instance-column MSMs, point
// decompression, one Poseidon sponge per proof, the whole Fr tape (gates, permutation / lookup / vanishing expressions,
// Lagrange terms, the scalars of eval_prepare) in one launch, the two multi_exps, +/- e*G and to_affine.  The host's only
// field arithmetic is the reference's own native constant folding (omega^rot, 1/n: `pow_vartime` / `invert` outside the
// chips, verify.rs:158-173, params.rs:57-72).
//
// What of `VerifyingKey` / `ConstraintSystem` the path reads is handed over as a serialized description (h2agg_vk_create;
// format in include/h2agg.h); halo2_proofs is not vendored in the reference.

struct h2agg_vk {
    h2agg_ctx* ctx = nullptr;
    uint64_t uid = 0;   // never reused (a recorded aggregation names the keys it was made for by uid, not by address)
    uint32_t k = 0, num_advice = 0, num_instance = 0, num_challenges = 0, degree = 0, blinding_factors = 0;
    std::vector<uint8_t> advice_phase, challenge_phase;
    struct Query {
        uint32_t column;
        int32_t rotation;
    };
    std::vector<Query> advice_q, instance_q, fixed_q;
    struct PermCol {
        uint32_t kind, index;   // 0 advice, 1 fixed, 2 instance
    };
    std::vector<PermCol> perm_cols;
    std::vector<uint8_t> fixed_commitments, perm_commitments;   // 64 B each
    uint8_t vk_scalar[32] = {0};
    int transcript_kind = H2AGG_TRANSCRIPT_KIND_POSEIDON;   // how the key's proofs are written (h2agg_vk_set_transcript)
    int multiopen_kind = H2AGG_MULTIOPEN_GWC;               // ... and opened (h2agg_vk_set_multiopen)
    typedef std::vector<uint8_t> Expr;   // postfix bytecode
    std::vector<std::vector<Expr>> gates;
    struct Lookup {
        std::vector<Expr> inputs, tables;
    };
    std::vector<Lookup> lookups;
    // derived
    uint32_t n_sets = 0, chunk_len = 0, quotient_deg = 0, max_phase = 0;
    poseidon_host::HFr omega, omega_inv;
};

namespace {

namespace ph = poseidon_host;

enum : uint8_t { EX_CONST = 0, EX_FIXED, EX_ADVICE, EX_INSTANCE, EX_CHALLENGE, EX_NEG, EX_SUM, EX_PRODUCT, EX_SCALED };

struct BlobReader {
    const uint8_t* p;
    size_t left;
    bool ok = true;
    bool take(void* out, size_t n) {
        if (!ok || n > left) {
            ok = false;
            return false;
        }
        memcpy(out, p, n);
        p += n;
        left -= n;
        return true;
    }
    uint32_t u32() {
        uint32_t v = 0;
        take(&v, 4);
        return v;
    }
    void skip_pad(size_t n) {   // items are padded to 4 bytes
        const size_t pad = (4 - (n & 3)) & 3;
        if (pad > left) ok = false;
        else p += pad, left -= pad;
    }
    bool bytes(std::vector<uint8_t>& v, size_t n) {
        if (!ok || n > left) {
            ok = false;
            return false;
        }
        v.assign(p, p + n);
        p += n;
        left -= n;
        skip_pad(n);
        return ok;
    }
};

// structural validation of an expression: operand counts, stack discipline, index ranges
bool expr_valid(const h2agg_vk::Expr& e, const h2agg_vk& vk) {
    int depth = 0;
    size_t i = 0;
    while (i < e.size()) {
        const uint8_t op = e[i++];
        uint32_t idx = 0;
        switch (op) {
        case EX_CONST:
            if (i + 32 > e.size()) return false;
            i += 32;
            ++depth;
            break;
        case EX_FIXED: case EX_ADVICE: case EX_INSTANCE: case EX_CHALLENGE:
            if (i + 4 > e.size()) return false;
            memcpy(&idx, e.data() + i, 4);
            i += 4;
            if (op == EX_FIXED && idx >= vk.fixed_q.size()) return false;
            if (op == EX_ADVICE && idx >= vk.advice_q.size()) return false;
            if (op == EX_INSTANCE && idx >= vk.instance_q.size()) return false;
            if (op == EX_CHALLENGE && idx >= vk.num_challenges) return false;
            ++depth;
            break;
        case EX_NEG:
            if (depth < 1) return false;
            break;
        case EX_SUM: case EX_PRODUCT:
            if (depth < 2) return false;
            --depth;
            break;
        case EX_SCALED:
            if (depth < 1 || i + 32 > e.size()) return false;
            i += 32;
            break;
        default:
            return false;
        }
    }
    return depth == 1;
}

ph::HFr hfr_pow(ph::HFr base, uint64_t e) {
    ph::HFr acc = ph::one();
    while (e) {
        if (e & 1) acc = ph::mul(acc, base);
        base = ph::mul(base, base);
        e >>= 1;
    }
    return acc;
}
void hfr_bytes(const ph::HFr& a, uint8_t out[32]) {
    uint64_t w[4];
    ph::to_canonical(a, w);
    memcpy(out, w, 32);
}
ph::HFr hfr_u64(uint64_t v) {
    const uint64_t w[4] = {v, 0, 0, 0};
    return ph::from_words(w);
}
// bn256::Fr constants of halo2curves (unvendored; tests/test_verifier_pipeline.py checks them against their definitions)
const uint64_t FR_ROOT_OF_UNITY[4] = {0xd34f1ed960c37c9cull, 0x3215cf6dd39329c8ull, 0x98865ea93dd31f74ull, 0x03ddb9f5166d18b7ull};   // 7^((r-1)/2^28)
const uint64_t FR_DELTA[4] = {0x870e56bbe533e9a2ull, 0x5b5f898e5e963f25ull, 0x64ec26aad4c86e71ull, 0x09226b6e22c6f0caull};          // 7^(2^28)
constexpr int FR_S = 28;

// ---- recording helpers on the schema's tape -----------------------------------------------------------------------
struct Rec {
    Schema& S;
    Tape& t;
    explicit Rec(Schema& s) : S(s), t(s.tape) {}
    uint32_t cbytes(const uint8_t v[32]) { return t.add_const(v); }
    uint32_t chfr(const ph::HFr& v) {
        uint8_t b[32];
        hfr_bytes(v, b);
        return t.add_const(b);
    }
    uint32_t cu64(uint64_t v) {
        uint8_t b[32] = {0};
        memcpy(b, &v, 8);
        return t.add_const(b);
    }
    uint32_t mul(uint32_t a, uint32_t b) { return t.record(TAPE_MUL, a, b); }
    uint32_t add(uint32_t a, uint32_t b) { return t.record(TAPE_ADD, a, b); }
    uint32_t sub(uint32_t a, uint32_t b) { return t.record(TAPE_SUB, a, b); }
    uint32_t inv(uint32_t a) { return t.record(TAPE_INV, a, a); }
    uint32_t div(uint32_t a, uint32_t b) { return mul(a, inv(b)); }
    // ArithFieldChip::mul_add_accumulate (arith/field.rs:68-81): acc = acc * b + v, acc_0 = 0.  Recorded in its expanded form
    // sum_i v_i b^(n-1-i) — the same field element (exact arithmetic), but n independent products against powers built by
    // halving and one balanced sum instead of a chain of 2n dependent operations: on the device a tape costs its DEPTH
    // (~3.5 us per dependency level: a round trip through the register file in memory), and the chain over a circuit's
    // ~40 expressions was the deepest thing on it.
    uint32_t horner(const std::vector<uint32_t>& vals, uint32_t b) {
        if (vals.empty()) return cu64(0);
        const size_t n = vals.size();
        uint32_t acc = vals[n - 1];
        for (size_t i = 0; i + 1 < n; ++i) acc = add(acc, mul(vals[i], t.pow(t.materialize(b), (uint32_t)(n - 1 - i))));
        return acc;
    }
    // product of the factors as a balanced tree (the reference multiplies them one after the other: permutation.rs:95-118)
    uint32_t product(std::vector<uint32_t> f) {
        while (f.size() > 1) {
            size_t o = 0;
            for (size_t i = 0; i + 1 < f.size(); i += 2) f[o++] = mul(f[i], f[i + 1]);
            if (f.size() & 1) f[o++] = f.back();
            f.resize(o);
        }
        return f[0];
    }
    uint32_t pow_small(uint32_t base, uint64_t e) {               // pow_constant (arith/field.rs:83-104), e >= 1
        uint32_t acc = 0;
        bool have = false;
        for (int bit = 63; bit >= 0; --bit) {
            if (have) acc = mul(acc, acc);
            if ((e >> bit) & 1) {
                acc = have ? mul(acc, base) : base;
                have = true;
            }
        }
        return acc;
    }
};

struct ProofRegs {
    std::vector<uint32_t> instance_evals, advice_evals, fixed_evals, permutation_evals, challenges;
    uint32_t random_eval = 0;
    struct Set {
        uint32_t eval, next, last;   // last == ~0u: None
    };
    std::vector<Set> sets;
    struct Lk {
        uint32_t product, product_next, input, input_inv, table;
    };
    std::vector<Lk> lookups;
    uint32_t theta = 0, beta = 0, gamma = 0, y = 0, x = 0, v = 0, u = 0;
    uint32_t y_open = 0;   // Shplonk: the challenge squeezed before v (the y of include/h2agg.h's Shplonk section)
};

// Evaluable::chip_evaluate (expression.rs:19-113) as a stack machine over tape registers
uint32_t eval_expr(Rec& R, const h2agg_vk::Expr& e, const ProofRegs& P, uint32_t zero) {
    std::vector<uint32_t> st;
    size_t i = 0;
    while (i < e.size()) {
        const uint8_t op = e[i++];
        uint32_t idx = 0;
        switch (op) {
        case EX_CONST:
            st.push_back(R.cbytes(e.data() + i));
            i += 32;
            break;
        case EX_FIXED: case EX_ADVICE: case EX_INSTANCE: case EX_CHALLENGE:
            memcpy(&idx, e.data() + i, 4);
            i += 4;
            st.push_back(op == EX_FIXED ? P.fixed_evals[idx] : op == EX_ADVICE ? P.advice_evals[idx]
                         : op == EX_INSTANCE ? P.instance_evals[idx] : P.challenges[idx]);
            break;
        case EX_NEG:
            st.back() = R.sub(zero, st.back());                               // arith_ast!(zero - a)
            break;
        case EX_SUM: {
            const uint32_t b = st.back();
            st.pop_back();
            st.back() = R.add(st.back(), b);
            break;
        }
        case EX_PRODUCT: {
            const uint32_t b = st.back();
            st.pop_back();
            st.back() = R.mul(st.back(), b);
            break;
        }
        case EX_SCALED:
            st.back() = R.mul(R.cbytes(e.data() + i), st.back());             // arith_ast!((f * a))
            i += 32;
            break;
        }
    }
    return st.back();
}

// the transcript script of one proof (build_params' reading order, verify.rs:342-571), n_w W points at the end; a Shplonk
// key's proofs end in y, v, H1, u, H2 instead (n_w is not read)
std::string proof_script(const h2agg_vk& vk, size_t n_w) {
    std::string s = "C";                                                       // init_transcript :57-75
    s.append(vk.num_instance, 'X');                                            // squeeze_instance_commitment :77-97
    for (uint32_t phase = 0; phase <= vk.max_phase; ++phase) {                 // :360-377
        for (uint8_t ph_ : vk.advice_phase)
            if (ph_ == phase) s += 'P';
        for (uint8_t ph_ : vk.challenge_phase)
            if (ph_ == phase) s += 'Q';
    }
    s += 'Q';                                                                  // theta
    s.append(2 * vk.lookups.size(), 'P');                                      // permuted input / table commitments
    s += "QQ";                                                                 // beta, gamma
    s.append(vk.n_sets, 'P');                                                  // permutation product commitments
    s.append(vk.lookups.size(), 'P');                                          // lookup product commitments
    s += 'P';                                                                  // random commitment
    s += 'Q';                                                                  // y
    s.append(vk.quotient_deg, 'P');                                            // h commitments
    s += 'Q';                                                                  // x
    const size_t n_evals = vk.instance_q.size() + vk.advice_q.size() + vk.fixed_q.size() + 1 + vk.perm_commitments.size() / 64 +
                           (vk.n_sets ? 3 * (size_t)vk.n_sets - 1 : 0) + 5 * vk.lookups.size();
    s.append(n_evals, 'S');
    if (vk.multiopen_kind == H2AGG_MULTIOPEN_SHPLONK) {
        s += "QQPQPQ";                                                         // y, v, H1, u, H2, the per-proof squeeze
        return s;
    }
    s += 'Q';                                                                  // v
    s.append(n_w, 'P');                                                        // `while let Ok(p) = self.load_point()`
    s += 'Q';                                                                  // u
    s += 'Q';                                                                  // the per-proof squeeze of verify.rs:910-913
    return s;
}
// bytes of a proof point on the wire: 32 compressed (transcript.rs:63-70), 64 as x | y under ShaRead (sha.rs:53-54)
size_t proof_point_bytes(const h2agg_vk& vk) { return vk.transcript_kind == H2AGG_TRANSCRIPT_KIND_POSEIDON ? 32 : 64; }
size_t script_fixed_bytes(const h2agg_vk& vk) {   // proof bytes other than the W points
    const std::string s = proof_script(vk, 0);
    size_t n = 0;
    for (char ch : s) n += ch == 'P' ? proof_point_bytes(vk) : ch == 'S' ? 32 : 0;
    return n;
}
// does a proof of `plen` bytes fit the key?  The W points are whatever is left (verify.rs:487-490); a Shplonk proof ends in
// exactly two points, H1 and H2, which its script holds already.
bool proof_len_fits(const h2agg_vk& vk, size_t plen, size_t* n_w) {
    const size_t fixed = script_fixed_bytes(vk), pt = proof_point_bytes(vk);
    if (vk.multiopen_kind == H2AGG_MULTIOPEN_SHPLONK) {
        if (n_w) *n_w = 0;
        return plen == fixed;
    }
    if (plen % 32 != 0 || plen < fixed || (plen - fixed) % pt != 0) return false;
    if (n_w) *n_w = (plen - fixed) / pt;
    return true;
}

}  // namespace

extern "C" {

int h2agg_vk_create(h2agg_ctx* c, const uint8_t* blob, size_t len, h2agg_vk** out) try {
    if (!c || !blob || !out) return H2AGG_ERR_INVALID;
    *out = nullptr;
    BlobReader r{blob, len};
    if (r.u32() != 0x4B563248u || r.u32() != 1u) return fail(c, H2AGG_ERR_INVALID, "vk blob: bad magic / version");
    std::unique_ptr<h2agg_vk> vk(new h2agg_vk());
    vk->ctx = c;
    vk->k = r.u32();
    vk->num_advice = r.u32();
    vk->num_instance = r.u32();
    vk->num_challenges = r.u32();
    vk->degree = r.u32();
    vk->blinding_factors = r.u32();
    if (!r.ok || vk->k < 1 || vk->k > (uint32_t)FR_S || vk->degree < 3 || vk->num_advice > 65536 || vk->num_instance > 65536 ||
        vk->num_challenges > 65536)
        return fail(c, H2AGG_ERR_INVALID, "vk blob: header out of range (k in [1, 28], degree >= 3)");
    // n - (blinding_factors + 1) usable rows (verify.rs:601-603) must stay positive: otherwise the bound below wraps to a
    // huge unsigned value and the assert it restates never fires (and -(l) in rotate_omega would overflow)
    if ((uint64_t)vk->blinding_factors + 1 >= ((uint64_t)1 << vk->k))
        return fail(c, H2AGG_ERR_INVALID, "vk blob: blinding_factors + 1 must be smaller than 2^k");
    r.bytes(vk->advice_phase, vk->num_advice);
    r.bytes(vk->challenge_phase, vk->num_challenges);
    auto read_queries = [&](std::vector<h2agg_vk::Query>& q) {
        const uint32_t n = r.u32();
        if (!r.ok || (size_t)n * 8 > r.left) return r.ok = false;
        q.resize(n);
        for (auto& e : q) {
            e.column = r.u32();
            e.rotation = (int32_t)r.u32();
        }
        return r.ok;
    };
    read_queries(vk->advice_q);
    read_queries(vk->instance_q);
    read_queries(vk->fixed_q);
    {
        const uint32_t n = r.u32();
        if (!r.ok || (size_t)n * 8 > r.left) return fail(c, H2AGG_ERR_INVALID, "vk blob: truncated");
        vk->perm_cols.resize(n);
        for (auto& e : vk->perm_cols) {
            e.kind = r.u32();
            e.index = r.u32();
        }
    }
    {
        const uint32_t nf = r.u32();
        if (!r.ok || (size_t)nf * 64 > r.left) return fail(c, H2AGG_ERR_INVALID, "vk blob: truncated");
        r.bytes(vk->fixed_commitments, (size_t)nf * 64);
        const uint32_t np = r.u32();
        if (!r.ok || (size_t)np * 64 > r.left) return fail(c, H2AGG_ERR_INVALID, "vk blob: truncated");
        r.bytes(vk->perm_commitments, (size_t)np * 64);
    }
    r.take(vk->vk_scalar, 32);
    auto read_exprs = [&](std::vector<h2agg_vk::Expr>& v) {
        const uint32_t n = r.u32();
        if (!r.ok || n > r.left) return r.ok = false;
        v.resize(n);
        for (auto& e : v) {
            const uint32_t nb = r.u32();
            if (!r.ok || nb > r.left) return r.ok = false;
            r.bytes(e, nb);
        }
        return r.ok;
    };
    {
        const uint32_t ng = r.u32();
        if (!r.ok || ng > r.left) return fail(c, H2AGG_ERR_INVALID, "vk blob: truncated");
        vk->gates.resize(ng);
        for (auto& g : vk->gates) read_exprs(g);
        const uint32_t nl = r.u32();
        if (!r.ok || nl > r.left) return fail(c, H2AGG_ERR_INVALID, "vk blob: truncated");
        vk->lookups.resize(nl);
        for (auto& l : vk->lookups) {
            read_exprs(l.inputs);
            read_exprs(l.tables);
        }
    }
    if (!r.ok || r.left != 0) return fail(c, H2AGG_ERR_INVALID, "vk blob: truncated or trailing bytes");
    // ---- consistency
    if (vk->perm_commitments.size() / 64 != vk->perm_cols.size())
        return fail(c, H2AGG_ERR_INVALID, "vk: one permutation commitment per permutation column");
    auto has_cur = [](const std::vector<h2agg_vk::Query>& q, uint32_t col) {
        for (const auto& e : q)
            if (e.column == col && e.rotation == 0) return true;
        return false;
    };
    for (const auto& pc : vk->perm_cols) {                                      // get_any_query_index(column, Rotation::cur())
        const bool ok = pc.kind == 0 ? has_cur(vk->advice_q, pc.index) : pc.kind == 1 ? has_cur(vk->fixed_q, pc.index)
                        : pc.kind == 2 ? has_cur(vk->instance_q, pc.index) : false;
        if (!ok) return fail(c, H2AGG_ERR_INVALID, "vk: a permutation column is not queried at the current rotation");
    }
    for (const auto& q : vk->advice_q)
        if (q.column >= vk->num_advice) return fail(c, H2AGG_ERR_INVALID, "vk: advice query of an unknown column");
    for (const auto& q : vk->instance_q)
        if (q.column >= vk->num_instance) return fail(c, H2AGG_ERR_INVALID, "vk: instance query of an unknown column");
    for (const auto& q : vk->fixed_q)
        if (q.column >= vk->fixed_commitments.size() / 64) return fail(c, H2AGG_ERR_INVALID, "vk: fixed query of an unknown column");
    for (const auto& g : vk->gates)
        for (const auto& e : g)
            if (!expr_valid(e, *vk)) return fail(c, H2AGG_ERR_INVALID, "vk: malformed gate expression");
    for (const auto& l : vk->lookups) {
        for (const auto& e : l.inputs)
            if (!expr_valid(e, *vk)) return fail(c, H2AGG_ERR_INVALID, "vk: malformed lookup expression");
        for (const auto& e : l.tables)
            if (!expr_valid(e, *vk)) return fail(c, H2AGG_ERR_INVALID, "vk: malformed lookup expression");
    }
    vk->chunk_len = vk->degree - 2;                                            // permutation.columns.chunks(degree - 2)
    vk->n_sets = (uint32_t)((vk->perm_cols.size() + vk->chunk_len - 1) / vk->chunk_len);
    vk->quotient_deg = vk->degree - 1;                                         // domain.get_quotient_poly_degree()
    vk->max_phase = 0;
    for (uint8_t p : vk->advice_phase) vk->max_phase = p > vk->max_phase ? p : vk->max_phase;
    for (uint8_t p : vk->challenge_phase) vk->max_phase = p > vk->max_phase ? p : vk->max_phase;
    ph::HFr w = ph::from_words(FR_ROOT_OF_UNITY);                              // get_omega(): ROOT_OF_UNITY^(2^(S - k))
    for (uint32_t i = vk->k; i < (uint32_t)FR_S; ++i) w = ph::mul(w, w);
    vk->omega = w;
    vk->omega_inv = ph::inv(w);
    static std::atomic<uint64_t> next_uid{1};
    vk->uid = next_uid.fetch_add(1);
    *out = vk.release();
    return H2AGG_OK;
} API_CATCH

void h2agg_vk_destroy(h2agg_vk* vk) { delete vk; }

int h2agg_vk_set_transcript(h2agg_vk* vk, int kind) {
    if (!vk) return H2AGG_ERR_INVALID;
    if (kind != H2AGG_TRANSCRIPT_KIND_POSEIDON && kind != H2AGG_TRANSCRIPT_KIND_SHA256 && kind != H2AGG_TRANSCRIPT_KIND_KECCAK256)
        return fail(vk->ctx, H2AGG_ERR_INVALID, "unknown transcript kind (H2AGG_TRANSCRIPT_KIND_*)");
    vk->transcript_kind = kind;
    return H2AGG_OK;
}

int h2agg_vk_set_multiopen(h2agg_vk* vk, int kind) {
    if (!vk) return H2AGG_ERR_INVALID;
    if (kind != H2AGG_MULTIOPEN_GWC && kind != H2AGG_MULTIOPEN_SHPLONK)
        return fail(vk->ctx, H2AGG_ERR_INVALID, "unknown multiopen kind (H2AGG_MULTIOPEN_*)");
    vk->multiopen_kind = kind;
    return H2AGG_OK;
}

}  // extern "C"

// ---- recorded aggregations ------------------------------------------------------------------------------------------
// What h2agg_verify_aggregation records on the host — the schema of every proof, the lambda fold, both eval_prepare walks, the
// tape's dependency levels — depends on the SHAPE of the call only (which verifying keys, how many proofs of each, the proofs'
// length), never on a value: proof scalars and challenges sit in registers of their own (Tape::add_const_placeholder, no
// interning by value), commitments are payloads of their nodes.  A caller that aggregates batch after batch of the same
// circuits therefore gets the recording of the first call back: the next call only refills those registers and payloads
// (this call's proof bytes, decompressed points, instance commitments, challenges) and runs the same tape and multi_exps on
// them.  Every field operation and every point of the result is still computed from this call's inputs; what is kept is the
// program, as a HIP graph keeps launches.  h2agg_debug_configure("plan_cache", 0) records every call afresh (tests compare the two).
struct AggPlan {
    std::string sig;
    h2agg_schema* sc = nullptr;
    struct ChalPatch {
        uint32_t reg, circuit;
        size_t off;            // the challenge's bytes: H[circuit].chal[off ..]
    };
    struct ScalarPatch {
        uint32_t reg, circuit, proof, off;   // transcripts[proof][off .. off + 32]
    };
    struct PointPatch {
        uint32_t slot, circuit;
        uint8_t kind;          // 0: H[circuit].points, 1: H[circuit].inst_aff
        size_t off;
    };
    std::vector<ChalPatch> chal;
    std::vector<ScalarPatch> scalars;
    std::vector<PointPatch> points;
    uint32_t lam_reg = 0, acc_x = 0, acc_g = 0;
    uint64_t stamp = 0;
    bool cacheable = true;   // false: a commitment came from a buffer that is neither this call's data nor the key's
};
struct AggPlanCache {
    static constexpr size_t MAX_PLANS = 8;   // least recently used goes first
    std::vector<AggPlan> plans;
    uint64_t clock = 0;
    uint64_t hits = 0, misses = 0;
};

namespace {
void agg_plans_release(h2agg_ctx* c) {
    if (!c->agg_plans) return;
    for (AggPlan& p : c->agg_plans->plans) h2agg_schema_destroy(p.sc);
    delete c->agg_plans;
    c->agg_plans = nullptr;
}
}   // namespace

namespace {

// params.rs:57-72 / verify.rs:158-173: x * omega^at as one chip multiplication by a natively computed constant
uint32_t rotate_omega(Rec& R, const h2agg_vk& vk, uint32_t x, int32_t at) {
    const ph::HFr c = at < 0 ? hfr_pow(vk.omega_inv, (uint64_t)(-(int64_t)at)) : hfr_pow(vk.omega, (uint64_t)at);
    return R.mul(x, R.chfr(c));
}

struct Query {
    int32_t rotation;
    uint32_t point_reg;
    uint32_t node;
    uint32_t poly;   // which polynomial is opened: the interned key of the query's commitment (Shplonk groups by it)
};
constexpr uint32_t POLY_VANISHING = 0xffffffffu;   // the vanishing query's polynomial

// where each advice column's commitment stands among a proof's points: the script reads them phase by phase (verify.rs:360-377)
std::vector<uint32_t> advice_point_order(const h2agg_vk& vk) {
    std::vector<uint32_t> advice_pt(vk.num_advice);
    uint32_t pi = 0;
    for (uint32_t phase = 0; phase <= vk.max_phase; ++phase)
        for (uint32_t col = 0; col < vk.num_advice; ++col)
            if (vk.advice_phase[col] == phase) advice_pt[col] = pi++;
    return advice_pt;
}

// VerifierParams::queries (params.rs:74-224) for ONE proof (one inner proof per transcript): records the expression
// arithmetic on the tape and returns the evaluation queries in the reference's order
int build_queries(h2agg_ctx* c, Schema& S, const h2agg_vk& vk, const std::string& key, const ProofRegs& P,
                  const uint8_t* inst_commitments /* num_instance x 64 */, const uint8_t* points /* decoded proof points */,
                  std::vector<Query>& out) {
    Rec R(S);
    const uint32_t zero = R.cu64(0), one = R.cu64(1);
    const uint32_t l = vk.blinding_factors + 1;
    const uint64_t n = (uint64_t)1 << vk.k;
    // ---- challenges' derived scalars (verify.rs:493-496)
    const uint32_t x = P.x;
    const uint32_t x_next = rotate_omega(R, vk, x, 1), x_last = rotate_omega(R, vk, x, -(int32_t)l),
                   x_inv = rotate_omega(R, vk, x, -1);
    const uint32_t xn = R.t.record(TAPE_SQRN, x, vk.k);                        // pow_constant(x, n), n = 2^k: k squarings, one operation
    // ---- lagrange.rs:17-39: l_i = (w_i / n) * (x^n - 1) / (x - w_i), w_i = omega^-i, i = 0 ..= l
    const ph::HFr n_inv = ph::inv(hfr_u64(n));
    const uint32_t xn_m1 = R.sub(xn, one);
    std::vector<uint32_t> ls(l + 1);
    ph::HFr wi = ph::one();
    for (uint32_t i = 0; i <= l; ++i) {
        ls[i] = R.div(R.mul(R.chfr(ph::mul(wi, n_inv)), xn_m1), R.sub(x, R.chfr(wi)));
        wi = ph::mul(wi, vk.omega_inv);
    }
    const uint32_t l_0 = ls[0], l_last = ls[l];
    uint32_t l_blind = zero;                                                   // sum_with_constant(ls[1..l], 0)
    for (uint32_t i = 1; i < l; ++i) l_blind = R.add(l_blind, ls[i]);
    // ---- the expressions: gates, permutation, lookups (params.rs:98-154)
    std::vector<uint32_t> expression;
    for (const auto& gate : vk.gates)
        for (const auto& poly : gate) expression.push_back(eval_expr(R, poly, P, zero));
    {   // permutation.rs:54-136
        const uint32_t delta = R.chfr(ph::from_words(FR_DELTA));
        if (!P.sets.empty()) {
            expression.push_back(R.mul(l_0, R.sub(one, P.sets.front().eval)));
            const uint32_t z = P.sets.back().eval;
            expression.push_back(R.mul(l_last, R.sub(R.mul(z, z), z)));
        }
        for (size_t i = 1; i < P.sets.size(); ++i)
            expression.push_back(R.mul(R.sub(P.sets[i].eval, P.sets[i - 1].last), l_0));
        const uint32_t t0 = R.mul(P.beta, x);
        const uint32_t t1 = R.sub(one, R.add(l_last, l_blind));
        std::vector<uint32_t> col_evals;                                       // verify.rs:240-268
        for (const auto& pc : vk.perm_cols) {
            const auto& qs = pc.kind == 0 ? vk.advice_q : pc.kind == 1 ? vk.fixed_q : vk.instance_q;
            size_t qi = 0;
            while (!(qs[qi].column == pc.index && qs[qi].rotation == 0)) ++qi;
            col_evals.push_back(pc.kind == 0 ? P.advice_evals[qi] : pc.kind == 1 ? P.fixed_evals[qi] : P.instance_evals[qi]);
        }
        for (size_t ci = 0; ci < P.sets.size(); ++ci) {
            // left = next * prod_j (col_j + gamma + beta perm_j),  right = eval * prod_j (col_j + gamma + beta x delta^(ci L + j))
            // (permutation.rs:95-118 multiplies the factors one after the other and steps d = delta * d; the same products as
            // balanced trees, delta^k by halving)
            std::vector<uint32_t> lf{P.sets[ci].next}, rf{P.sets[ci].eval};
            const size_t lo = ci * vk.chunk_len, hi = std::min(col_evals.size(), lo + vk.chunk_len);
            for (size_t j = lo; j < hi; ++j) {
                const uint32_t t2 = R.add(col_evals[j], P.gamma);
                const uint32_t d = j == 0 ? t0 : R.mul(t0, R.t.pow(delta, (uint32_t)j));   // (cached powers of the constant)
                lf.push_back(R.add(t2, R.mul(P.beta, P.permutation_evals[j])));
                rf.push_back(R.add(t2, d));
            }
            expression.push_back(R.mul(R.sub(R.product(lf), R.product(rf)), t1));
        }
    }
    for (size_t j = 0; j < vk.lookups.size(); ++j) {                           // lookup.rs:34-119
        const auto& lk = P.lookups[j];
        const uint32_t left = R.mul(R.mul(lk.product_next, R.add(lk.input, P.beta)), R.add(lk.table, P.gamma));
        std::vector<uint32_t> iv, tv;
        for (const auto& e : vk.lookups[j].inputs) iv.push_back(eval_expr(R, e, P, zero));
        for (const auto& e : vk.lookups[j].tables) tv.push_back(eval_expr(R, e, P, zero));
        const uint32_t input_eval = R.horner(iv, P.theta), table_eval = R.horner(tv, P.theta);
        const uint32_t t0 = R.sub(one, R.add(l_last, l_blind));
        const uint32_t t1 = R.sub(lk.input, lk.table);
        expression.push_back(R.mul(l_0, R.sub(one, lk.product)));
        expression.push_back(R.mul(l_last, R.sub(R.mul(lk.product, lk.product), lk.product)));
        expression.push_back(R.mul(R.sub(left, R.mul(R.mul(lk.product, R.add(input_eval, P.beta)), R.add(table_eval, P.gamma))), t0));
        expression.push_back(R.mul(l_0, t1));
        expression.push_back(R.mul(R.mul(t1, R.sub(lk.input, lk.input_inv)), t0));
    }
    // ---- the queries (params.rs:156-223)
    auto evq = [&](int32_t rot, const std::string& name, uint32_t point, const uint8_t* commitment, uint32_t eval_reg) {
        const uint32_t cn = S.add_commitment(name.c_str(), commitment);
        const uint32_t en = S.add_leaf_reg(SchemaNode::EVAL, eval_reg);
        out.push_back(Query{rot, point, S.add_binary(SchemaNode::ADD, cn, en), S.nodes[cn].key});
    };
    S.grow_nodes(8 * (vk.instance_q.size() + vk.advice_q.size() + vk.fixed_q.size() + 16 + 5 * vk.lookups.size() + 3 * vk.n_sets));
    // proof point order (script): advice (by phase) | lookups permuted (2 each) | permutation products | lookup products |
    // random | h pieces | W
    const std::vector<uint32_t> advice_pt = advice_point_order(vk);
    size_t pi = vk.num_advice;
    const size_t pt_lookup_permuted = pi;
    pi += 2 * vk.lookups.size();
    const size_t pt_perm_product = pi;
    pi += vk.n_sets;
    const size_t pt_lookup_product = pi;
    pi += vk.lookups.size();
    const size_t pt_random = pi++;
    const size_t pt_h = pi;
    auto PT = [&](size_t i) { return points + 64 * i; };
    for (size_t qi = 0; qi < vk.instance_q.size(); ++qi)
        evq(vk.instance_q[qi].rotation, key + "_instance_commitments" + std::to_string(vk.instance_q[qi].column),
            rotate_omega(R, vk, x, vk.instance_q[qi].rotation), inst_commitments + 64 * vk.instance_q[qi].column, P.instance_evals[qi]);
    for (size_t qi = 0; qi < vk.advice_q.size(); ++qi)
        evq(vk.advice_q[qi].rotation, key + "_advice_commitments" + std::to_string(vk.advice_q[qi].column),
            rotate_omega(R, vk, x, vk.advice_q[qi].rotation), PT(advice_pt[vk.advice_q[qi].column]), P.advice_evals[qi]);
    const std::string pkey = key + "_0";                                       // verify.rs:286 ("{key}_{i}", i = inner proof)
    for (size_t si = 0; si < P.sets.size(); ++si) {                            // permutation.rs:138-201
        const std::string name = pkey + "_permutation_product_commitment_" + std::to_string(si);
        evq(0, name, x, PT(pt_perm_product + si), P.sets[si].eval);
        evq(1, name, x_next, PT(pt_perm_product + si), P.sets[si].next);
    }
    for (size_t si = P.sets.size() >= 2 ? P.sets.size() - 1 : 0; si-- > 0;)    // .rev().skip(1)
        evq(-(int32_t)(vk.blinding_factors + 1), pkey + "_permutation_product_commitment_" + std::to_string(si), x_last,
            PT(pt_perm_product + si), P.sets[si].last);
    for (size_t j = 0; j < vk.lookups.size(); ++j) {                           // lookup.rs:121-181
        const std::string kk = key + "_0_" + std::to_string(j);                // verify.rs:329
        const auto& lk = P.lookups[j];
        evq(0, kk + "_product_commitment", x, PT(pt_lookup_product + j), lk.product);
        evq(0, kk + "_permuted_input_commitment", x, PT(pt_lookup_permuted + 2 * j), lk.input);
        evq(0, kk + "_permuted_table_commitment", x, PT(pt_lookup_permuted + 2 * j + 1), lk.table);
        evq(-1, kk + "_permuted_input_commitment", x_inv, PT(pt_lookup_permuted + 2 * j), lk.input_inv);
        evq(1, kk + "_product_commitment", x_next, PT(pt_lookup_product + j), lk.product_next);
    }
    for (size_t qi = 0; qi < vk.fixed_q.size(); ++qi)
        evq(vk.fixed_q[qi].rotation, key + "_fixed_commitments" + std::to_string(vk.fixed_q[qi].column),
            rotate_omega(R, vk, x, vk.fixed_q[qi].rotation), vk.fixed_commitments.data() + 64 * vk.fixed_q[qi].column, P.fixed_evals[qi]);
    for (size_t i = 0; i < P.permutation_evals.size(); ++i)                    // permutation.rs:34-52
        evq(0, key + "_permutation_commitments" + std::to_string(i), x, vk.perm_commitments.data() + 64 * i, P.permutation_evals[i]);
    {   // vanish.rs:18-72
        const uint32_t expected_h_eval = R.div(R.horner(expression, P.y), R.sub(xn, one));
        uint32_t h = 0;
        for (uint32_t i = 0; i < vk.quotient_deg; ++i) {                       // expect_commitments.iter().rev().enumerate()
            const uint32_t cq = S.add_commitment((key + "_h_commitment" + std::to_string(i)).c_str(), PT(pt_h + (vk.quotient_deg - 1 - i)));
            h = i == 0 ? cq : S.add_binary(SchemaNode::ADD, S.add_binary(SchemaNode::MUL, S.add_leaf_reg(SchemaNode::SCALAR, xn), h), cq);
        }
        // (the vanishing query opens the h pieces folded with x^n: a polynomial of its own, under an id no interned key has)
        out.push_back(Query{0, x, S.add_binary(SchemaNode::ADD, h, S.add_leaf_reg(SchemaNode::SCALAR, expected_h_eval)), POLY_VANISHING});
        evq(0, key + "_random_commitment", x, PT(pt_random), P.random_eval);
    }
    (void)c;
    return H2AGG_OK;
}

}  // namespace

