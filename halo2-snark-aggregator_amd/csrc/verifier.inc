// The verifier-params pipeline and the aggregation driver on the GPU backend (included into h2agg.hip).
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

// the transcript script of one proof (build_params' reading order, verify.rs:342-571), n_w W points at the end
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
// does a proof of `plen` bytes fit the key?  The W points are whatever is left (verify.rs:487-490).
bool proof_len_fits(const h2agg_vk& vk, size_t plen, size_t* n_w) {
    const size_t fixed = script_fixed_bytes(vk), pt = proof_point_bytes(vk);
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
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

void h2agg_vk_destroy(h2agg_vk* vk) { delete vk; }

int h2agg_vk_set_transcript(h2agg_vk* vk, int kind) {
    if (!vk) return H2AGG_ERR_INVALID;
    if (kind != H2AGG_TRANSCRIPT_KIND_POSEIDON && kind != H2AGG_TRANSCRIPT_KIND_SHA256 && kind != H2AGG_TRANSCRIPT_KIND_KECCAK256)
        return fail(vk->ctx, H2AGG_ERR_INVALID, "unknown transcript kind (H2AGG_TRANSCRIPT_KIND_*)");
    vk->transcript_kind = kind;
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
};


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
        out.push_back(Query{rot, point, S.add_binary(SchemaNode::ADD, cn, en)});
    };
    S.grow_nodes(8 * (vk.instance_q.size() + vk.advice_q.size() + vk.fixed_q.size() + 16 + 5 * vk.lookups.size() + 3 * vk.n_sets));
    // proof point order (script): advice (by phase) | lookups permuted (2 each) | permutation products | lookup products |
    // random | h pieces | W
    std::vector<uint32_t> advice_pt(vk.num_advice);
    size_t pi = 0;
    for (uint32_t phase = 0; phase <= vk.max_phase; ++phase)
        for (uint32_t col = 0; col < vk.num_advice; ++col)
            if (vk.advice_phase[col] == phase) advice_pt[col] = (uint32_t)pi++;
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
        out.push_back(Query{0, x, S.add_binary(SchemaNode::ADD, h, S.add_leaf_reg(SchemaNode::SCALAR, expected_h_eval))});
        evq(0, key + "_random_commitment", x, PT(pt_random), P.random_eval);
    }
    (void)c;
    return H2AGG_OK;
}

// One all-gather of a sharded aggregation: every rank contributes `bytes`, every rank receives [world][bytes].  Through the
// caller's transport (shard->allgather: MPI, a torch.distributed store, sockets, ...) or, without one, through the context's
// RCCL communicator over xGMI.
int shard_allgather(h2agg_ctx* c, const h2agg_shard* sh, const uint8_t* send, size_t bytes, std::vector<uint8_t>& recv) {
    const int nth = ++c->dbg_shard_calls;   // (debug key shard_fail 3 / 4: a failure of THIS rank inside exchange 1 / 2, before the gather)
    if ((c->dbg_shard_fail == 3 && nth == 1) || (c->dbg_shard_fail == 4 && nth == 2))
        return fail(c, H2AGG_ERR_NOMEM, "injected failure inside an exchange before its all-gather (debug key shard_fail)");
    recv.assign(bytes * sh->world, 0);
    if (sh->allgather) {
        const int rc = sh->allgather(sh->user, send, bytes, recv.data());
        if (rc != 0) return fail(c, H2AGG_ERR_HIP, "the caller's all-gather reported error " + std::to_string(rc));
        return H2AGG_OK;
    }
    RcclApi* a = rccl();
    if (!a) return fail(c, H2AGG_ERR_HIP, rccl_why());
    TRY(ensure(c, c->in_a, bytes));
    TRY(ensure(c, c->in_b, bytes * sh->world));
    HIP_TRY(c, hipMemcpyAsync(c->in_a.p, send, bytes, hipMemcpyHostToDevice, c->stream));
    NCCL_TRY(c, a, a->AllGather(c->in_a.p, c->in_b.p, bytes, ncclUint8, (ncclComm_t)c->comm, c->stream));
    HIP_TRY(c, hipMemcpyAsync(recv.data(), c->in_b.p, bytes * sh->world, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return H2AGG_OK;
}

// Both exchanges carry a STATUS word per rank (0 = fine, else the H2AGG_ERR_* code of a failure local to that rank: a proof that
// does not decode, a non-canonical scalar, no memory ...).  A rank that fails between the validation of its shard description
// and an exchange still enters that exchange, with its code in the word; every rank then leaves the call at the same point —
// the failing one with its own error, the others with H2AGG_ERR_PEER — instead of waiting forever in an all-gather one rank
// never joins (ADVICE r4).  Returns 0 when every rank reported 0.
int shard_peer_status(h2agg_ctx* c, const h2agg_shard* sh, const uint8_t* recv, size_t stride, size_t off, uint32_t my_status,
                      const char* where) {
    for (size_t r = 0; r < sh->world; ++r) {
        uint32_t st;
        memcpy(&st, recv + r * stride + off, 4);
        if (st == 0) continue;
        if (my_status) return (int)my_status;   // (the caller keeps its own message)
        return fail(c, H2AGG_ERR_PEER, "sharded aggregation: rank " + std::to_string(r) + " failed with code " + std::to_string(st) + " " + where);
    }
    return H2AGG_OK;
}

// Exchange 1 (verify.rs:909-913, :924): the aggregation transcript absorbs EVERY proof's last squeeze, in aggregation order,
// before it yields lambda.  Each rank contributes its status word and {position, squeeze} records for its proofs (N_all slots
// per rank, unused ones marked), every rank assembles the same N_all x 32 bytes and runs the same sponge: the same lambda
// everywhere.
// *gathered (both exchanges): set once the all-gather has returned — from there on every rank has seen the same bytes, so a
// failure is one every rank has alike; before it, the failure is this rank's alone and the others still wait for it.
int shard_lambda(h2agg_ctx* c, const h2agg_shard* sh, size_t N_all, const uint8_t* local_sq, size_t nlocal, uint8_t lambda[32],
                 uint32_t& flags, uint32_t my_status = 0, bool* gathered = nullptr) {
    constexpr size_t REC = 36, HDR = 4;
    std::vector<uint8_t> send(HDR + N_all * REC, 0xff), recv;
    memcpy(send.data(), &my_status, 4);
    for (size_t i = 0; i < nlocal && !my_status; ++i) {
        const uint32_t g = sh->global_index[i];
        memcpy(send.data() + HDR + REC * i, &g, 4);
        memcpy(send.data() + HDR + REC * i + 4, local_sq + 32 * i, 32);
    }
    TRY(shard_allgather(c, sh, send.data(), send.size(), recv));
    if (gathered) *gathered = true;
    TRY(shard_peer_status(c, sh, recv.data(), send.size(), 0, my_status, "before the lambda exchange"));
    std::vector<uint8_t> all(N_all * 32);
    std::vector<uint8_t> seen(N_all, 0);
    for (size_t r = 0; r < sh->world; ++r)
        for (size_t i = 0; i < N_all; ++i) {
            const uint8_t* rec = recv.data() + r * send.size() + HDR + i * REC;
            uint32_t g;
            memcpy(&g, rec, 4);
            if (g == 0xffffffffu) continue;
            if (g >= N_all || seen[g]) return fail(c, H2AGG_ERR_INVALID, "sharded aggregation: two ranks claim one proof position (or a position is out of range)");
            seen[g] = 1;
            memcpy(all.data() + 32 * (size_t)g, rec + 4, 32);
        }
    for (size_t g = 0; g < N_all; ++g)
        if (!seen[g]) return fail(c, H2AGG_ERR_INVALID, "sharded aggregation: no rank holds proof " + std::to_string(g));
    const uint32_t upto = (uint32_t)N_all;
    flags |= poseidon_run_host(all.data(), 32 * N_all, &upto, 1, 1, lambda, 1);
    return H2AGG_OK;
}
// Exchange 2 (the fold of verify.rs:926-938 made distributive): all-gather of every rank's partial (W_x, W_g) and status word,
// summed with the group law on every rank.  The partials come from the transport: they are checked like any other input of
// the C ABI — canonical coordinates AND on the curve (k_g1_sum_strided_affine refuses either with FLAG_BAD_POINT /
// FLAG_NONCANONICAL) — before they enter the sum that goes to the pairing.
int shard_sum_pair(h2agg_ctx* c, const h2agg_shard* sh, uint8_t left_aff[64], uint8_t right_aff[64], uint32_t my_status = 0,
                   bool* gathered = nullptr) {
    constexpr size_t PAY = 132;
    uint8_t mine[PAY] = {};
    if (!my_status) {
        memcpy(mine, left_aff, 64);
        memcpy(mine + 64, right_aff, 64);
    }
    memcpy(mine + 128, &my_status, 4);
    std::vector<uint8_t> recv;
    TRY(shard_allgather(c, sh, mine, PAY, recv));
    if (gathered) *gathered = true;
    TRY(shard_peer_status(c, sh, recv.data(), PAY, 128, my_status, "between the two exchanges"));
    std::vector<uint8_t> jac(96 * 2 * (size_t)sh->world, 0);   // [rank][2] canonical Jacobian: (x, y, 1), identity (0, 1, 0)
    for (size_t k = 0; k < 2 * (size_t)sh->world; ++k) {
        const uint8_t* a = recv.data() + PAY * (k / 2) + 64 * (k & 1);
        bool zero = true;
        for (int b = 0; b < 64 && zero; ++b) zero = a[b] == 0;
        uint8_t* j = jac.data() + 96 * k;
        if (zero) j[32] = 1;
        else {
            memcpy(j, a, 64);
            j[64] = 1;
        }
    }
    TRY(ensure(c, c->in_b, jac.size()));
    TRY(ensure(c, c->out, 128));
    TRY(clear_flags(c));
    HIP_TRY(c, hipMemcpyAsync(c->in_b.p, jac.data(), jac.size(), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_g1_sum_strided_affine, dim3(2), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->in_b.p, (size_t)sh->world, (size_t)2,
                       (uint8_t*)c->out.p, c->d_flags);
    HIP_TRY(c, hipMemcpyAsync(c->h_pinned + 1024, c->out.p, 128, hipMemcpyDeviceToHost, c->stream));
    TRY(finish(c));   // (a partial that is not a canonical point of the curve surfaces here)
    memcpy(left_aff, c->h_pinned + 1024, 64);
    memcpy(right_aff, c->h_pinned + 1024 + 64, 64);
    return H2AGG_OK;
}

}  // namespace

extern "C" {

// advice_out (optional): the advice commitments of every proof, in aggregation order, num_advice_columns x 64 B each
// (canonical affine) — the fourth return value of verify_aggregation_proofs_in_chip (`commits`, verify.rs:852-856,927-939),
// which the production caller feeds to `coherent` (halo2-snark-aggregator-circuit/src/verify_circuit.rs:487-492).
// advice_cap: bytes available; too small -> H2AGG_ERR_INVALID before any work.
// each (h2agg_verify_proofs): no aggregation challenge and no fold — every proof's own (left, right) to each->pairs (128 B per
// proof of this call, in its order), a proof whose W count does not fit its rotation groups gets H2AGG_ERR_INVALID in
// each->status and is left out; left_aff / right_aff, lambda_out, s_g2 are not used.  The recording is never cached.
struct EachOut {
    uint8_t* pairs;
    int32_t* status;
};
static int verify_aggregation_impl(h2agg_ctx* c, const h2agg_circuit_proofs* circuits, size_t ncircuits, const h2agg_shard* shard,
                                   const uint8_t* s_g2, const uint8_t* g2, uint8_t left_aff[64], uint8_t right_aff[64],
                                   uint8_t lambda_out[32], int* pairing_ok, uint8_t* advice_out, size_t advice_cap,
                                   EachOut* each = nullptr) try {
    TRY(bind(c));
    if (!circuits || ncircuits == 0 || !left_aff || !right_aff) return fail(c, H2AGG_ERR_INVALID, "null argument");
    if ((s_g2 == nullptr) != (g2 == nullptr) || (s_g2 && !pairing_ok))
        return fail(c, H2AGG_ERR_INVALID, "pass s_g2, g2 and pairing_ok together (or none)");
    if (pairing_ok) *pairing_ok = 0;
    memset(left_aff, 0, 64);
    memset(right_aff, 0, 64);
    if (!each)   // the reference never folds ShaRead proofs under an aggregation transcript (include/h2agg.h)
        for (size_t ci = 0; ci < ncircuits; ++ci)
            if (circuits[ci].vk && circuits[ci].vk->transcript_kind != H2AGG_TRANSCRIPT_KIND_POSEIDON)
                return fail(c, H2AGG_ERR_INVALID, "aggregation of proofs written with the SHA-256 / Keccak-256 transcript is not supported: verify them with h2agg_verify_proofs");
    PhaseTrace trace(c->dbg_phases ? &c->last_phases : nullptr);
    struct TraceScope {
        explicit TraceScope(PhaseTrace* t) { g_trace = t; }
        ~TraceScope() { g_trace = nullptr; }
    } trace_scope(&trace);
    struct Guard {   // a schema recorded by this call and not (yet) handed to the context's plan cache
        h2agg_schema* s = nullptr;
        ~Guard() { if (s) h2agg_schema_destroy(s); }
    } guard;
    size_t total_proofs = 0;   // the proofs THIS call holds (a shard: this rank's)
    for (size_t ci = 0; ci < ncircuits; ++ci) total_proofs += circuits[ci].nproofs;
    // Sharded aggregation (SURVEY.md 8(e)): the proofs are spread over `world` ranks, this call holds those whose positions in
    // the aggregation order are shard->global_index[]; N_all = the length of the whole aggregation.
    const size_t N_all = shard ? shard->total_proofs : total_proofs;
    if (N_all == 0) return fail(c, H2AGG_ERR_INVALID, "no proofs (the reference unwraps an empty fold: verify.rs:940)");
    if (shard) {
        if (shard->world < 1 || shard->rank >= shard->world || total_proofs > N_all || (total_proofs && !shard->global_index))
            return fail(c, H2AGG_ERR_INVALID, "bad shard description");
        if (!shard->allgather && (!c->comm || c->comm_size != (int)shard->world || c->comm_rank != (int)shard->rank))
            return fail(c, H2AGG_ERR_INVALID, "sharded aggregation without an exchange: pass shard->allgather or give the context an RCCL communicator of that rank / world (h2agg_comm_init_rank)");
        for (size_t i = 0; i < total_proofs; ++i) {
            if (shard->global_index[i] >= N_all) return fail(c, H2AGG_ERR_INVALID, "global_index out of range");
            for (size_t j = 0; j < i; ++j)
                if (shard->global_index[j] == shard->global_index[i]) return fail(c, H2AGG_ERR_INVALID, "global_index repeats");
        }
    }
    // From here on a shard is committed to both exchanges (include/h2agg.h): the rest of the call runs as `body`; whatever makes
    // it return early — any TRY below, an exception — is followed by the exchange this rank has not been through yet, with its
    // error code in the status word, so that no other rank waits for it.  ex1 / ex2: that exchange's all-gather has RETURNED
    // on this rank (a failure before that — no memory for the buffers, a transport error — is local like any other: ADVICE
    // r5).  `global` marks failures raised inside an exchange AFTER its all-gather (a peer's status, positions claimed twice,
    // a non-canonical squeeze): every rank sees those alike and leaves at the same point.
    struct { bool ex1 = false, ex2 = false, global = false; } xs;
    c->dbg_shard_calls = 0;
    // both exchanges as the body takes them
    auto exchange1 = [&](const uint8_t* sq, size_t nsq_local, uint8_t lam[32]) -> int {
        uint32_t fl = 0;
        const int rc = shard_lambda(c, shard, N_all, sq, nsq_local, lam, fl, 0, &xs.ex1);
        xs.global = xs.ex1;   // (whatever follows the gather is the same on every rank)
        if (rc != H2AGG_OK) return rc;
        if (fl) return fail(c, H2AGG_ERR_NONCANONICAL, "a proof's squeeze is not a canonical scalar");
        xs.global = false;
        return H2AGG_OK;
    };
    auto exchange2 = [&]() -> int {
        const int rc = shard_sum_pair(c, shard, left_aff, right_aff, 0, &xs.ex2);
        xs.global = xs.ex2;
        if (rc != H2AGG_OK) return rc;
        xs.global = false;
        return H2AGG_OK;
    };
    auto body = [&]() -> int {
    if (c->dbg_shard_fail == 1 && shard) return fail(c, H2AGG_ERR_INVALID, "injected failure before the lambda exchange (debug key shard_fail)");
    if (shard && total_proofs == 0) {   // more ranks than proofs: this rank only takes part in the two exchanges (identity partials)
        uint8_t lam0[32];
        TRY(exchange1(nullptr, 0, lam0));
        if (lambda_out) memcpy(lambda_out, lam0, 32);
        if (c->dbg_shard_fail == 2) return fail(c, H2AGG_ERR_INVALID, "injected failure between the exchanges (debug key shard_fail)");
        TRY(exchange2());
        if (s_g2) TRY(h2agg_final_pair_check(c, left_aff, right_aff, s_g2, g2, pairing_ok));
        return H2AGG_OK;
    }
    if (advice_out) {
        size_t need = 0;
        for (size_t ci = 0; ci < ncircuits; ++ci)
            if (circuits[ci].vk) need += circuits[ci].nproofs * (size_t)circuits[ci].vk->num_advice * 64;
        if (need > advice_cap) return fail(c, H2AGG_ERR_INVALID, "advice_out is too small for the proofs' advice commitments");
    }
    // sponge backend for this call (csrc/transcript.inc): host threads for small batches, the device sponge for large ones
    const bool host_sponge = transcript_backend(c, total_proofs) == 2;
    if (host_sponge && c->dbg_prewake) HostPool::get().prewake(total_proofs);   // the chains are posted ~0.3 ms from here
    uint32_t host_flags = 0;
    std::vector<uint8_t> agg_host;   // host backend: every proof's last squeeze
    if (host_sponge) agg_host.resize(total_proofs * 32);
    size_t advice_off = 0;
    // per-proof squeezes of every circuit, absorbed by the aggregation transcript (verify.rs:909-913, :924)
    TRY(ensure(c, c->agg_elems, total_proofs * 32 + 64));
    struct CircuitHost {
        std::vector<uint8_t> points, chal, inst_aff;   // downloaded
        std::vector<uint8_t> elems;                    // host sponge: the proofs' element streams
        const uint8_t* elems_p = nullptr;              // ... where they are (the vector, or the context's page-locked block)
        std::vector<uint32_t> upto;                    // squeeze positions of the layout
        size_t npoints = 0, nsq = 0, n_w = 0, elem_stride = 0, first_proof = 0;
        bool hashed = false;                           // a ShaRead circuit: its challenges are in `chal` when its turn ends
        std::string script;
    };
    std::vector<CircuitHost> H(ncircuits);
    TRY(clear_flags(c));
    size_t proof_base = 0;
    // The LAST circuit's downloads are taken apart (host sponges, no advice_out): only the element streams stand between the
    // device and the sponges, so they come down first, into page-locked memory, and the chains are posted; the decompressed
    // points and the instance commitments — wanted by the recording, 0.3 ms later — follow without the host waiting for them.
    // (All three went to pageable vectors, which makes every hipMemcpyAsync a blocking round trip: 75 us in front of the sponges.)
    size_t last_ci = ncircuits;
    for (size_t ci = 0; ci < ncircuits; ++ci)
        if (circuits[ci].nproofs) last_ci = ci;
    struct { bool on = false; size_t ci = 0, off_points = 0, off_inst = 0; } late;
    auto ensure_down = [&](size_t bytes) -> int {
        if (bytes <= c->h_down_cap) return H2AGG_OK;
        if (c->h_down) HIP_TRY(c, hipHostFree(c->h_down));
        c->h_down = nullptr;
        c->h_down_cap = 0;
        const size_t want = bytes + bytes / 2 + 4096;
        if (hipHostMalloc((void**)&c->h_down, want, hipHostMallocDefault) != hipSuccess) return fail(c, H2AGG_ERR_NOMEM, "hipHostMalloc(download block)");
        c->h_down_cap = want;
        return H2AGG_OK;
    };
    for (size_t ci = 0; ci < ncircuits; ++ci) {
        const h2agg_circuit_proofs& cp = circuits[ci];
        if (!cp.vk || cp.vk->ctx != c || !cp.name) return fail(c, H2AGG_ERR_INVALID, "circuit without a verifying key / name");
        const h2agg_vk& vk = *cp.vk;
        if (cp.nproofs == 0) continue;
        if (!cp.transcripts || !cp.transcript_lens || (vk.num_instance && (!cp.instances || !cp.instance_lens)))
            return fail(c, H2AGG_ERR_INVALID, "null proof data");
        auto tit = c->tables.find(cp.g_lagrange);
        if (vk.num_instance && tit == c->tables.end()) return fail(c, H2AGG_ERR_INVALID, "unknown g_lagrange handle");
        // ---- proof layout: all proofs of a circuit have the same length; the W points are whatever is left (verify.rs:487-490)
        const size_t plen = cp.transcript_lens[0];
        for (size_t i = 0; i < cp.nproofs; ++i)
            if (cp.transcript_lens[i] != plen || !cp.transcripts[i])
                return fail(c, H2AGG_ERR_INVALID, "proofs of one circuit must have one length");
        CircuitHost& h = H[ci];
        if (!proof_len_fits(vk, plen, &h.n_w))
            return fail(c, H2AGG_ERR_INVALID, "proof too short for this verifying key (read_exact fails: transcript.rs:63,101; sha.rs:46,65)");
        h.hashed = vk.transcript_kind != H2AGG_TRANSCRIPT_KIND_POSEIDON;
        h.script = proof_script(vk, h.n_w);
        TrLayout L;
        if (h.hashed) parse_script_hash(h.script.data(), h.script.size(), L);
        else parse_script(h.script.data(), h.script.size(), L);
        h.npoints = L.npoints;
        h.nsq = L.upto.size();
        h.upto = L.upto;
        h.elem_stride = 32 * (size_t)(L.nelem ? L.nelem : 1);
        h.first_proof = proof_base;
        // ---- assign_instance_commitment (verify.rs:574-649): one MSM per (proof, instance column) against g_lagrange
        const size_t ncol = vk.num_instance;
        TRY(ensure(c, c->inst_jac, (cp.nproofs * ncol + 1) * 96));
        TRY(ensure(c, c->inst_aff, (cp.nproofs * ncol + 1) * 64));
        size_t total_vals = 0;
        if (ncol) {
            const uint64_t max_len = ((uint64_t)1 << vk.k) - (vk.blinding_factors + 1);
            for (size_t i = 0; i < cp.nproofs * ncol; ++i) {
                if (cp.instance_lens[i] > max_len)
                    return fail(c, H2AGG_ERR_INVALID, "assert!(instance.len() <= params.n() - (blinding_factors + 1)) failed (verify.rs:601-603)");
                if (cp.instance_lens[i] > tit->second.n) return fail(c, H2AGG_ERR_INVALID, "instance column longer than the g_lagrange table");
                total_vals += cp.instance_lens[i];
            }
            for (size_t i = 0; i < cp.nproofs; ++i) {
                size_t pl = 0;
                for (size_t col = 0; col < ncol; ++col) pl += cp.instance_lens[i * ncol + col];
                if (pl && !cp.instances[i]) return fail(c, H2AGG_ERR_INVALID, "null instance data");
            }
        }
        // ONE page-locked staging block for this circuit: [transcript layout + proof bytes | instance values].  The transcript
        // half goes up on the auxiliary stream, where point decompression (a 254-step square root per point, ~0.17 ms of pure
        // latency) and everything else that depends on the proof bytes only run BESIDE the instance-column MSMs; only the
        // instance commitments' own two elements per proof wait for those (k_transcript_elements `which` = 1 / 2).
        const TrBlock tb = transcript_block(L, cp.nproofs);
        const size_t inst_off = (tb.total + 255) & ~(size_t)255;
        TRY(ensure_stage(c, inst_off + total_vals * 32 + 32));
        trace.mark("entry");
        HIP_TRY(c, hipEventRecord(c->ev_aux_go, c->stream));                 // (the previous users of tr_* are behind us)
        HIP_TRY(c, hipStreamWaitEvent(c->aux_stream, c->ev_aux_go, 0));
        chaos_wait(8, c->aux_stream);
        if (h.hashed) TRY(hash_transcript_begin(c, L, tb, cp.transcripts, nullptr, cp.nproofs, vk.vk_scalar, c->aux_stream));
        else TRY(transcript_begin(c, L, tb, cp.transcripts, cp.nproofs, vk.vk_scalar, c->aux_stream, 0));
        HIP_TRY(c, hipEventRecord(c->ev_aux, c->aux_stream));
        trace.mark("tr_begin");
        if (ncol) {
            TRY(ensure(c, c->inst_vals, total_vals * 32 + 32));
            size_t off = 0;
            uint8_t* hs = c->h_stage + inst_off;
            for (size_t i = 0; i < cp.nproofs; ++i) {
                size_t pl = 0;
                for (size_t col = 0; col < ncol; ++col) pl += cp.instance_lens[i * ncol + col];
                if (pl) memcpy(hs + 32 * off, cp.instances[i], 32 * pl);
                off += pl;
            }
            HIP_TRY(c, hipMemcpyAsync(c->inst_vals.p, hs, 32 * total_vals, hipMemcpyHostToDevice, c->stream));   // one copy
            if (trace.on) {
                trace.mark("inst_h2d_call");
                HIP_TRY(c, hipStreamSynchronize(c->stream));
                trace.mark("inst_upload");
            }
            off = 0;
            bool uniform = cp.nproofs * ncol > 1 && cp.instance_lens[0] > 0;
            for (size_t i = 1; uniform && i < cp.nproofs * ncol; ++i) uniform = cp.instance_lens[i] == cp.instance_lens[0];
            if (uniform) {   // [batch][n] scalars over one table: ONE set of launches (h2agg_g1_msm_device_batch_async)
                TRY(h2agg_g1_msm_device_batch_async(c, cp.g_lagrange, c->inst_vals.p, cp.instance_lens[0], cp.nproofs * ncol,
                                                    c->inst_jac.p));
            } else
            for (size_t i = 0; i < cp.nproofs * ncol; ++i) {
                uint8_t* dst = (uint8_t*)c->inst_jac.p + 96 * i;
                const size_t len = cp.instance_lens[i];
                if (len == 0) {                                               // None => assign_const(identity)  (:638)
                    uint8_t idj[96];
                    set_identity_jac(idj);
                    HIP_TRY(c, hipMemcpyAsync(dst, idj, 96, hipMemcpyHostToDevice, c->stream));
                    HIP_TRY(c, hipStreamSynchronize(c->stream));
                } else {
                    TRY(h2agg_g1_msm_device_async(c, cp.g_lagrange, (const uint8_t*)c->inst_vals.p + 32 * off, len, dst));
                }
                off += len;
            }
            TRY(join_tails(c));
            if (trace.on) {
                HIP_TRY(c, hipStreamSynchronize(c->stream));
                trace.mark("inst_msm_join");
            }
            hipLaunchKernelGGL(k_g1_batch_to_affine, dim3(grid_for(c, cp.nproofs * ncol)), dim3(BLOCK), 0, c->stream,
                               (const uint8_t*)c->inst_jac.p, cp.nproofs * ncol, (uint8_t*)c->inst_aff.p, c->d_flags);
        }
        if (trace.on) {
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            trace.mark("instance_msm");
        }
        // ---- the transcripts of this circuit's proofs: the late half (the instance commitments' elements), then the sponges
        h.points.resize(cp.nproofs * h.npoints * 64);
        h.chal.resize(cp.nproofs * h.nsq * 32);
        h.inst_aff.resize(cp.nproofs * ncol * 64 + 1);
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_aux, 0));
        if (h.hashed) {
            // ShaRead: no square roots and no sponge — the on-curve checks and the message streams are done; the chains run now
            // (device or host threads, csrc/transcript.inc hash_backend) and this circuit's challenges are complete when its
            // turn ends
            if (L.next) hash_stream_launch(c, L, tb, cp.nproofs, (const uint8_t*)c->inst_aff.p, c->stream, 2);
            const bool chain_host = hash_backend(c, cp.nproofs) == 2;
            TRY(hash_chain_run(c, vk.transcript_kind, L, tb, cp.nproofs, chain_host ? h.chal.data() : nullptr));
            if (!chain_host && !h.chal.empty())
                HIP_TRY(c, hipMemcpyAsync(h.chal.data(), c->tr_chal.p, h.chal.size(), hipMemcpyDeviceToHost, c->stream));
            if (!h.points.empty()) HIP_TRY(c, hipMemcpyAsync(h.points.data(), c->tr_points.p, h.points.size(), hipMemcpyDeviceToHost, c->stream));
            if (ncol) HIP_TRY(c, hipMemcpyAsync(h.inst_aff.data(), c->inst_aff.p, cp.nproofs * ncol * 64, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));   // tr_* and the staging block are reused by the next circuit
            trace.mark("hash_transcripts");
        } else {
        if (L.next) transcript_elements_launch(c, L, tb, cp.nproofs, (const uint8_t*)c->inst_aff.p, c->stream, 2);
        // host backend: only the element streams are made on the device (point decompression + PoseidonEncode); the sponges run
        // on worker threads further down, UNDER the recording of the schema their challenges feed
        const bool split_down = host_sponge && !advice_out && ci == last_ci && c->dbg_prewake;
        if (split_down) {
            const size_t nb_el = cp.nproofs * tb.elem_stride, nb_pt = h.points.size(), nb_in = ncol ? cp.nproofs * ncol * 64 : 0;
            auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
            TRY(ensure_down(al(nb_el) + al(nb_pt) + al(nb_in) + 256));
            late.on = true;
            late.ci = ci;
            late.off_points = al(nb_el);
            late.off_inst = al(nb_el) + al(nb_pt);
            h.elems_p = c->h_down;
            HIP_TRY(c, hipMemcpyAsync(c->h_down, c->tr_elems.p, nb_el, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));   // the element streams are here: the sponges can go
            if (nb_pt) HIP_TRY(c, hipMemcpyAsync(c->h_down + late.off_points, c->tr_points.p, nb_pt, hipMemcpyDeviceToHost, c->stream));
            if (nb_in) HIP_TRY(c, hipMemcpyAsync(c->h_down + late.off_inst, c->inst_aff.p, nb_in, hipMemcpyDeviceToHost, c->stream));
            trace.mark("tr_elements");
            proof_base += cp.nproofs;
            continue;
        }
        if (host_sponge) {
            h.elems.resize(cp.nproofs * tb.elem_stride);
            h.elems_p = h.elems.data();
            HIP_TRY(c, hipMemcpyAsync(h.elems.data(), c->tr_elems.p, h.elems.size(), hipMemcpyDeviceToHost, c->stream));
        } else if (tb.nsq) {
            TRY(poseidon_run(c, (const uint8_t*)c->tr_elems.p, tb.elem_stride, (const uint32_t*)((const uint8_t*)c->tr_in.p + tb.hdr),
                             (uint32_t)tb.nsq, (uint32_t)cp.nproofs, (uint8_t*)c->tr_chal.p));
        }
        if (!h.points.empty()) HIP_TRY(c, hipMemcpyAsync(h.points.data(), c->tr_points.p, h.points.size(), hipMemcpyDeviceToHost, c->stream));
        if (ncol) HIP_TRY(c, hipMemcpyAsync(h.inst_aff.data(), c->inst_aff.p, cp.nproofs * ncol * 64, hipMemcpyDeviceToHost, c->stream));
        if (!host_sponge) {   // the last squeeze of every proof -> the aggregation transcript's elements (device)
            HIP_TRY(c, hipMemcpyAsync(h.chal.data(), c->tr_chal.p, h.chal.size(), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpy2DAsync((uint8_t*)c->agg_elems.p + 32 * proof_base, 32, (const uint8_t*)c->tr_chal.p + 32 * (h.nsq - 1),
                                        32 * h.nsq, 32, cp.nproofs, hipMemcpyDeviceToDevice, c->stream));
        }
        HIP_TRY(c, hipStreamSynchronize(c->stream));   // tr_* and the staging block are reused by the next circuit
        trace.mark(host_sponge ? "tr_elements" : "transcripts");
        }   // (Poseidon)
        if (advice_out) {   // the proof's advice commitments = its first num_advice 'P' items, column order restored
            size_t pi = 0;
            std::vector<uint32_t> advice_pt(vk.num_advice);
            for (uint32_t phase = 0; phase <= vk.max_phase; ++phase)
                for (uint32_t col = 0; col < vk.num_advice; ++col)
                    if (vk.advice_phase[col] == phase) advice_pt[col] = (uint32_t)pi++;
            for (size_t i = 0; i < cp.nproofs; ++i)
                for (uint32_t col = 0; col < vk.num_advice; ++col, advice_off += 64)
                    memcpy(advice_out + advice_off, h.points.data() + 64 * (h.npoints * i + advice_pt[col]), 64);
        }
        proof_base += cp.nproofs;
    }
    // ---- the sponges.  Device backend: they have run (above); the aggregation challenge follows on the device.  Host backend:
    // every proof's chain goes to a worker thread NOW and runs while this thread records the schema below with placeholder
    // registers for the challenges (Tape::add_const_placeholder) — the values are patched in before the tape runs.
    uint8_t lambda[32];
    HostPool& pool = HostPool::get();
    std::vector<std::pair<size_t, size_t>> job_of;   // host sponge job -> (circuit, proof)
    std::atomic<uint32_t> sponge_bad{0};
    struct PoolScope {   // an early return between begin() and end() must still end the run
        HostPool* p = nullptr;
        HostPool::Run* r = nullptr;
        ~PoolScope() { if (p && r) p->end(r); }
    } pool_scope;
    if (host_sponge) {
        for (size_t ci = 0; ci < ncircuits; ++ci)
            for (size_t i = 0; i < circuits[ci].nproofs && !H[ci].hashed; ++i) job_of.push_back({ci, i});
        const poseidon_host::FastSpec* fs = &poseidon_fast_spec();
        const void* ic_any = nullptr;   // (captured by VALUE: the workers run after this block is left)
#ifdef H2AGG_HAVE_IFMA_BUILD
        if (host_sponge_kind() == 1 && poseidon_host::ifma::cpu_has_ifma() && poseidon_ifma_consts().ok) ic_any = &poseidon_ifma_consts();
#endif
        CircuitHost* Hp = H.data();
        const std::pair<size_t, size_t>* jobs = job_of.data();
        std::atomic<uint32_t>* bad = &sponge_bad;
        if (trace.on) {
            trace.jobs.resize(job_of.size());
            trace.posted_us = trace.since_call_us();
        }
        PhaseTrace* tr = trace.on ? &trace : nullptr;   // (outlives the run: PoolScope ends it before `trace` goes)
        pool_scope.r = pool.begin(job_of.size(), pool.size(), [Hp, jobs, bad, fs, ic_any, tr](size_t j) {
            struct Stamp {
                PhaseTrace* t;
                size_t j;
                float t_in;
                Stamp(PhaseTrace* t_, size_t j_) : t(t_), j(j_), t_in(t_ ? t_->since_call_us() : 0) {}
                ~Stamp() {
                    if (t) t->jobs[j] = {t_in, t->since_call_us() - t_in, sched_getcpu()};
                }
            } stamp(tr, j);
            CircuitHost& h = Hp[jobs[j].first];
            const size_t i = jobs[j].second;
            const uint8_t* el = h.elems_p + i * h.elem_stride;
            uint8_t* out = h.chal.data() + 32 * h.nsq * i;
            bool ok;
#ifdef H2AGG_HAVE_IFMA_BUILD
            if (ic_any)
                ok = poseidon_host::ifma::sponge_run(*(const poseidon_host::ifma::Consts*)ic_any, el, h.upto.data(), (uint32_t)h.nsq, out);
            else
#endif
                ok = poseidon_host::sponge_run(*fs, el, h.upto.data(), (uint32_t)h.nsq, out);
            if (!ok) bad->fetch_or(FLAG_NONCANONICAL, std::memory_order_relaxed);
        });
        pool_scope.p = &pool;
        trace.mark("pool_begin");
        if (late.on) {   // the chains are running: now the points and instance commitments the recording reads
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            CircuitHost& h = H[late.ci];
            if (!h.points.empty()) memcpy(h.points.data(), c->h_down + late.off_points, h.points.size());
            if (h.inst_aff.size() > 1) memcpy(h.inst_aff.data(), c->h_down + late.off_inst, h.inst_aff.size() - 1);
            trace.mark("points_down");
        }
    } else if (each) {
        TRY(finish(c));   // every transcript has run: bad point encodings / non-canonical scalars surface here
    } else if (!shard) {
        uint32_t upto = (uint32_t)total_proofs;
        TRY(ensure(c, c->tr_in, 256));
        HIP_TRY(c, hipMemcpyAsync(c->tr_in.p, &upto, 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        TRY(poseidon_run(c, (const uint8_t*)c->agg_elems.p, 32 * total_proofs, (const uint32_t*)c->tr_in.p, 1, 1,
                         (uint8_t*)c->agg_elems.p + 32 * total_proofs));
        HIP_TRY(c, hipMemcpyAsync(c->h_pinned + 1024, (uint8_t*)c->agg_elems.p + 32 * total_proofs, 32, hipMemcpyDeviceToHost, c->stream));
        TRY(finish(c));   // every transcript has run: bad point encodings / non-canonical scalars surface here
        memcpy(lambda, c->h_pinned + 1024, 32);
        trace.mark("lambda");
    } else {
        TRY(finish(c));   // (sharded, device sponges: lambda follows the exchange further down)
    }
    // ---- a recording of this shape from an earlier call?
    const bool cache_on = c->dbg_plan_cache != 0 && !each;   // (h2agg_debug_configure "plan_cache" 0: record every call afresh)
    std::string sig;
    for (size_t ci = 0; ci < ncircuits; ++ci) {
        char buf[96];
        snprintf(buf, sizeof buf, "%llu:%zu:%zu:", (unsigned long long)circuits[ci].vk->uid, circuits[ci].nproofs,
                 circuits[ci].nproofs ? circuits[ci].transcript_lens[0] : (size_t)0);
        sig += buf;
        sig += circuits[ci].name;
        sig += ';';
    }
    if (shard) {   // a shard's recording carries ITS powers of lambda
        sig += "shard:" + std::to_string(N_all) + ":";
        for (size_t i = 0; i < total_proofs; ++i) sig += std::to_string(shard->global_index[i]) + ",";
    }
    AggPlan* plan = nullptr;
    if (cache_on && c->agg_plans)
        for (AggPlan& pl : c->agg_plans->plans)
            if (pl.sig == sig) plan = &pl;
    AggPlan fresh;
    h2agg_schema* sc = nullptr;
    std::vector<std::pair<uint32_t, uint32_t>> each_roots;   // each: (w_x, w_g) of every proof that has them ...
    std::vector<size_t> each_idx;                            // ... and its place in the call
    if (plan) {
        sc = plan->sc;
        plan->stamp = ++c->agg_plans->clock;
        ++c->agg_plans->hits;
        Tape& t = sc->s.tape;
        for (const AggPlan::ScalarPatch& sp : plan->scalars)
            t.set_const(sp.reg, circuits[sp.circuit].transcripts[sp.proof] + sp.off);
        for (const AggPlan::PointPatch& pp : plan->points)
            memcpy(sc->s.points.data() + 64 * (size_t)pp.slot, (pp.kind ? H[pp.circuit].inst_aff.data() : H[pp.circuit].points.data()) + pp.off, 64);
        sc->tape_done_ops = (size_t)-1;   // the register file on the device holds the previous call's values
        trace.mark("plan_refill");
    } else {
    TRY(h2agg_schema_create(c, &sc));
    guard.s = sc;
    Schema& S = sc->s;
    S.track_src = true;
    // ---- host: the reference's control flow over tape registers
    Rec R(S);
    std::vector<AggPlan::ChalPatch>& patches = fresh.chal;
    std::vector<std::pair<uint32_t, uint32_t>> proofs;   // (w_x, w_g) per proof, in aggregation order
    each_idx.clear();
    for (size_t ci = 0; ci < ncircuits; ++ci) {
        const h2agg_circuit_proofs& cp = circuits[ci];
        const h2agg_vk& vk = *cp.vk;
        const CircuitHost& h = H[ci];
        // the W commitments must be one per rotation group (multiopen.rs:48); checked by batch_multi_open below
        for (size_t i = 0; i < cp.nproofs; ++i) {
            const uint8_t* proof = cp.transcripts[i];
            const uint8_t* pts = h.points.data() + 64 * h.npoints * i;
            ProofRegs P;
            // scalars of the proof, in reading order
            size_t soff = 0;
            {
                size_t before = 0;   // byte offset of the first scalar = point bytes * (#P before the evals)
                for (char ch : h.script) {
                    if (ch == 'S') break;
                    if (ch == 'P') ++before;
                }
                soff = proof_point_bytes(vk) * before;
            }
            auto next_scalar = [&] {   // (a register of its own, whatever its value: see AggPlan)
                const uint32_t r = S.tape.add_const_placeholder();
                S.tape.set_const(r, proof + soff);
                fresh.scalars.push_back({r, (uint32_t)ci, (uint32_t)i, (uint32_t)soff});
                soff += 32;
                return r;
            };
            size_t qn = 0;
            auto next_chal = [&] {
                const uint32_t reg = S.tape.add_const_placeholder();
                patches.push_back({reg, (uint32_t)ci, 32 * (h.nsq * i + qn++)});
                return reg;
            };
            P.challenges.assign(vk.num_challenges, R.cu64(0));
            for (uint32_t phase = 0; phase <= vk.max_phase; ++phase)
                for (uint32_t k2 = 0; k2 < vk.num_challenges; ++k2)
                    if (vk.challenge_phase[k2] == phase) P.challenges[k2] = next_chal();
            P.theta = next_chal();
            P.beta = next_chal();
            P.gamma = next_chal();
            P.y = next_chal();
            P.x = next_chal();
            P.v = next_chal();
            P.u = next_chal();
            for (size_t q = 0; q < vk.instance_q.size(); ++q) P.instance_evals.push_back(next_scalar());
            for (size_t q = 0; q < vk.advice_q.size(); ++q) P.advice_evals.push_back(next_scalar());
            for (size_t q = 0; q < vk.fixed_q.size(); ++q) P.fixed_evals.push_back(next_scalar());
            P.random_eval = next_scalar();
            for (size_t q = 0; q < vk.perm_commitments.size() / 64; ++q) P.permutation_evals.push_back(next_scalar());
            for (uint32_t si = 0; si < vk.n_sets; ++si) {                      // verify.rs:215-237
                ProofRegs::Set st;
                st.eval = next_scalar();
                st.next = next_scalar();
                st.last = si + 1 < vk.n_sets ? next_scalar() : ~0u;
                P.sets.push_back(st);
            }
            for (size_t j = 0; j < vk.lookups.size(); ++j) {                   // verify.rs:308-312
                ProofRegs::Lk lk;
                lk.product = next_scalar();
                lk.product_next = next_scalar();
                lk.input = next_scalar();
                lk.input_inv = next_scalar();
                lk.table = next_scalar();
                P.lookups.push_back(lk);
            }
            const std::string key = std::string(cp.name) + "_p" + std::to_string(i);   // verify_circuit.rs:140
            std::vector<Query> qs;
            TRY(build_queries(c, S, vk, key, P, h.inst_aff.data() + 64 * vk.num_instance * i, pts, qs));
            std::vector<int32_t> rot(qs.size());
            std::vector<uint32_t> preg(qs.size()), qnode(qs.size());
            for (size_t q = 0; q < qs.size(); ++q) {
                rot[q] = qs[q].rotation;
                preg[q] = qs[q].point_reg;
                qnode[q] = qs[q].node;
            }
            const uint8_t* w = pts + 64 * (h.npoints - h.n_w);
            uint32_t w_x = 0, w_g = 0;
            if (!S.batch_multi_open_regs(key.c_str(), qs.size(), rot.data(), preg.data(), qnode.data(), h.n_w, w, P.v, P.u, w_x, w_g)) {
                if (!each) return fail(c, H2AGG_ERR_INVALID, S.err);
                each->status[h.first_proof + i] = H2AGG_ERR_INVALID;   // (this proof only: the others go on)
                continue;
            }
            proofs.push_back({w_x, w_g});
            if (each) each_idx.push_back(h.first_proof + i);
        }
    }
    trace.mark("host_queries");
    if (each) {
        each_roots = proofs;
        fresh.sc = sc;
        plan = &fresh;
    } else {
    // ---- acc = acc * lambda + proof  (verify.rs:926-938)
    // Recorded in its distributed form  sum_i lambda^(N-1-i) * proof_i  (what the nested fold expands to; field arithmetic is
    // exact, the entries keep the fold's order): every proof's entries meet ONE factor, lambda^e built by halving, instead of
    // being multiplied through once per later proof — the nested form costs O(N^2) tape operations (4 ms of host time and a
    // 700 k-operation tape at 64 proofs).
    const size_t np = proofs.size();
    const uint32_t lam_reg = S.tape.add_const_placeholder();
    auto weighted = [&](uint32_t node, size_t i) {   // (a shard: i-th LOCAL proof, exponent from its place in the whole aggregation)
        const uint32_t e = (uint32_t)(N_all - 1 - (shard ? (size_t)shard->global_index[i] : i));
        if (e == 0) return node;
        return S.add_binary(SchemaNode::MUL, node, S.add_leaf_reg(SchemaNode::SCALAR, S.tape.pow(lam_reg, e)));
    };
    uint32_t acc_x = weighted(proofs[0].first, 0), acc_g = weighted(proofs[0].second, 0);
    for (size_t i = 1; i < np; ++i) {
        acc_x = S.add_binary(SchemaNode::ADD, acc_x, weighted(proofs[i].first, i));
        acc_g = S.add_binary(SchemaNode::ADD, acc_g, weighted(proofs[i].second, i));
    }
    // the host half of the evaluation (both eval_prepare walks, the tape's dependency levels): still under the sponges
    TRY(h2agg_evaluate_multiopen_prepare(sc, acc_x, acc_g));
    trace.mark("host_prepare");
    if (trace.on) {
        char buf[160];
        snprintf(buf, sizeof buf, " [tape: %zu ops, %u levels, %u consts, %u live at once: %s]", S.tape.ops.size(), sc->prep.tape.maxlevel,
                 S.tape.nconst, sc->prep.tape.lds_peak, sc->prep.tape.lds ? "register file in LDS" : "register file in L2");
        trace.line += buf;
    }
    // where the points came from: this call's decompressed proof points / instance commitments (refilled next time) or the
    // verifying key's own commitments (constant)
    // Every commitment the recording refers to must be accounted for: per-call data (refilled on a hit) or the verifying
    // key's own (constant for the key).  A point copied in from anywhere else would be frozen into the recording as the first
    // call's value — such a recording is used once and not kept (ADVICE r3).
    auto inside = [](const uint8_t* p, const std::vector<uint8_t>& v) { return !v.empty() && p >= v.data() && p + 64 <= v.data() + v.size(); };
    for (size_t slot = 0; slot < S.point_src.size(); ++slot) {
        const uint8_t* src = S.point_src[slot];
        bool known = false;
        for (size_t ci = 0; ci < ncircuits && !known; ++ci) {
            const CircuitHost& h = H[ci];
            if (inside(src, h.points)) {
                fresh.points.push_back({(uint32_t)slot, (uint32_t)ci, 0, (size_t)(src - h.points.data())});
                known = true;
            } else if (inside(src, h.inst_aff)) {
                fresh.points.push_back({(uint32_t)slot, (uint32_t)ci, 1, (size_t)(src - h.inst_aff.data())});
                known = true;
            } else if (inside(src, circuits[ci].vk->fixed_commitments) || inside(src, circuits[ci].vk->perm_commitments)) {
                known = true;
            }
        }
        if (!known) fresh.cacheable = false;
    }
    S.track_src = false;
    S.point_src.clear();
    S.point_src.shrink_to_fit();
    fresh.sig = sig;
    fresh.sc = sc;
    fresh.lam_reg = lam_reg;
    fresh.acc_x = acc_x;
    fresh.acc_g = acc_g;
    plan = &fresh;
    }   // (aggregation)
    }   // (recorded afresh)
    Schema& S = sc->s;
    const uint32_t lam_reg = plan->lam_reg, acc_x = plan->acc_x, acc_g = plan->acc_g;
    if (host_sponge) {
        pool_scope.p = nullptr;
        pool.end(pool_scope.r);   // this thread takes whatever chains are left, then waits for the rest
        for (size_t j = 0; j < job_of.size(); ++j) {
            const CircuitHost& h = H[job_of[j].first];
            memcpy(agg_host.data() + 32 * j, h.chal.data() + 32 * (h.nsq * job_of[j].second + h.nsq - 1), 32);
        }
        const uint32_t upto = (uint32_t)total_proofs;
        host_flags |= sponge_bad.load();
        if (!shard && !each) host_flags |= poseidon_run_host(agg_host.data(), 32 * total_proofs, &upto, 1, 1, lambda, 1);
        trace.mark("sponge_wait");
        TRY(finish(c, host_flags));   // every transcript has run: bad point encodings / non-canonical scalars surface here
    }
    if (shard) {   // exchange 1: every rank's squeezes -> the same lambda on every rank
        if (!host_sponge) {
            agg_host.resize(total_proofs * 32);
            size_t j = 0;
            for (size_t ci = 0; ci < ncircuits; ++ci)
                for (size_t i = 0; i < circuits[ci].nproofs; ++i, ++j)
                    memcpy(agg_host.data() + 32 * j, H[ci].chal.data() + 32 * (H[ci].nsq * i + H[ci].nsq - 1), 32);
        }
        TRY(exchange1(agg_host.data(), total_proofs, lambda));
        trace.mark("lambda_exchange");
        if (c->dbg_shard_fail == 2) return fail(c, H2AGG_ERR_INVALID, "injected failure between the exchanges (debug key shard_fail)");
    }
    for (const AggPlan::ChalPatch& pt : plan->chal) S.tape.set_const(pt.reg, H[pt.circuit].chal.data() + pt.off);
    if (each) {   // verify_single_proof_in_chip: every proof's own evaluate_multiopen_proof, 2N sides in one set of launches
        if (each_roots.empty()) return H2AGG_OK;
        std::vector<uint8_t> pairs(128 * each_roots.size());
        TRY(evaluate_multiopen_many(sc, each_roots, pairs.data()));
        for (size_t k = 0; k < each_idx.size(); ++k) memcpy(each->pairs + 128 * each_idx[k], pairs.data() + 128 * k, 128);
        trace.mark("evaluate");
        return H2AGG_OK;
    }
    if (lambda_out) memcpy(lambda_out, lambda, 32);
    S.tape.set_const(lam_reg, lambda);
    // (the pairing behind the evaluation wants one worker awake: its second pair's Miller loop runs there)
    if (s_g2 && !shard && c->dbg_prewake) HostPool::get().prewake(1);
    const int rc_eval = h2agg_evaluate_multiopen_proof(sc, acc_x, acc_g, left_aff, right_aff);
    if (plan == &fresh && cache_on && fresh.cacheable && (rc_eval == H2AGG_OK || rc_eval == H2AGG_ERR_NONCANONICAL || rc_eval == H2AGG_ERR_DIV_ZERO)) {
        // (the recording is good whatever this call's VALUES were) keep it for the next call of this shape
        if (!c->agg_plans) c->agg_plans = new AggPlanCache();
        AggPlanCache& pc = *c->agg_plans;
        ++pc.misses;
        if (pc.plans.size() >= AggPlanCache::MAX_PLANS) {
            size_t lru = 0;
            for (size_t k = 1; k < pc.plans.size(); ++k)
                if (pc.plans[k].stamp < pc.plans[lru].stamp) lru = k;
            h2agg_schema_destroy(pc.plans[lru].sc);
            pc.plans.erase(pc.plans.begin() + (long)lru);
        }
        fresh.stamp = ++pc.clock;
        pc.plans.push_back(std::move(fresh));
        guard.s = nullptr;   // the cache owns the schema now
    }
    TRY(rc_eval);
    trace.mark("evaluate");
    if (shard) {
        if (s_g2 && c->dbg_prewake) HostPool::get().prewake(1);   // (the pairing's second Miller loop; the exchange is ~0.1 ms)
        TRY(exchange2());
        trace.mark("pair_exchange");
    }
    if (s_g2) TRY(h2agg_final_pair_check(c, left_aff, right_aff, s_g2, g2, pairing_ok));
    trace.mark("pairing");
    return H2AGG_OK;
    };   // body
    int rc;
    try {
        rc = body();
    } catch (const std::bad_alloc&) {
        rc = fail(c, H2AGG_ERR_NOMEM, "out of host memory");
    } catch (...) {
        rc = fail(c, H2AGG_ERR_INVALID, "unexpected exception");
    }
    if (shard && rc != H2AGG_OK && !xs.global && !(xs.ex1 && xs.ex2)) {
        const std::string why = c->err;   // (the exchange below must not replace this rank's own message)
        try {
            if (!xs.ex1) {       // the others learn it in exchange 1 and leave there: no exchange 2 for anybody
                uint8_t lam0[32];
                uint32_t fl = 0;
                (void)shard_lambda(c, shard, N_all, nullptr, 0, lam0, fl, (uint32_t)rc);
            } else {             // ... in exchange 2
                uint8_t l0[64] = {}, r0[64] = {};
                (void)shard_sum_pair(c, shard, l0, r0, (uint32_t)rc);
            }
        } catch (...) {
        }
        c->err = why;
    }
    return rc;
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

}  // extern "C"

namespace {
// e(left_i, s_g2) * e(right_i, -g2) == 1 for every proof whose status is OK, one proof per job on the host pool; the prepared
// lines of s_g2 and -g2 are made once for all of them
template <class P>
int pair_checks_t(h2agg_ctx* c, const uint8_t* pairs, const int32_t* status, size_t n, const uint8_t s_g2[128], const uint8_t g2[128],
                  int* ok) {
    std::vector<typename P::G1> ps(2 * n);
    std::vector<typename P::G2> qs(2);
    uint8_t g2s[256];
    memcpy(g2s, s_g2, 128);
    memcpy(g2s + 128, g2, 128);
    {   // (the G2 points' checks, beside the generator of G1)
        uint8_t gen2[128] = {0};
        gen2[0] = gen2[64] = 1;
        gen2[32] = gen2[96] = 2;
        std::vector<typename P::G1> p0;
        TRY(pairing_load<P>(c, gen2, g2s, 2, p0, qs));
    }
    P::negate(qs[1]);
    const std::shared_ptr<const typename P::Prepared> keep[2] = {P::prepared(s_g2, false, qs[0]), P::prepared(g2, true, qs[1])};
    const std::vector<const typename P::Prepared*> preps = {keep[0].get(), keep[1].get()};
    std::vector<size_t> todo;
    for (size_t i = 0; i < n; ++i) {
        ok[i] = 0;
        if (status[i] != H2AGG_OK) continue;
        for (int side = 0; side < 2; ++side) {
            const int r = P::load1(pairs + 128 * i + 64 * side, ps[2 * i + side]);
            if (r == 1) return fail(c, H2AGG_ERR_HIP, "pairing: an evaluated G1 coordinate is >= p");
            if (r) return fail(c, H2AGG_ERR_HIP, "pairing: an evaluated G1 point is not on the curve");
        }
        todo.push_back(i);
    }
    HostPool::get().run(todo.size(), HostPool::get().size(), [&](size_t j) {
        const size_t i = todo[j];
        ok[i] = P::check_prepared(std::vector<typename P::G1>{ps[2 * i], ps[2 * i + 1]}, preps) ? 1 : 0;
    });
    return H2AGG_OK;
}
}  // namespace

extern "C" {

int h2agg_verify_proofs(h2agg_ctx* c, const h2agg_circuit_proofs* circuits, size_t ncircuits, const uint8_t* s_g2, const uint8_t* g2,
                        uint8_t* left_aff, uint8_t* right_aff, int32_t* status, int* pairing_ok, uint8_t* advice_out,
                        size_t advice_cap) try {
    TRY(bind(c));
    if (!circuits || ncircuits == 0 || !left_aff || !right_aff || !status) return fail(c, H2AGG_ERR_INVALID, "null argument");
    if ((s_g2 == nullptr) != (g2 == nullptr) || (s_g2 && !pairing_ok))
        return fail(c, H2AGG_ERR_INVALID, "pass s_g2, g2 and pairing_ok together (or none)");
    size_t N = 0, advice_need = 0;
    std::vector<size_t> advice_at;   // byte offset of every proof's advice commitments in advice_out
    for (size_t ci = 0; ci < ncircuits; ++ci) {
        const h2agg_circuit_proofs& cp = circuits[ci];
        if (!cp.vk || cp.vk->ctx != c || !cp.name) return fail(c, H2AGG_ERR_INVALID, "circuit without a verifying key / name");
        if (cp.nproofs == 0) continue;
        const h2agg_vk& vk = *cp.vk;
        if (!cp.transcripts || !cp.transcript_lens || (vk.num_instance && (!cp.instances || !cp.instance_lens)))
            return fail(c, H2AGG_ERR_INVALID, "null proof data");
        if (vk.num_instance && c->tables.find(cp.g_lagrange) == c->tables.end()) return fail(c, H2AGG_ERR_INVALID, "unknown g_lagrange handle");
        for (size_t i = 0; i < cp.nproofs; ++i) {
            if (!cp.transcripts[i]) return fail(c, H2AGG_ERR_INVALID, "null proof data");
            size_t pl = 0;
            for (size_t col = 0; col < vk.num_instance; ++col) pl += cp.instance_lens[i * vk.num_instance + col];
            if (pl && !cp.instances[i]) return fail(c, H2AGG_ERR_INVALID, "null instance data");
            advice_at.push_back(advice_need);
            advice_need += (size_t)vk.num_advice * 64;
        }
        N += cp.nproofs;
    }
    if (N == 0) return fail(c, H2AGG_ERR_INVALID, "no proofs");
    if (advice_out && advice_need > advice_cap) return fail(c, H2AGG_ERR_INVALID, "advice_out is too small for the proofs' advice commitments");
    memset(left_aff, 0, 64 * N);
    memset(right_aff, 0, 64 * N);
    if (pairing_ok) memset(pairing_ok, 0, sizeof(int) * N);
    if (advice_out) memset(advice_out, 0, advice_need);
    for (size_t i = 0; i < N; ++i) status[i] = H2AGG_OK;
    // ---- what is decided by a proof's shape alone (verify.rs:487-490, :601-603): that proof's status, before any work
    struct Item { size_t ci, i, g; };
    std::vector<Item> items;
    {
        size_t g = 0;
        for (size_t ci = 0; ci < ncircuits; ++ci) {
            const h2agg_circuit_proofs& cp = circuits[ci];
            if (cp.nproofs == 0) continue;
            const h2agg_vk& vk = *cp.vk;
            const uint64_t max_len = ((uint64_t)1 << vk.k) - (vk.blinding_factors + 1);
            const size_t table_n = vk.num_instance ? c->tables.find(cp.g_lagrange)->second.n : 0;
            for (size_t i = 0; i < cp.nproofs; ++i, ++g) {
                const size_t plen = cp.transcript_lens[i];
                bool bad = !proof_len_fits(vk, plen, nullptr);
                for (size_t col = 0; col < vk.num_instance; ++col) {
                    const uint32_t l = cp.instance_lens[i * vk.num_instance + col];
                    if (l > max_len || l > table_n) bad = true;
                }
                if (bad) status[g] = H2AGG_ERR_INVALID;
                else items.push_back({ci, i, g});
            }
        }
    }
    // ---- one verify_aggregation_impl call (per-proof mode) over a list of proofs: each circuit's proofs grouped by length
    // (the device transcripts take one length per launch); results scattered back to the proofs' places
    std::vector<uint8_t> pairs(128 * N);
    auto run = [&](const std::vector<Item>& list) -> int {
        std::vector<h2agg_circuit_proofs> sub;
        std::vector<std::string> names;
        std::vector<std::vector<const uint8_t*>> tr, in;
        std::vector<std::vector<size_t>> lens;
        std::vector<std::vector<uint32_t>> ilens;
        std::vector<size_t> order;   // the call's proof j -> the item's place g
        std::vector<bool> taken(list.size(), false);
        for (size_t a = 0; a < list.size(); ++a) {
            if (taken[a]) continue;
            const h2agg_circuit_proofs& cp = circuits[list[a].ci];
            const size_t plen = cp.transcript_lens[list[a].i], ncol = cp.vk->num_instance;
            tr.emplace_back();
            in.emplace_back();
            lens.emplace_back();
            ilens.emplace_back();
            for (size_t b = a; b < list.size(); ++b) {
                if (taken[b] || list[b].ci != list[a].ci || cp.transcript_lens[list[b].i] != plen) continue;
                taken[b] = true;
                tr.back().push_back(cp.transcripts[list[b].i]);
                lens.back().push_back(plen);
                if (ncol) {
                    in.back().push_back(cp.instances[list[b].i]);
                    for (size_t col = 0; col < ncol; ++col) ilens.back().push_back(cp.instance_lens[list[b].i * ncol + col]);
                }
                order.push_back(list[b].g);
            }
            // (a circuit split by length: every group's keys of its own, "{name}_p{i}" must not meet twice in one schema)
            names.push_back(std::string(cp.name) + "#" + std::to_string(names.size()));
            h2agg_circuit_proofs g = cp;
            g.nproofs = tr.back().size();
            sub.push_back(g);
        }
        for (size_t k = 0; k < sub.size(); ++k) {
            sub[k].name = names[k].c_str();
            sub[k].transcripts = tr[k].data();
            sub[k].transcript_lens = lens[k].data();
            sub[k].instances = in[k].empty() ? nullptr : in[k].data();
            sub[k].instance_lens = ilens[k].empty() ? nullptr : ilens[k].data();
        }
        const size_t n = order.size();
        std::vector<uint8_t> p(128 * n, 0), adv;
        std::vector<int32_t> st(n, H2AGG_OK);
        size_t adv_need = 0;
        for (const h2agg_circuit_proofs& g : sub) adv_need += g.nproofs * (size_t)g.vk->num_advice * 64;
        if (advice_out) adv.resize(adv_need + 1);
        EachOut eo{p.data(), st.data()};
        uint8_t l0[64], r0[64];
        const int rc = verify_aggregation_impl(c, sub.data(), sub.size(), nullptr, nullptr, nullptr, l0, r0, nullptr, nullptr,
                                               advice_out ? adv.data() : nullptr, adv_need, &eo);
        if (rc != H2AGG_OK) return rc;
        size_t aoff = 0;
        for (size_t j = 0; j < n; ++j) {
            const size_t g = order[j];
            status[g] = st[j];
            if (st[j] == H2AGG_OK) memcpy(pairs.data() + 128 * g, p.data() + 128 * j, 128);
        }
        if (advice_out) {   // (in the call's order: circuit groups, proofs in order)
            for (size_t j = 0; j < n; ++j) {
                const size_t g = order[j];
                size_t ci = 0, base = 0;
                while (g >= base + circuits[ci].nproofs) base += circuits[ci++].nproofs;
                const size_t bytes = (size_t)circuits[ci].vk->num_advice * 64;
                if (st[j] == H2AGG_OK) memcpy(advice_out + advice_at[g], adv.data() + aoff, bytes);
                aoff += bytes;
            }
        }
        return H2AGG_OK;
    };
    if (!items.empty()) {
        const int rc = run(items);
        if (rc == H2AGG_ERR_BAD_POINT || rc == H2AGG_ERR_NONCANONICAL) {
            // a proof's bytes do not decode (the device's flags are batch-wide): verify the proofs one by one to name it
            for (const Item& it : items) {
                const int r1 = run(std::vector<Item>{it});
                if (r1 == H2AGG_ERR_BAD_POINT || r1 == H2AGG_ERR_NONCANONICAL || r1 == H2AGG_ERR_INVALID || r1 == H2AGG_ERR_EMPTY)
                    status[it.g] = r1;
                else if (r1 != H2AGG_OK)
                    return r1;
            }
        } else if (rc != H2AGG_OK) {
            return rc;
        }
    }
    for (size_t g = 0; g < N; ++g) {
        memcpy(left_aff + 64 * g, pairs.data() + 128 * g, 64);
        memcpy(right_aff + 64 * g, pairs.data() + 128 * g + 64, 64);
    }
    // (h2agg_last_phases: the phases of the per-proof verification as the aggregation names them, then the pairings)
    if (s_g2) {
        const auto t0 = std::chrono::steady_clock::now();
        int rc;
#ifdef H2AGG_PAIRING_ADX_BUILD
        if (pairing_adx_ok()) rc = pair_checks_t<pairing_adx::Api>(c, pairs.data(), status, N, s_g2, g2, pairing_ok);
        else
#endif
        rc = pair_checks_t<pairing::Api>(c, pairs.data(), status, N, s_g2, g2, pairing_ok);
        TRY(rc);
        if (c->dbg_phases) {
            char buf[64];
            snprintf(buf, sizeof buf, " pairing=%.3f", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            c->last_phases += buf;
        }
    }
    return H2AGG_OK;
} catch (const std::bad_alloc&) {
    return H2AGG_ERR_NOMEM;   // no C++ exception crosses the C ABI
} catch (...) {
    return H2AGG_ERR_INVALID;
}

int h2agg_verify_plan_stats(h2agg_ctx* c, uint64_t* hits, uint64_t* misses, uint64_t* plans_kept) {
    if (!c) return H2AGG_ERR_INVALID;
    const AggPlanCache* pc = c->agg_plans;
    if (hits) *hits = pc ? pc->hits : 0;
    if (misses) *misses = pc ? pc->misses : 0;
    if (plans_kept) *plans_kept = pc ? pc->plans.size() : 0;
    return H2AGG_OK;
}

const char* h2agg_last_phases(h2agg_ctx* c) { return c ? c->last_phases.c_str() : ""; }

int h2agg_verify_aggregation_ex(h2agg_ctx* c, const h2agg_circuit_proofs* circuits, size_t ncircuits, const uint8_t* s_g2,
                                const uint8_t* g2, uint8_t left_aff[64], uint8_t right_aff[64], uint8_t lambda_out[32],
                                int* pairing_ok, uint8_t* advice_out, size_t advice_cap) {
    return verify_aggregation_impl(c, circuits, ncircuits, nullptr, s_g2, g2, left_aff, right_aff, lambda_out, pairing_ok, advice_out, advice_cap);
}

int h2agg_verify_aggregation(h2agg_ctx* c, const h2agg_circuit_proofs* circuits, size_t ncircuits, const uint8_t* s_g2,
                             const uint8_t* g2, uint8_t left_aff[64], uint8_t right_aff[64], uint8_t lambda_out[32],
                             int* pairing_ok) {
    return verify_aggregation_impl(c, circuits, ncircuits, nullptr, s_g2, g2, left_aff, right_aff, lambda_out, pairing_ok, nullptr, 0);
}

int h2agg_verify_aggregation_sharded(h2agg_ctx* c, const h2agg_circuit_proofs* circuits, size_t ncircuits, const h2agg_shard* shard,
                                     const uint8_t* s_g2, const uint8_t* g2, uint8_t left_aff[64], uint8_t right_aff[64],
                                     uint8_t lambda_out[32], int* pairing_ok, uint8_t* advice_out, size_t advice_cap) {
    if (!c) return H2AGG_ERR_INVALID;
    if (!shard) return fail(c, H2AGG_ERR_INVALID, "null shard description");
    return verify_aggregation_impl(c, circuits, ncircuits, shard, s_g2, g2, left_aff, right_aff, lambda_out, pairing_ok, advice_out, advice_cap);
}

}  // extern "C"
