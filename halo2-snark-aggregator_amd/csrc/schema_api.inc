// C ABI of the schema layer (included into h2agg.hip: shares the context internals).
// EvaluationQuerySchema::eval (evaluation.rs:172-203) and evaluate_multiopen_proof (verify.rs:705-731).

struct EvalLists {
    std::vector<uint8_t> pts_s;       // points that carry a scalar (64 B each)
    std::vector<uint32_t> regs_s;     // their scalar registers (tape ids, resolved at run time)
    std::vector<uint8_t> pts_ns;      // scalar-less points
    std::vector<int32_t> pidx_s, pidx_ns;   // where those points live in Schema::points (a prepared evaluation re-reads them)
    int64_t e_reg = -1;               // scalar of the "" entry (tape id), -1 = None
    std::vector<uint32_t> names;      // interned key ids
};

struct h2agg_schema {
    h2agg_ctx* ctx;
    Schema s;
    // what the register file on the device (ctx->sch_regs, valid while ctx->sch_owner == this) reflects
    size_t tape_done_ops = (size_t)-1, tape_done_consts = (size_t)-1;
    const uint8_t* side_xyzz[2] = {nullptr, nullptr};   // per side of evaluate_multiopen_proof: MSM result slot,
    const uint8_t* side_pns[2] = {nullptr, nullptr};    // scalar-less points (device)
    size_t side_k[2] = {0, 0};
    // h2agg_evaluate_multiopen_prepare: the host half of evaluate_multiopen_proof done ahead of time (both eval_prepare
    // walks, the tape's dependency levels).  Good for the roots and the schema / tape sizes it was made for; commitment
    // POINTS may still change (h2agg_schema_query_set_commitment): they are read again when the evaluation runs.
    struct Prep {
        bool valid = false;
        uint32_t w_x = 0, w_g = 0;
        size_t nodes_n = 0, ops_n = 0, consts_n = 0;
        EvalLists L[2];
        int64_t extra[2] = {-1, -1};
        std::vector<uint32_t> all_names;
        CompiledTape tape;
    } prep;
};

namespace {

// host half of eval(): eval_prepare + the partition of evaluation.rs:183-196
int eval_lists(h2agg_schema* sc, uint32_t node, EvalLists& L) {
    Schema& S = sc->s;
    if (!S.valid(node)) return fail(sc->ctx, H2AGG_ERR_INVALID, "unknown schema node");
    Prepared pr;
    if (!S.eval_prepare(node, -1, pr)) return fail(sc->ctx, H2AGG_ERR_INVALID, S.err);
    bool have_e = false;
    L.names.reserve(pr.v.size());
    L.pts_s.reserve(pr.v.size() * 64 + 64);
    L.regs_s.reserve(pr.v.size() + 1);
    for (PreparedEntry& e : pr.v) {
        if (e.scalar >= 0) e.scalar = (int64_t)S.tape.materialize((uint32_t)e.scalar);   // deferred sums -> registers
        L.names.push_back(e.key);
        if (e.key == 0 && !have_e) {                          // .find(|b| b.0.is_empty())  :185-188
            have_e = true;
            L.e_reg = e.scalar;
        }
        if (e.point >= 0) {
            const uint8_t* p = S.points.data() + 64 * (size_t)e.point;
            if (e.scalar < 0) {
                L.pts_ns.insert(L.pts_ns.end(), p, p + 64);   // p_wo_scalar  :189-192
                L.pidx_ns.push_back(e.point);
            } else {
                L.pts_s.insert(L.pts_s.end(), p, p + 64);     // (p_l, s_l)   :193-196
                L.pidx_s.push_back(e.point);
                L.regs_s.push_back((uint32_t)e.scalar);
            }
        }
    }
    return H2AGG_OK;
}

// The tape's part of a staging block and of the launches behind it: every caller packs what the device needs into ONE pinned
// block (256-byte aligned regions; the tape's four first, the caller's own behind them), uploads it with ONE copy, then runs the
// tape.
size_t stage_align(size_t x) { return (x + 255) & ~(size_t)255; }
struct TapeOffsets {
    size_t consts = 0, ops = 0, lvl = 0, cslot = 0;
};
TapeOffsets tape_layout(size_t& off, const CompiledTape& ct, uint32_t nconst) {
    TapeOffsets o;
    o.consts = off;  off = stage_align(off + (size_t)nconst * 32);
    o.ops = off;     off = stage_align(off + ct.sorted.size() * sizeof(TapeOp));
    o.lvl = off;     off = stage_align(off + ct.lstart.size() * 4);
    o.cslot = off;   off = stage_align(off + ct.cslot.size() * 4);
    return o;
}
void tape_fill(uint8_t* h, const TapeOffsets& o, const CompiledTape& ct, const uint8_t* consts, uint32_t nconst) {
    if (nconst) memcpy(h + o.consts, consts, (size_t)nconst * 32);
    if (!ct.sorted.empty()) memcpy(h + o.ops, ct.sorted.data(), ct.sorted.size() * sizeof(TapeOp));
    if (!ct.lstart.empty()) memcpy(h + o.lvl, ct.lstart.data(), ct.lstart.size() * 4);
    if (!ct.cslot.empty()) memcpy(h + o.cslot, ct.cslot.data(), ct.cslot.size() * 4);
}
// d: the uploaded block on the device.  Fills c->sch_regs (the caller has sized it) on the context's stream.
void tape_launch(h2agg_ctx* c, const uint8_t* d, const TapeOffsets& o, const CompiledTape& ct, uint32_t nconst) {
    hipStream_t st = c->stream;
    uint32_t* regs = (uint32_t*)c->sch_regs.p;
    if (ct.lds) {   // constants + every level in one launch, the register file in LDS (schema.hpp)
        hipLaunchKernelGGL(k_tape_run_lds, dim3(1), dim3(TAPE_THREADS), 0, st, d + o.consts, (const uint32_t*)(d + o.cslot), nconst,
                           (const TapeOp*)(d + o.ops), (const uint32_t*)(d + o.lvl), ct.maxlevel, regs, c->d_flags);
        return;
    }
    if (nconst)
        hipLaunchKernelGGL(k_tape_load_consts, dim3((nconst + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, d + o.consts, nconst, regs,
                           c->d_flags);
    if (!ct.sorted.empty())
        hipLaunchKernelGGL(k_tape_run, dim3(1), dim3(TAPE_THREADS), 0, st, (const TapeOp*)(d + o.ops), (const uint32_t*)(d + o.lvl),
                           ct.maxlevel, regs, c->d_flags);
}

// (X, Y, ZZ, ZZZ) as the device leaves its results (128 B each, canonical) -> affine x = X / ZZ, y = Y / ZZZ (64 B each; the
// identity: zeros, as the device's affine store writes it).  The division happens on the host: ONE field inversion for all n
// (Montgomery's trick) is ~10 us on a host core and ~55 us of a lone wave's latency on the device, at the very end of an
// evaluation's chain.  false: a coordinate is not canonical.
bool xyzz_to_affine(const uint8_t* xyzz, size_t n, uint8_t* out_aff) {
    namespace pr = h2agg::pairing;
    struct Pt {
        pr::Fq X, Y, ZZ, ZZZ, before;   // before: the product of the earlier points' denominators
    };
    Pt two[2];   // (the two sides of one evaluation: no allocation)
    std::vector<Pt> many(n > 2 ? n : 0);
    Pt* p = n > 2 ? many.data() : two;
    pr::Fq acc = pr::fq_one();
    for (size_t s = 0; s < n; ++s) {
        const uint8_t* o = xyzz + 128 * s;
        if (!pr::fq_from_bytes(o, p[s].X) || !pr::fq_from_bytes(o + 32, p[s].Y) || !pr::fq_from_bytes(o + 64, p[s].ZZ) ||
            !pr::fq_from_bytes(o + 96, p[s].ZZZ))
            return false;
        p[s].before = acc;
        if (!pr::fq_is_zero(p[s].ZZ)) acc = pr::fq_mul(acc, pr::fq_mul(p[s].ZZ, p[s].ZZZ));
    }
    pr::Fq inv = pr::fq_inv(acc);   // 1 / prod(ZZ ZZZ)
    memset(out_aff, 0, 64 * n);
    for (size_t s = n; s-- > 0;) {
        if (pr::fq_is_zero(p[s].ZZ)) continue;
        const pr::Fq dinv = pr::fq_mul(inv, p[s].before);                      // 1 / (ZZ_s ZZZ_s)
        inv = pr::fq_mul(inv, pr::fq_mul(p[s].ZZ, p[s].ZZZ));
        pr::fq_to_bytes(pr::fq_mul(p[s].X, pr::fq_mul(dinv, p[s].ZZZ)), out_aff + 64 * s);        // X / ZZ
        pr::fq_to_bytes(pr::fq_mul(p[s].Y, pr::fq_mul(dinv, p[s].ZZ)), out_aff + 64 * s + 32);   // Y / ZZZ
    }
    return true;
}

// Device half of eval(), for one evaluation or for the two sides of evaluate_multiopen_proof at once.
// Everything the device needs (tape constants, the tape sorted by dependency level, per side the scalar
// register indices, the points and the scalar-less points) is packed into ONE pinned staging block and uploaded
// with ONE copy; then: tape -> gather the scalars -> multi_exp per side, all queued without a host wait (the MSM
// tails overlap on the tail streams).  extra_* optionally folds one more (point, register) pair into a side's
// multi_exp (+/- e*G in evaluate_multiopen_proof).
int eval_launch_sides(h2agg_schema* sc, EvalLists* L, int nsides, const uint8_t* const* extra_pt, const int64_t* extra_reg,
                      const h2agg_schema::Prep* pre = nullptr) {
    h2agg_ctx* c = sc->ctx;
    Schema& S = sc->s;
    Tape& t = S.tape;
    for (int s = 0; s < nsides; ++s)
        if (L[s].regs_s.empty())                              // pchip.multi_exp(ctx, [], []) panics
            return fail(c, H2AGG_ERR_EMPTY, "multi_exp of zero pairs (reference panics: mock/arith/ecc.rs:128)");
    // ---- the tape is final from here on: its dependency levels (the prepared ones, if they are this tape's)
    const uint32_t nconst = t.nconst, nops = (uint32_t)t.ops.size(), nreg = nconst + nops;
    const bool need_tape = !(c->sch_owner == sc && sc->tape_done_ops == nops && sc->tape_done_consts == nconst);
    const bool use_prepared = need_tape && pre && pre->ops_n == nops && pre->consts_n == nconst && pre->tape.sorted.size() == nops;
    CompiledTape own;
    if (need_tape && !use_prepared && !compile_tape(t.resolved_ops(), nconst, c->dbg_tape_lds, own))
        return fail(c, H2AGG_ERR_INVALID, "tape: operand not yet defined");
    const CompiledTape& ct = use_prepared ? pre->tape : own;   // (by reference: an aggregation's tape is megabytes)
    // ---- staging layout
    size_t off = 0;
    TapeOffsets to;
    if (need_tape) to = tape_layout(off, ct, nconst);
    size_t off_idx[2] = {0, 0}, off_pts[2] = {0, 0}, off_pns[2] = {0, 0}, m[2] = {0, 0}, k[2] = {0, 0};
    for (int s = 0; s < nsides; ++s) {
        m[s] = L[s].regs_s.size() + (extra_pt && extra_pt[s] ? 1 : 0);
        k[s] = L[s].pts_ns.size() / 64;
    }
    // both multi_exps as ONE set of launches over the concatenated pairs (msm_run's split mode): the second one's sort
    // and its latency chain no longer queue behind the first one's accumulation
    const bool split = nsides == 2 && c->dbg_eval_split && msm_split_ok(c, m[0] + m[1]);
    if (split) {
        off_idx[0] = off;  off_idx[1] = off + m[0] * 4;   off = stage_align(off + (m[0] + m[1]) * 4);
        off_pts[0] = off;  off_pts[1] = off + m[0] * 64;  off = stage_align(off + (m[0] + m[1]) * 64);
        for (int s = 0; s < 2; ++s) {
            off_pns[s] = off;
            off = stage_align(off + k[s] * 64);
        }
    } else {
        for (int s = 0; s < nsides; ++s) {
            off_idx[s] = off;  off = stage_align(off + m[s] * 4);
            off_pts[s] = off;  off = stage_align(off + m[s] * 64);
            off_pns[s] = off;  off = stage_align(off + k[s] * 64);
        }
    }
    const size_t total = off;
    TRY(ensure_pinned(c, c->h_stage, total, "staging block"));
    TRY(ensure(c, c->sch_in, total));
    if (need_tape) TRY(ensure(c, c->sch_regs, (size_t)nreg * REG_WORDS * 4 + 64));
    uint8_t* h = c->h_stage;
    if (need_tape) tape_fill(h, to, ct, t.consts.data(), nconst);
    for (int s = 0; s < nsides; ++s) {
        uint32_t* idx = (uint32_t*)(h + off_idx[s]);
        const size_t base_m = L[s].regs_s.size();
        for (size_t i = 0; i < base_m; ++i) idx[i] = t.resolve(L[s].regs_s[i]);
        memcpy(h + off_pts[s], L[s].pts_s.data(), base_m * 64);
        if (m[s] > base_m) {
            idx[base_m] = t.resolve((uint32_t)extra_reg[s]);
            memcpy(h + off_pts[s] + base_m * 64, extra_pt[s], 64);
        }
        if (k[s]) memcpy(h + off_pns[s], L[s].pts_ns.data(), k[s] * 64);
        TRY(ensure(c, c->sch_scalars[s], (split ? m[0] + m[1] : m[s]) * 32));
        TRY(ensure(c, c->sch_bases[s], (split ? m[0] + m[1] : m[s]) * 64));
    }
    hipStream_t st = c->stream;
    uint8_t* d = (uint8_t*)c->sch_in.p;
    HIP_TRY(c, hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, st));
    if (need_tape) {
        tape_launch(c, d, to, ct, nconst);
        c->sch_owner = sc;
        sc->tape_done_ops = nops;
        sc->tape_done_consts = nconst;
    }
    // the longer multi_exp first: its bucket reduction and Horner tail are the evaluation's critical path, the shorter
    // one's bulk and tail fit beside them (w_x holds one W commitment per rotation group, w_g every commitment)
    int order[2] = {0, 1};
    if (nsides == 2 && m[1] > m[0]) {
        order[0] = 1;
        order[1] = 0;
    }
    if (split) {
        const size_t mt = m[0] + m[1];
        // gather + Montgomery form + beta * x + GLV decomposition in one launch (the plan says whether the last two apply)
        MsmCall call{(const uint8_t*)c->sch_bases[0].p, (const uint8_t*)c->sch_scalars[0].p, mt, nullptr};
        call.split = (uint32_t)m[0];
        const bool glv = msm_route(c, call).p.glv;
        const unsigned g = (unsigned)((mt + BLOCK - 1) / BLOCK);
        if (glv) {
            TRY(ensure(c, c->sch_endo, mt * 32));
            hipLaunchKernelGGL(k_eval_prep<true>, dim3(g), dim3(BLOCK), 0, st, (const uint32_t*)c->sch_regs.p,
                               (const uint32_t*)(d + off_idx[0]), (const uint8_t*)(d + off_pts[0]), (uint32_t)mt,
                               (uint8_t*)c->sch_scalars[0].p, (uint8_t*)c->sch_bases[0].p, (uint8_t*)c->sch_endo.p, c->d_flags);
        } else {
            hipLaunchKernelGGL(k_eval_prep<false>, dim3(g), dim3(BLOCK), 0, st, (const uint32_t*)c->sch_regs.p,
                               (const uint32_t*)(d + off_idx[0]), (const uint8_t*)(d + off_pts[0]), (uint32_t)mt,
                               (uint8_t*)c->sch_scalars[0].p, (uint8_t*)c->sch_bases[0].p, (uint8_t*)nullptr, c->d_flags);
        }
        call.d_endo_x = glv ? (const uint8_t*)c->sch_endo.p : nullptr;
        TRY(msm_run(c, call));
        for (int s = 0; s < 2; ++s) {
            sc->side_xyzz[s] = c->d_res_xyzz + XYZZ_BYTES * s;
            sc->side_pns[s] = d + off_pns[s];
            sc->side_k[s] = k[s];
        }
    } else
    for (int os = 0; os < nsides; ++os) {
        const int s = order[os];
        hipLaunchKernelGGL(k_tape_gather, dim3((unsigned)((m[s] + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st,
                           (const uint32_t*)c->sch_regs.p, (const uint32_t*)(d + off_idx[s]), (uint32_t)m[s],
                           (uint8_t*)c->sch_scalars[s].p);
        hipLaunchKernelGGL(k_bases_to_mont, dim3(grid_for(c, m[s])), dim3(BLOCK), 0, st,
                           (const uint8_t*)(d + off_pts[s]), m[s], (uint8_t*)c->sch_bases[s].p, c->d_flags);
        TRY(msm_run(c, MsmCall{(const uint8_t*)c->sch_bases[s].p, (const uint8_t*)c->sch_scalars[s].p, m[s], nullptr}));
        sc->side_xyzz[s] = c->d_res_xyzz;   // this MSM's slot
        sc->side_pns[s] = d + off_pns[s];
        sc->side_k[s] = k[s];
    }
    S.point_list_len = L[nsides - 1].regs_s.size();           // ctx.point_list after the LAST multi_exp in the reference's order  mock/arith/ecc.rs:112-116
    return H2AGG_OK;
}
// part 2: add the scalar-less points (evaluation.rs:198-200); canonical Jacobian to d_out_jac (device).
// The caller has joined the tail streams.
int eval_finish(h2agg_schema* sc, int side, uint8_t* d_out_jac) {
    h2agg_ctx* c = sc->ctx;
    hipLaunchKernelGGL(k_eval_tail, dim3(1), dim3(BLOCK), 0, c->stream, sc->side_xyzz[side], sc->side_pns[side],
                       sc->side_k[side], d_out_jac, c->d_flags);
    return H2AGG_OK;
}
int eval_device(h2agg_schema* sc, EvalLists& L) {
    h2agg_ctx* c = sc->ctx;
    TRY(clear_flags(c));
    TRY(eval_launch_sides(sc, &L, 1, nullptr, nullptr));
    TRY(join_tails(c));
    return eval_finish(sc, 0, c->d_res_jac);
}

int fetch_reg_canonical(h2agg_schema* sc, uint32_t reg, uint8_t out[32]) {
    h2agg_ctx* c = sc->ctx;
    if (c->sch_owner != sc) return fail(c, H2AGG_ERR_INVALID, "register file belongs to another schema");
    TRY(ensure(c, c->sch_in, 256));
    TRY(ensure(c, c->sch_scalars[0], 32));
    memcpy(c->h_pinned + 1536, &reg, 4);
    HIP_TRY(c, hipMemcpyAsync(c->sch_in.p, c->h_pinned + 1536, 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_tape_gather, dim3(1), dim3(BLOCK), 0, c->stream, (const uint32_t*)c->sch_regs.p,
                       (const uint32_t*)c->sch_in.p, 1u, (uint8_t*)c->sch_scalars[0].p);
    HIP_TRY(c, hipMemcpyAsync(c->h_pinned + 1024, c->sch_scalars[0].p, 32, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    memcpy(out, c->h_pinned + 1024, 32);
    return H2AGG_OK;
}

}  // namespace

extern "C" {

int h2agg_schema_create(h2agg_ctx* c, h2agg_schema** out) try {
    TRY(bind(c));
    if (!out) return fail(c, H2AGG_ERR_INVALID, "null out");
    h2agg_schema* sc = new h2agg_schema();
    sc->ctx = c;
    *out = sc;
    return H2AGG_OK;
} API_CATCH
void h2agg_schema_destroy(h2agg_schema* sc) {
    if (!sc) return;
    if (sc->ctx->sch_owner == sc) sc->ctx->sch_owner = nullptr;   // device scratch belongs to the context
    delete sc;
}
int h2agg_schema_node_commitment(h2agg_schema* sc, const char* key, const uint8_t point_aff[64], uint32_t* node) try {
    if (!sc || !key || !point_aff || !node) return H2AGG_ERR_INVALID;
    *node = sc->s.add_commitment(key, point_aff);
    return H2AGG_OK;
} API_CATCH
int h2agg_schema_node_eval(h2agg_schema* sc, const uint8_t eval[32], uint32_t* node) try {
    if (!sc || !eval || !node) return H2AGG_ERR_INVALID;
    *node = sc->s.add_leaf_scalar(SchemaNode::EVAL, eval);
    return H2AGG_OK;
} API_CATCH
int h2agg_schema_node_scalar(h2agg_schema* sc, const uint8_t scalar[32], uint32_t* node) try {
    if (!sc || !scalar || !node) return H2AGG_ERR_INVALID;
    *node = sc->s.add_leaf_scalar(SchemaNode::SCALAR, scalar);
    return H2AGG_OK;
} API_CATCH
int h2agg_schema_node_add(h2agg_schema* sc, uint32_t l, uint32_t r, uint32_t* node) try {
    if (!sc || !node) return H2AGG_ERR_INVALID;
    if (!sc->s.valid(l) || !sc->s.valid(r)) return fail(sc->ctx, H2AGG_ERR_INVALID, "unknown schema node");
    *node = sc->s.add_binary(SchemaNode::ADD, l, r);
    return H2AGG_OK;
} API_CATCH
int h2agg_schema_node_mul(h2agg_schema* sc, uint32_t l, uint32_t r, uint32_t* node) try {
    if (!sc || !node) return H2AGG_ERR_INVALID;
    if (!sc->s.valid(l) || !sc->s.valid(r)) return fail(sc->ctx, H2AGG_ERR_INVALID, "unknown schema node");
    *node = sc->s.add_binary(SchemaNode::MUL, l, r);
    return H2AGG_OK;
} API_CATCH
int h2agg_schema_evaluation_queries(h2agg_schema* sc, size_t n, const char* const* keys, const uint8_t* commitments,
                                    const uint8_t* evals, uint32_t* nodes_out) try {
    if (!sc) return H2AGG_ERR_INVALID;
    if (n && (!keys || !commitments || !evals || !nodes_out)) return fail(sc->ctx, H2AGG_ERR_INVALID, "null buffer");
    sc->s.grow_nodes(3 * n);
    for (size_t i = 0; i < n; ++i) {
        if (!keys[i]) return fail(sc->ctx, H2AGG_ERR_INVALID, "null key");
        nodes_out[i] = sc->s.add_evaluation_query(keys[i], commitments + 64 * i, evals + 32 * i);
    }
    return H2AGG_OK;
} API_CATCH
int h2agg_schema_query_set_commitment(h2agg_schema* sc, uint32_t query_node, const uint8_t point_aff[64]) try {
    if (!sc || !point_aff) return H2AGG_ERR_INVALID;
    Schema& S = sc->s;
    if (!S.valid(query_node) || S.nodes[query_node].kind != SchemaNode::ADD ||
        S.nodes[S.nodes[query_node].l].kind != SchemaNode::COMMITMENT)
        return fail(sc->ctx, H2AGG_ERR_INVALID, "not an EvaluationQuery node ([C] + eval)");
    memcpy(S.points.data() + 64 * (size_t)S.nodes[S.nodes[query_node].l].point, point_aff, 64);
    return H2AGG_OK;
} API_CATCH
int h2agg_schema_batch_multi_open(h2agg_schema* sc, const char* key, size_t nq, const int32_t* rotations,
                                  const uint8_t* points, const uint32_t* query_nodes, size_t nw, const uint8_t* w,
                                  const uint8_t v[32], const uint8_t u[32], uint32_t* w_x_out, uint32_t* w_g_out) try {
    if (!sc) return H2AGG_ERR_INVALID;
    if (!key || !rotations || !points || !query_nodes || !w || !v || !u || !w_x_out || !w_g_out || nq == 0)
        return fail(sc->ctx, H2AGG_ERR_INVALID, "null buffer or no queries");
    if (!sc->s.batch_multi_open(key, nq, rotations, points, query_nodes, nw, w, v, u, *w_x_out, *w_g_out))
        return fail(sc->ctx, H2AGG_ERR_INVALID, sc->s.err);
    return H2AGG_OK;
} API_CATCH
int h2agg_schema_shplonk_multi_open(h2agg_schema* sc, const char* key, size_t nq, const uint32_t* poly_ids, const int32_t* rotations,
                                    const uint8_t* points, const uint32_t* query_nodes, const uint8_t h1[64], const uint8_t h2[64],
                                    const uint8_t y[32], const uint8_t v[32], const uint8_t u[32], uint32_t* left_out,
                                    uint32_t* right_out) try {
    if (!sc) return H2AGG_ERR_INVALID;
    if (!key || !poly_ids || !rotations || !points || !query_nodes || !h1 || !h2 || !y || !v || !u || !left_out || !right_out || nq == 0)
        return fail(sc->ctx, H2AGG_ERR_INVALID, "null buffer or no queries");
    if (!shplonk_multi_open(sc->s, key, nq, poly_ids, rotations, points, query_nodes, h1, h2, y, v, u, *left_out, *right_out))
        return fail(sc->ctx, H2AGG_ERR_INVALID, sc->s.err);
    return H2AGG_OK;
} API_CATCH
int h2agg_schema_estimate(h2agg_schema* sc, uint32_t node, size_t* out) try {
    if (!sc || !out) return H2AGG_ERR_INVALID;
    if (!sc->s.valid(node)) return fail(sc->ctx, H2AGG_ERR_INVALID, "unknown schema node");
    *out = sc->s.estimate(node, false);
    return H2AGG_OK;
} API_CATCH

int h2agg_schema_eval(h2agg_schema* sc, uint32_t node, uint8_t out_jac[96], int* has_scalar, uint8_t out_scalar[32]) try {
    if (!sc) return H2AGG_ERR_INVALID;
    h2agg_ctx* c = sc->ctx;
    TRY(bind(c));
    if (!out_jac || !has_scalar || !out_scalar) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    set_identity_jac(out_jac);
    *has_scalar = 0;
    memset(out_scalar, 0, 32);
    EvalLists L;
    TRY(eval_lists(sc, node, L));
    sc->s.names = L.names;
    TRY(eval_device(sc, L));
    TRY(fetch_result_jac(c, out_jac));
    if (L.e_reg >= 0) {
        *has_scalar = 1;
        TRY(fetch_reg_canonical(sc, sc->s.tape.resolve((uint32_t)L.e_reg), out_scalar));
    }
    return H2AGG_OK;
} API_CATCH

namespace {
// host half of evaluate_multiopen_proof (verify.rs:705-728): both eval_prepare walks recorded on the tape, and the
// (G, +/- e) pair each side folds into its multi_exp
int multiopen_lists(h2agg_schema* sc, uint32_t w_x, uint32_t w_g, EvalLists L[2], int64_t extra[2],
                    std::vector<uint32_t>& all_names) {
    h2agg_ctx* c = sc->ctx;
    Schema& S = sc->s;
    const uint32_t roots[2] = {w_x, w_g};
    extra[0] = extra[1] = -1;
    for (int side = 0; side < 2; ++side) {
        TRY(eval_lists(sc, roots[side], L[side]));
        all_names.insert(all_names.end(), L[side].names.begin(), L[side].names.end());
        // left = left_s + e*G ; right = right_s - e*G   (verify.rs:715-728): fold (G, +/- e) into the multi_exp
        if (L[side].e_reg >= 0) {
            if (side == 0) {
                extra[side] = L[side].e_reg;
            } else {
                uint8_t z[32] = {0};
                const uint32_t zero = S.tape.add_const(z);
                extra[side] = (int64_t)S.tape.record(TAPE_SUB, zero, (uint32_t)L[side].e_reg);   // 0 - e
            }
        }
        if (L[side].regs_s.empty())
            return fail(c, H2AGG_ERR_EMPTY, "multi_exp of zero pairs (reference panics: mock/arith/ecc.rs:128)");
    }
    return H2AGG_OK;
}

// (seg_msm.inc)
int seg_msm_run(h2agg_ctx* c, const uint8_t* d_bases, const uint8_t* d_scalars, const uint64_t* seg, size_t S,
                const uint32_t* d_seg, uint8_t* d_out_jac);

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
    CompiledTape ct;
    if (!compile_tape(t.resolved_ops(), nconst, c->dbg_tape_lds, ct)) return fail(c, H2AGG_ERR_INVALID, "tape: operand not yet defined");
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
    size_t off = 0;
    const TapeOffsets to = tape_layout(off, ct, nconst);
    const size_t off_idx = off;     off = stage_align(off + M * 4);
    const size_t off_pts = off;     off = stage_align(off + M * 64);
    const size_t off_pns = off;     off = stage_align(off + K * 64);
    const size_t off_seg = off;     off = stage_align(off + (nsides + 1) * 4);
    const size_t off_pseg = off;    off = stage_align(off + (nsides + 1) * 4);
    const size_t total = off;
    TRY(ensure_pinned(c, c->h_stage, total, "staging block"));
    TRY(ensure(c, c->sch_in, total));
    TRY(ensure(c, c->sch_regs, (size_t)nreg * REG_WORDS * 4 + 64));
    TRY(ensure(c, c->sch_scalars[0], M * 32 + 32));
    TRY(ensure(c, c->sch_bases[0], M * 64 + 64));
    TRY(ensure(c, c->seg_out, nsides * (96 + 128) + 256));
    uint8_t gen[64] = {0};
    gen[0] = 1;
    gen[32] = 2;   // pchip.assign_one = generator (1, 2)   verify.rs:714
    uint8_t* h = c->h_stage;
    tape_fill(h, to, ct, t.consts.data(), nconst);
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
    tape_launch(c, d, to, ct, nconst);
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
    if (!xyzz_to_affine(xyzz.data(), nsides, out_aff))
        return fail(c, H2AGG_ERR_HIP, "evaluate_multiopen_proof: the device returned a non-canonical coordinate");
    return H2AGG_OK;
}

}   // namespace

int h2agg_evaluate_multiopen_prepare(h2agg_schema* sc, uint32_t w_x, uint32_t w_g) try {
    if (!sc) return H2AGG_ERR_INVALID;
    h2agg_ctx* c = sc->ctx;
    Schema& S = sc->s;
    h2agg_schema::Prep& P = sc->prep;
    P = h2agg_schema::Prep();
    TRY(multiopen_lists(sc, w_x, w_g, P.L, P.extra, P.all_names));
    // the tape is final for this evaluation: its dependency levels (eval_launch_sides takes them as they are)
    if (!compile_tape(S.tape.resolved_ops(), S.tape.nconst, c->dbg_tape_lds, P.tape))
        return fail(c, H2AGG_ERR_INVALID, "tape: operand not yet defined");
    P.w_x = w_x;
    P.w_g = w_g;
    P.nodes_n = S.nodes.size();
    P.ops_n = S.tape.ops.size();
    P.consts_n = S.tape.nconst;
    P.valid = true;
    return H2AGG_OK;
} API_CATCH

int h2agg_evaluate_multiopen_proof(h2agg_schema* sc, uint32_t w_x, uint32_t w_g, uint8_t left_aff[64],
                                   uint8_t right_aff[64]) try {
    if (!sc) return H2AGG_ERR_INVALID;
    h2agg_ctx* c = sc->ctx;
    TRY(bind(c));
    if (!left_aff || !right_aff) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    memset(left_aff, 0, 64);
    memset(right_aff, 0, 64);
    Schema& S = sc->s;
    static const bool trace = getenv("H2AGG_TRACE") != nullptr;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto t_begin = now();
    auto lap = [&](const char* what) {
        if (!trace) return;
        auto t1 = now();
        fprintf(stderr, "[h2agg] evaluate_multiopen_proof %-12s %8.3f ms\n", what,
                std::chrono::duration<double, std::milli>(t1 - t_begin).count());
        t_begin = t1;
    };
    uint8_t gen[64] = {0};
    gen[0] = 1;
    gen[32] = 2;  // pchip.assign_one = generator (1, 2)   verify.rs:714
    // Record BOTH evaluations on the tape first (host), then run the tape once and do the two multi_exps.  A matching
    // h2agg_evaluate_multiopen_prepare has done that already; only the points are read again (they may have been
    // replaced since: h2agg_schema_query_set_commitment).
    h2agg_schema::Prep& P = sc->prep;
    const bool prepared = P.valid && P.w_x == w_x && P.w_g == w_g && P.nodes_n == S.nodes.size() &&
                          P.ops_n == S.tape.ops.size() && P.consts_n == S.tape.nconst;
    EvalLists L_own[2];
    int64_t extra_own[2] = {-1, -1};
    std::vector<uint32_t> names_own;
    EvalLists* L = prepared ? P.L : L_own;
    int64_t* extra = prepared ? P.extra : extra_own;
    std::vector<uint32_t>& all_names = prepared ? P.all_names : names_own;
    if (prepared) {
        for (int side = 0; side < 2; ++side) {
            for (size_t i = 0; i < L[side].pidx_s.size(); ++i)
                memcpy(L[side].pts_s.data() + 64 * i, S.points.data() + 64 * (size_t)L[side].pidx_s[i], 64);
            for (size_t i = 0; i < L[side].pidx_ns.size(); ++i)
                memcpy(L[side].pts_ns.data() + 64 * i, S.points.data() + 64 * (size_t)L[side].pidx_ns[i], 64);
        }
    } else {
        P.valid = false;
        TRY(multiopen_lists(sc, w_x, w_g, L, extra, all_names));
    }
    // both multi_exps are queued before either result is awaited: the second one's sort + accumulation run under
    // the first one's bucket reduction and Horner tail (tail slots)
    lap("eval_lists");
    TRY(clear_flags(c));
    const uint8_t* extra_pts[2] = {extra[0] >= 0 ? gen : nullptr, extra[1] >= 0 ? gen : nullptr};
    // the two multi_exps always overlap (the second one's sort + accumulation under the first one's bucket
    // reduction and Horner tail), whatever the context's setting for back-to-back standalone MSMs: both are
    // joined before this call returns
    {
        OverlapScope overlap(c);
        TRY(eval_launch_sides(sc, L, 2, extra_pts, extra, prepared ? &P : nullptr));
    }
    lap("launch");
    TRY(join_tails(c));
    // scalar-less points (evaluation.rs:198-200) + to_value (verify.rs:730-731), both sides in one launch
    // The device leaves both results as (X, Y, ZZ, ZZZ): xyzz_to_affine.
    hipLaunchKernelGGL(k_eval_tail_affine2, dim3(2), dim3(BLOCK), 0, c->stream, sc->side_xyzz[0], sc->side_xyzz[1],
                       sc->side_pns[0], sc->side_pns[1], sc->side_k[0], sc->side_k[1], (uint8_t*)nullptr, c->d_flags,
                       (uint8_t*)c->small.p + 512);
    HIP_TRY(c, hipMemcpyAsync(c->h_pinned + 512, (uint8_t*)c->small.p + 512, 256, hipMemcpyDeviceToHost, c->stream));
    TRY(finish(c));
    lap("device wait");
    uint8_t aff[128];
    if (!xyzz_to_affine(c->h_pinned + 512, 2, aff))
        return fail(c, H2AGG_ERR_HIP, "evaluate_multiopen_proof: the device returned a non-canonical coordinate");
    memcpy(left_aff, aff, 64);
    memcpy(right_aff, aff + 64, 64);
    S.names = all_names;  // points_wx ++ points_wg  (verify.rs:711-712)
    return H2AGG_OK;
} API_CATCH

// A straight-line Fr program on the device: the interpreter that EvaluationQuerySchema::eval records into, exposed for
// callers that have their own expressions (SURVEY.md 8(f)-1: the lookup / permutation / vanishing / lagrange expressions of
// params.rs etc. are exactly this shape).  Registers 0 .. nconst-1 are the inputs, register nconst + k is the result of
// op k; ops: 3 words {opcode (0 = mul, 1 = add, 2 = sub), a, b} with a, b < nconst + k.  Ops whose inputs are ready run
// in parallel (dependency levels); out_regs selects the registers to return (canonical, 32 B each).
int h2agg_fr_tape_eval(h2agg_ctx* c, const uint8_t* consts, size_t nconst, const uint32_t* ops3, size_t nops,
                       const uint32_t* out_regs, size_t nout, uint8_t* out) try {
    TRY(bind(c));
    if ((nconst && !consts) || (nops && !ops3) || (nout && (!out_regs || !out)))
        return fail(c, H2AGG_ERR_INVALID, "null buffer");
    if (nconst + nops >= ((size_t)1 << 30)) return fail(c, H2AGG_ERR_INVALID, "program too large");
    if (nout == 0) return H2AGG_OK;
    const uint32_t nreg = (uint32_t)(nconst + nops);
    std::vector<TapeOp> ops(nops);
    for (size_t k = 0; k < nops; ++k) {
        if (ops3[3 * k] > TAPE_INV) return fail(c, H2AGG_ERR_INVALID, "unknown tape opcode");
        ops[k] = TapeOp{(uint32_t)(nconst + k), ops3[3 * k + 1], ops3[3 * k + 2], ops3[3 * k]};
    }
    CompiledTape ct;
    if (!compile_tape(ops, (uint32_t)nconst, c->dbg_tape_lds, ct))
        return fail(c, H2AGG_ERR_INVALID, "tape: operand not defined before its use");
    for (size_t i = 0; i < nout; ++i)
        if (out_regs[i] >= nreg) return fail(c, H2AGG_ERR_INVALID, "tape: output register out of range");
    size_t off = 0;
    const TapeOffsets to = tape_layout(off, ct, (uint32_t)nconst);
    const size_t off_idx = off, total = stage_align(off + nout * 4);
    TRY(ensure_pinned(c, c->h_stage, total, "staging block"));
    TRY(ensure(c, c->sch_in, total));
    TRY(ensure(c, c->sch_regs, (size_t)nreg * REG_WORDS * 4 + 64));
    TRY(ensure(c, c->sch_scalars[0], nout * 32));
    c->sch_owner = nullptr;   // the register file no longer reflects any schema's tape
    uint8_t* h = c->h_stage;
    tape_fill(h, to, ct, consts, (uint32_t)nconst);
    memcpy(h + off_idx, out_regs, nout * 4);
    uint8_t* d = (uint8_t*)c->sch_in.p;
    hipStream_t st = c->stream;
    TRY(clear_flags(c));
    HIP_TRY(c, hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, st));
    tape_launch(c, d, to, ct, (uint32_t)nconst);
    hipLaunchKernelGGL(k_tape_gather, dim3((unsigned)((nout + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st,
                       (const uint32_t*)c->sch_regs.p, (const uint32_t*)(d + off_idx), (uint32_t)nout,
                       (uint8_t*)c->sch_scalars[0].p);
    HIP_TRY(c, hipMemcpyAsync(out, c->sch_scalars[0].p, nout * 32, hipMemcpyDeviceToHost, st));
    return finish(c);
} API_CATCH

size_t h2agg_schema_name_count(h2agg_schema* sc) { return sc ? sc->s.names.size() : 0; }
const char* h2agg_schema_name(h2agg_schema* sc, size_t i) {
    return (sc && i < sc->s.names.size()) ? sc->s.key_names[sc->s.names[i]].c_str() : "";
}
size_t h2agg_schema_names_joined(h2agg_schema* sc, char* out, size_t cap) {
    if (!sc) return 0;
    size_t need = 0;
    for (uint32_t id : sc->s.names) need += sc->s.key_names[id].size() + 1;
    if (!out || cap < need) return need;
    char* w = out;
    for (uint32_t id : sc->s.names) {
        const std::string& s = sc->s.key_names[id];
        memcpy(w, s.data(), s.size());
        w += s.size();
        *w++ = '\n';
    }
    return need;
}
size_t h2agg_schema_point_list_len(h2agg_schema* sc) { return sc ? sc->s.point_list_len : 0; }

}  // extern "C"
