// The Shplonk (BDFG20) verifier as schema nodes: the verifier half of include/h2agg.h's Shplonk section, beside the GWC fold
// Schema::batch_multi_open (csrc/schema.hpp).  Host code only: it records scalars on the schema's Fr tape and adds nodes; the
// tape's kernels and the evaluation are schema.hpp's and schema_api.inc's, unchanged.  (A file of its own because schema.hpp
// also holds the kernels between the tape and the multi_exp, whose sources the committed counter evidence is stamped with.)
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "schema.hpp"

namespace h2agg {

// queries: (polynomial id, rotation, evaluation point, schema node) in VerifierParams::queries order; a rotation names a
// point, the one its first query carries.  left = 1 * commit(H2), right = F + u H2 with
//   F = sum_i v^i c_i sum_j y^j sum_{a in S_i} l_{i,a}(u) node(p_{i,j}, a)  -  t H1
// (sum_a l_{i,a}(u) = 1: a node's commitment keeps v^i c_i y^j, its eval! parts add up to r_{i,j}(u), which
// evaluate_multiopen_proof subtracts as e G; the nodes stay opaque).  Every scalar is recorded on the schema's Fr tape.
constexpr size_t SCHEMA_SHPLONK_MAX_SET = 32;
struct SchemaShplonkSet {
    std::vector<uint32_t> points;   // indices into the rotation list, in the order the set's first polynomial names them
    std::vector<uint32_t> polys;    // indices into the first-seen polynomial list
};
// The ordering of the sets, in ONE place (halo2_proofs' construct_intermediate_sets is recalled, not pinned: a later pin
// changes this function only).  poly_points[m]: the rotation indices polynomial m (first-seen order) names, in first-seen
// order.  Polynomials with equal point sets form a set; sets in first-seen order of their first polynomial, polynomials
// inside a set in first-seen order of their first query.
inline std::vector<SchemaShplonkSet> schema_shplonk_sets(const std::vector<std::vector<uint32_t>>& poly_points) {
    std::vector<SchemaShplonkSet> sets;
    std::vector<std::vector<uint32_t>> sorted;   // each set's points, sorted: equality as SETS
    for (size_t m = 0; m < poly_points.size(); ++m) {
        std::vector<uint32_t> mine(poly_points[m]);
        std::sort(mine.begin(), mine.end());
        size_t s = 0;
        for (; s < sets.size(); ++s)
            if (sorted[s] == mine) break;
        if (s == sets.size()) {
            sets.push_back({poly_points[m], {}});
            sorted.push_back(mine);
        }
        sets[s].polys.push_back((uint32_t)m);
    }
    return sets;
}
inline bool shplonk_multi_open_regs(Schema& S, const char* key, size_t nq, const uint32_t* poly_ids, const int32_t* rotation,
                                    const uint32_t* point_regs, const uint32_t* qnodes, const uint8_t h1[64], const uint8_t h2[64],
                                    uint32_t y_reg, uint32_t v_reg, uint32_t u_reg, uint32_t& left_out, uint32_t& right_out);
inline bool shplonk_multi_open(Schema& S, const char* key, size_t nq, const uint32_t* poly_ids, const int32_t* rotation,
                               const uint8_t* points, const uint32_t* qnodes, const uint8_t h1[64], const uint8_t h2[64],
                               const uint8_t y[32], const uint8_t v[32], const uint8_t u[32], uint32_t& left_out, uint32_t& right_out) {
    std::vector<uint32_t> preg(nq);
    for (size_t i = 0; i < nq; ++i) preg[i] = S.tape.add_const(points + 32 * i);
    return shplonk_multi_open_regs(S, key, nq, poly_ids, rotation, preg.data(), qnodes, h1, h2, S.tape.add_const(y), S.tape.add_const(v),
                                   S.tape.add_const(u), left_out, right_out);
}
// the same with the evaluation points and y, v, u given as tape registers
inline bool shplonk_multi_open_regs(Schema& S, const char* key, size_t nq, const uint32_t* poly_ids, const int32_t* rotation,
                                    const uint32_t* point_regs, const uint32_t* qnodes, const uint8_t h1[64], const uint8_t h2[64],
                                    uint32_t y_reg, uint32_t v_reg, uint32_t u_reg, uint32_t& left_out, uint32_t& right_out) {
    if (nq == 0) {
        S.err = "no queries";
        return false;
    }
    // ---- rotations (= points) and polynomials in first-seen order; node_at[m][k]: the node of polynomial m at its k-th point
    std::vector<int32_t> rots;
    std::vector<uint32_t> z;   // the point register of every rotation
    std::vector<uint32_t> polys;
    std::vector<std::vector<uint32_t>> poly_points, node_at;
    for (size_t i = 0; i < nq; ++i) {
        if (!S.valid(qnodes[i])) {
            S.err = "unknown schema node";
            return false;
        }
        size_t a = 0, m = 0;
        for (; a < rots.size(); ++a)
            if (rots[a] == rotation[i]) break;
        if (a == rots.size()) {
            rots.push_back(rotation[i]);
            z.push_back(S.tape.materialize(point_regs[i]));
        }
        for (; m < polys.size(); ++m)
            if (polys[m] == poly_ids[i]) break;
        if (m == polys.size()) {
            polys.push_back(poly_ids[i]);
            poly_points.emplace_back();
            node_at.emplace_back();
        }
        for (uint32_t b : poly_points[m])
            if (b == a) {
                S.err = "a (polynomial, rotation) pair is named twice";
                return false;
            }
        poly_points[m].push_back((uint32_t)a);
        node_at[m].push_back(qnodes[i]);
    }
    const std::vector<SchemaShplonkSet> sets = schema_shplonk_sets(poly_points);
    for (const SchemaShplonkSet& s : sets)
        if (s.points.size() > SCHEMA_SHPLONK_MAX_SET) {
            S.err = "a set of more than 32 points";
            return false;
        }
    // ---- the scalars, on the tape
    auto mul = [&](uint32_t a, uint32_t b) { return S.tape.record(TAPE_MUL, a, b); };
    auto sub = [&](uint32_t a, uint32_t b) { return S.tape.record(TAPE_SUB, a, b); };
    auto inv = [&](uint32_t a) { return S.tape.record(TAPE_INV, a, a); };
    auto product = [&](std::vector<uint32_t> f) {   // a balanced tree; the empty product is one
        if (f.empty()) return S.one();
        while (f.size() > 1) {
            size_t o = 0;
            for (size_t i = 0; i + 1 < f.size(); i += 2) f[o++] = mul(f[i], f[i + 1]);
            if (f.size() & 1) f[o++] = f.back();
            f.resize(o);
        }
        return f[0];
    };
    const uint32_t u_r = S.tape.materialize(u_reg), v_r = S.tape.materialize(v_reg), y_r = S.tape.materialize(y_reg);
    const size_t nt = rots.size();
    std::vector<uint32_t> um(nt);   // u - z_b
    for (size_t b = 0; b < nt; ++b) um[b] = sub(u_r, z[b]);
    // two rotations with equal points invert zero: inside a set through its Lagrange denominators, the pairs no set
    // holds together through one inversion of their own.  NOTHING READS THAT INVERSE: it is recorded for its side effect,
    // FLAG_DIV_ZERO (tape_exec, schema.hpp), and stays on the tape because a compiled tape runs every recorded operation
    // — compile_tape (tape_compile.hpp) orders and places operations, it removes none; a value nobody reads only gets no
    // LDS slot.  A dead-code pass there would have to keep TAPE_INV.  Cost: one SUB per pair that no set holds together, their
    // product and one inversion on the level all inversions share (a circuit's rotations are few: 4 here, 6 pairs at most).
    {
        std::vector<uint8_t> together(nt * nt, 0);
        for (const SchemaShplonkSet& s : sets)
            for (uint32_t a : s.points)
                for (uint32_t b : s.points) together[a * nt + b] = 1;
        std::vector<uint32_t> apart;
        for (size_t a = 0; a < nt; ++a)
            for (size_t b = a + 1; b < nt; ++b)
                if (!together[a * nt + b]) apart.push_back(sub(z[a], z[b]));
        if (!apart.empty()) (void)inv(product(apart));
    }
    std::vector<uint32_t> c(sets.size());   // c_i = d_i / d_0, d_i = prod_{b in T \ S_i} (u - z_b)
    c[0] = S.one();
    if (sets.size() > 1) {
        std::vector<uint32_t> d(sets.size());
        for (size_t i = 0; i < sets.size(); ++i) {
            std::vector<uint8_t> in(nt, 0);
            for (uint32_t a : sets[i].points) in[a] = 1;
            std::vector<uint32_t> f;
            for (size_t b = 0; b < nt; ++b)
                if (!in[b]) f.push_back(um[b]);
            d[i] = product(f);
        }
        const uint32_t d0_inv = inv(d[0]);
        for (size_t i = 1; i < sets.size(); ++i) c[i] = mul(d[i], d0_inv);
    }
    std::vector<uint32_t> t_f;   // t = prod_{b in S_0} (u - z_b)  (= Z_T(u) / d_0)
    for (uint32_t a : sets[0].points) t_f.push_back(um[a]);
    const uint32_t t = product(t_f);
    size_t nterms = 0;
    for (const SchemaShplonkSet& s : sets) nterms += s.points.size() * s.polys.size();
    S.grow_nodes(3 * nterms + 16);
    bool have = false;
    uint32_t right = 0;
    auto add_term = [&](uint32_t scalar_reg, uint32_t node) {
        const uint32_t term = S.add_binary(SchemaNode::MUL, S.add_leaf_reg(SchemaNode::SCALAR, scalar_reg), node);
        right = have ? S.add_binary(SchemaNode::ADD, right, term) : term;
        have = true;
    };
    for (size_t i = 0; i < sets.size(); ++i) {
        const SchemaShplonkSet& s = sets[i];
        const size_t np = s.points.size();
        std::vector<uint32_t> l(np);   // l_{i,a}(u) = prod_{b != a} (u - z_b) / (z_a - z_b), 1 for a single point
        for (size_t a = 0; a < np; ++a) {
            if (np == 1) {
                l[a] = S.one();
                break;
            }
            std::vector<uint32_t> num, den;
            for (size_t b = 0; b < np; ++b)
                if (b != a) {
                    num.push_back(um[s.points[b]]);
                    den.push_back(sub(z[s.points[a]], z[s.points[b]]));
                }
            l[a] = mul(product(num), inv(product(den)));
        }
        const uint32_t w_i = i == 0 ? c[0] : mul(S.tape.pow(v_r, (uint32_t)i), c[i]);   // v^i c_i; powers ascend from 0
        for (size_t j = 0; j < s.polys.size(); ++j) {
            const uint32_t m = s.polys[j];
            const uint32_t w = j == 0 ? w_i : mul(w_i, S.tape.pow(y_r, (uint32_t)j));
            for (size_t a = 0; a < np; ++a) {
                size_t k = 0;   // where polynomial m names this point
                while (poly_points[m][k] != s.points[a]) ++k;
                add_term(np == 1 ? w : mul(w, l[a]), node_at[m][k]);
            }
        }
    }
    uint8_t zero32[32] = {0};
    const uint32_t h1_id = S.intern((std::string(key) + "_shplonk_h1").c_str()), h2_id = S.intern((std::string(key) + "_shplonk_h2").c_str());
    add_term(sub(S.tape.add_const(zero32), t), S.add_commitment_id(h1_id, h1));
    add_term(u_r, S.add_commitment_id(h2_id, h2));
    // (a bare commitment has no scalar, and multi_exp of zero pairs is the reference's panic, H2AGG_ERR_EMPTY: left = 1 * H2)
    left_out = S.add_binary(SchemaNode::MUL, S.add_leaf_reg(SchemaNode::SCALAR, S.one()), S.add_commitment_id(h2_id, h2));
    right_out = right;
    return true;
}

}  // namespace h2agg
