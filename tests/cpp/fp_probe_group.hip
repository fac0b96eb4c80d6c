// TEST INFRASTRUCTURE ONLY — second translation unit of the field-layer probe (see fp_probe.hip): the group-law formulas of
// csrc/g1.hpp, the lean insertion forms of csrc/msm_kernels.hpp and the limb-parallel code of csrc/lp_kernels.hpp, over raw
// XYZZ records (36 limbs: x || y || zz || zzz) and raw affine points (18 limbs: x || y).
#include "fp_probe.hpp"
#include "msm_kernels.hpp"
#include "lp_kernels.hpp"

using namespace h2agg;

namespace fp_probe {
namespace {

FP_INLINE Fq ld(const uint32_t* p) {
    Fq r;
#pragma unroll
    for (int i = 0; i < NL; ++i) r.l[i] = p[i];
    return r;
}
FP_INLINE void st(uint32_t* p, const Fq& a) {
#pragma unroll
    for (int i = 0; i < NL; ++i) p[i] = a.l[i];
}
FP_INLINE G1Affine lda(const uint32_t* p) {
    G1Affine r;
    r.x = ld(p);
    r.y = ld(p + 9);
    return r;
}
FP_INLINE G1XYZZ ldx(const uint32_t* p) {
    G1XYZZ r;
    r.x = ld(p);
    r.y = ld(p + 9);
    r.zz = ld(p + 18);
    r.zzz = ld(p + 27);
    return r;
}
FP_INLINE void stx(uint32_t* p, const G1XYZZ& a) {
    st(p, a.x);
    st(p + 9, a.y);
    st(p + 18, a.zz);
    st(p + 27, a.zzz);
}

#define OP(NAME, NIN, NOUT, ...)                                                  \
    struct NAME {                                                                  \
        static constexpr int IN = (NIN), OUT = (NOUT);                             \
        static FP_INLINE void run(const uint32_t* in, uint32_t* out) { __VA_ARGS__ } \
    }

OP(OpDouble, 36, 36, stx(out, xyzz_double(ldx(in))););
OP(OpDoubleAffine, 18, 36, stx(out, xyzz_double_affine(lda(in))););
OP(OpAddAffine, 54, 36, G1XYZZ acc = ldx(in); xyzz_add_affine(acc, lda(in + 36)); stx(out, acc););
OP(OpAddAffineAffine, 36, 36, stx(out, xyzz_add_affine_affine(lda(in), lda(in + 18))););
OP(OpAdd, 72, 36, stx(out, xyzz_add(ldx(in), ldx(in + 36))););
OP(OpAddChains, 72, 36, stx(out, xyzz_add_chains(ldx(in), ldx(in + 36))););
// (acc, q, sgn) -> acc || returned bool; the following entry's gather is empty
template <bool DUAL, int VAR>
OP(OpLeanAdd, 55, 37, G1XYZZ acc = ldx(in); const bool ok = xyzz_add_affine_lean<DUAL, VAR>(acc, lda(in + 36), in[54], [] {});
   stx(out, acc); out[36] = ok ? 1u : 0u;);
// (a, q, sgn) -> o || returned bool; o is only written when the form returns true (it starts as the identity record)
template <bool DUAL, int VAR>
OP(OpLeanAddAA, 37, 37, G1XYZZ o = G1XYZZ::identity(); const bool ok = xyzz_add_affine_affine_lean<DUAL, VAR>(o, lda(in), lda(in + 18), in[36]);
   stx(out, o); out[36] = ok ? 1u : 0u;);

// ---- limb-parallel: one case per wave, the case's limbs spread over every DPP row (limb j in lane j of each row, lanes 9..15
// zero) as tools/lp_test.hip does; out: the raw result limbs of all four rows (4 x 9), so the test sees that the rows agree
FP_INLINE uint32_t lp_in(const uint32_t* a, const LpConst& k) { return k.j < NL ? a[k.j < NL ? k.j : 0] : 0u; }
FP_INLINE void lp_out(uint32_t* out, uint32_t v, const LpConst& k) {
    if (k.j < NL) out[9 * k.row + k.j] = v;
}
OP(OpLpMul, 18, 36, const LpConst k = lp_const(); lp_out(out, lp_mul(lp_in(in, k), lp_in(in + 9, k), k), k););
template <int K> OP(OpLpSub, 18, 36, const LpConst k = lp_const(); lp_out(out, lp_sub<K>(lp_in(in, k), lp_in(in + 9, k), k), k););
template <int K> OP(OpLpNeg, 9, 36, const LpConst k = lp_const(); lp_out(out, lp_neg<K>(lp_in(in, k), k), k););
OP(OpLpTriple, 9, 36, const LpConst k = lp_const(); lp_out(out, lp_triple(lp_in(in, k), k), k););
// points: out = row 0's raw limbs of x || y || zz || zzz
FP_INLINE void lp_out_point(uint32_t* out, const LpPoint& p, const LpConst& k) {
    if (k.row == 0 && k.j < NL) {
        out[k.j] = p.x;
        out[9 + k.j] = p.y;
        out[18 + k.j] = p.zz;
        out[27 + k.j] = p.zzz;
    }
}
OP(OpLpDouble, 36, 36, const LpConst k = lp_const(); lp_out_point(out, lp_double(lp_load(in, k), k), k););
OP(OpLpAddPoints, 72, 36, __shared__ uint32_t sm[4 * 64]; const LpConst k = lp_const();
   lp_out_point(out, lp_add_points(lp_load(in, k), lp_load(in + 36, k), k, sm), k););

#define E(NAME, ...) {NAME, 0, __VA_ARGS__::IN, __VA_ARGS__::OUT, &launch<__VA_ARGS__, false>}
#define EW(NAME, ...) {NAME, 0, __VA_ARGS__::IN, __VA_ARGS__::OUT, &launch<__VA_ARGS__, true>}
#define LEAN(D, DN) \
    E("xyzz_add_affine_lean<" DN ",0>", OpLeanAdd<D, 0>), E("xyzz_add_affine_lean<" DN ",1>", OpLeanAdd<D, 1>),              \
    E("xyzz_add_affine_lean<" DN ",2>", OpLeanAdd<D, 2>), E("xyzz_add_affine_lean<" DN ",3>", OpLeanAdd<D, 3>),              \
    E("xyzz_add_affine_affine_lean<" DN ",0>", OpLeanAddAA<D, 0>), E("xyzz_add_affine_affine_lean<" DN ",1>", OpLeanAddAA<D, 1>), \
    E("xyzz_add_affine_affine_lean<" DN ",2>", OpLeanAddAA<D, 2>), E("xyzz_add_affine_affine_lean<" DN ",3>", OpLeanAddAA<D, 3>)

const Entry TABLE[] = {
    E("xyzz_double", OpDouble), E("xyzz_double_affine", OpDoubleAffine), E("xyzz_add_affine", OpAddAffine),
    E("xyzz_add_affine_affine", OpAddAffineAffine), E("xyzz_add", OpAdd), E("xyzz_add_chains", OpAddChains),
    LEAN(true, "1"), LEAN(false, "0"),
    EW("lp_mul", OpLpMul), EW("lp_sub<3>", OpLpSub<3>), EW("lp_sub<5>", OpLpSub<5>), EW("lp_sub<7>", OpLpSub<7>),
    EW("lp_sub<9>", OpLpSub<9>), EW("lp_sub<11>", OpLpSub<11>), EW("lp_neg<3>", OpLpNeg<3>), EW("lp_neg<5>", OpLpNeg<5>),
    EW("lp_triple", OpLpTriple), EW("lp_double", OpLpDouble), EW("lp_add_points", OpLpAddPoints),
};

}  // namespace

const Entry* group_table(int* count) {
    *count = (int)(sizeof(TABLE) / sizeof(TABLE[0]));
    return TABLE;
}

}  // namespace fp_probe
