// TEST INFRASTRUCTURE ONLY — the field layer of csrc/fp.hpp and csrc/fp_asm.inc, one primitive per kernel, over raw limbs.
// Built by tests/fp_probe.py into tests/libfp_probe.so (never into libh2agg.so: the product keeps no test kernels); what is
// asserted about the results is in tests/field_ref.py.
//
//   int fp_probe_run(int field, int op, const uint32_t* host_in, uint32_t n, uint32_t* host_out)     -> the HIP error code
//
// field 0 = Fq, 1 = Fr; op = an index into fp_probe_op_name(); records as fp_probe_shape() reports them.
#include "fp_probe.hpp"
#include "fp.hpp"

using namespace h2agg;

namespace fp_probe {
namespace {

template <class P>
FP_INLINE Fp<P> ld(const uint32_t* p) {
    Fp<P> r;
#pragma unroll
    for (int i = 0; i < NL; ++i) r.l[i] = p[i];
    return r;
}
template <class P>
FP_INLINE void st(uint32_t* p, const Fp<P>& a) {
#pragma unroll
    for (int i = 0; i < NL; ++i) p[i] = a.l[i];
}
// no instructions: the limbs become opaque register values, so what is stored after an asm block is what the block left in them
template <class P>
FP_INLINE void fence(Fp<P>& a) {
#pragma unroll
    for (int i = 0; i < NL; ++i) asm volatile("" : "+v"(a.l[i]));
}

#define OP(NAME, NIN, NOUT, ...)                                                  \
    struct NAME {                                                                  \
        static constexpr int IN = (NIN), OUT = (NOUT);                             \
        static FP_INLINE void run(const uint32_t* in, uint32_t* out) { __VA_ARGS__ } \
    }
#define A ld<P>(in)
#define B ld<P>(in + 9)
#define C ld<P>(in + 18)
#define D ld<P>(in + 27)

// ---- linear
template <class P> OP(OpAdd, 18, 9, st(out, fp_add<P>(A, B)););
template <class P> OP(OpDbl, 9, 9, st(out, fp_dbl<P>(A)););
template <class P> OP(OpTriple, 9, 9, st(out, fp_triple<P>(A)););
template <class P> OP(OpNormalize, 9, 9, int32_t x[NL]; for (int i = 0; i < NL; ++i) x[i] = (int32_t)in[i]; st(out, fp_normalize<P>(x)););
template <class P> OP(OpCondSub, 9, 9, st(out, fp_cond_sub<P>(A)););
template <class P> OP(OpIsCanonical, 9, 1, out[0] = fp_is_canonical<P>(A) ? 1u : 0u;);
// ---- subtractions
template <int K, class P> OP(OpSub, 18, 9, st(out, fp_sub<K, P>(A, B)););
template <int K, class P> OP(OpNeg, 9, 9, st(out, fp_neg<K, P>(A)););
template <int K, class P> OP(OpSub2, 18, 9, st(out, fp_sub2<K, P>(A, B)););
template <int K, class P> OP(OpSubSub2, 27, 9, st(out, fp_sub_sub2<K, P>(A, B, C)););
template <int KP, int KN, class P> OP(OpSubSgn, 19, 9, st(out, fp_sub_sgn<KP, KN, P>(A, in[18], B)););   // (a, b, sgn)
template <int K, class P> OP(OpSubLoose, 18, 9, st(out, fp_sub_loose<K, P>(A, B)););
template <int K, class P> OP(OpNegLoose, 9, 9, st(out, fp_neg_loose<K, P>(A)););
// ---- products
template <class P> OP(OpMulPs, 18, 9, st(out, fp_mul_ps<P>(A, B)););
template <class P> OP(OpMulOs, 18, 9, st(out, fp_mul_os<P>(A, B)););
template <class P> OP(OpSqrPs, 9, 9, st(out, fp_sqr_ps<P>(A)););
template <class P> OP(OpSqrOs, 9, 9, st(out, fp_sqr_os<P>(A)););
template <class P> OP(OpMul2Ps, 36, 9, st(out, fp_mul2_ps<P>(A, B, C, D)););
template <class P> OP(OpMul2Os, 36, 9, st(out, fp_mul2_os<P>(A, B, C, D)););
template <class P> OP(OpMul3Ps, 54, 9, st(out, fp_mul3_ps<P>(A, B, C, D, ld<P>(in + 36), ld<P>(in + 45))););
template <class P> OP(OpMulDual, 36, 18, Fp<P> r0, r1; fp_mul_dual<P>(A, B, C, D, r0, r1); st(out, r0); st(out + 9, r1););
template <class P> OP(OpSqrDual, 18, 18, Fp<P> r0, r1; fp_sqr_dual<P>(A, B, r0, r1); st(out, r0); st(out + 9, r1););
template <class P>
OP(OpMul2MulMul, 72, 27, Fp<P> r0, r1, r2;
   fp_mul2_mul_mul<P>(A, B, C, D, ld<P>(in + 36), ld<P>(in + 45), ld<P>(in + 54), ld<P>(in + 63), r0, r1, r2);
   st(out, r0); st(out + 9, r1); st(out + 18, r2););
// the blocks of fp_asm.inc: every operand is stored back, so an in-place block that touched another operand shows
template <class P> OP(OpaMulIp, 18, 18, Fp<P> a = A, b = B; fence(a); fence(b); fpa_mul_ip<P>(a, b); fence(b); st(out, a); st(out + 9, b););
template <class P> OP(OpaMul, 18, 27, Fp<P> a = A, b = B, r; fence(a); fence(b); fpa_mul<P>(r, a, b); fence(a); fence(b); st(out, r); st(out + 9, a); st(out + 18, b););
template <class P> OP(OpaSqr, 9, 18, Fp<P> a = A, r; fence(a); fpa_sqr<P>(r, a); fence(a); st(out, r); st(out + 9, a););
template <class P>
OP(OpaMul2Ip1, 36, 36, Fp<P> a = A, b = B, c = C, d = D; fence(a); fence(b); fence(c); fence(d); fpa_mul2_ip1<P>(a, b, c, d);
   fence(b); fence(c); fence(d); st(out, a); st(out + 9, b); st(out + 18, c); st(out + 27, d););
template <class P>
OP(OpaMul2Ip, 36, 36, Fp<P> a = A, b = B, c = C, d = D; fence(a); fence(b); fence(c); fence(d); fpa_mul2_ip<P>(a, b, c, d);
   fence(b); fence(c); fence(d); st(out, a); st(out + 9, b); st(out + 18, c); st(out + 27, d););
template <class P>
OP(OpaMulDualIp, 36, 36, Fp<P> a = A, b = B, c = C, d = D; fence(a); fence(b); fence(c); fence(d); fpa_mul_dual_ip<P>(a, b, c, d);
   fence(b); fence(d); st(out, a); st(out + 9, b); st(out + 18, c); st(out + 27, d););
template <class P>
OP(OpaSqrDual, 18, 36, Fp<P> a = A, c = B, r0, r1; fence(a); fence(c); fpa_sqr_dual<P>(r0, r1, a, c); fence(a); fence(c);
   st(out, r0); st(out + 9, r1); st(out + 18, a); st(out + 27, c););
// the tail of the lean insertion as it stands in csrc/msm_kernels.hpp: (Y1, PPP, r, Q, X3) -> the real fp_neg_loose / fp_sub_loose
// -> the two-product block.  out: Y3 || ny || d (the loose operands as the block received them)
template <int KNY, bool TWO, class P>
OP(OpLooseTail, 45, 27, Fp<P> y1 = A, ppp = B, r = C, q = D, x3 = ld<P>(in + 36);
   Fp<P> d = fp_sub_loose<10, P>(q, x3); Fp<P> ny = fp_neg_loose<KNY, P>(y1); const Fp<P> ny0 = ny;
   if (TWO) fpa_mul2_ip<P>(ny, ppp, r, d); else fpa_mul2_ip1<P>(ny, ppp, r, d);
   st(out, ny); st(out + 9, ny0); st(out + 18, d););
// ---- reduction and tests
template <class P> OP(OpCanonical, 9, 9, st(out, fp_canonical<P>(A)););
template <class P> OP(OpToMont, 9, 9, st(out, fp_to_mont<P>(A)););
template <class P> OP(OpFromMont, 9, 9, st(out, fp_from_mont<P>(A)););
template <int K, class P> OP(OpMaybeZero, 9, 1, out[0] = fp_maybe_zero_mod<K, P>(A) ? 1u : 0u;);
template <int K, class P> OP(OpMaybeZero2, 9, 1, out[0] = fp_maybe_zero_mod2<K, P>(A) ? 1u : 0u;);
template <int K, class P> OP(OpIsZero, 9, 1, out[0] = fp_is_zero_mod<K, P>(A) ? 1u : 0u;);
template <class P> OP(OpUnpack, 8, 9, uint32_t w[8]; for (int i = 0; i < 8; ++i) w[i] = in[i]; st(out, fp_unpack<P>(w)););
template <class P> OP(OpPack, 9, 8, uint32_t w[8]; fp_pack<P>(w, A); for (int i = 0; i < 8; ++i) out[i] = w[i];);
// ---- inversion
template <class P> OP(OpInvInt, 9, 9, st(out, fp_inv_int<P>(A)););
template <class P> OP(OpInv, 9, 9, st(out, fp_inv<P>(A)););

#undef A
#undef B
#undef C
#undef D

#define E(NAME, FIELD, ...) {NAME, FIELD, __VA_ARGS__::IN, __VA_ARGS__::OUT, &launch<__VA_ARGS__, false>}
#define BOTH(NAME, T) E(NAME, 0, T<FqParams>), E(NAME, 1, T<FrParams>)
#define FQ(NAME, ...) E(NAME, 0, __VA_ARGS__)
#define FR(NAME, ...) E(NAME, 1, __VA_ARGS__)

// Fq / Fr as the product instantiates the primitive (grep the callers); the _os forms, the A/B variants of the products, follow
// their _ps twins.
const Entry TABLE[] = {
    BOTH("fp_add", OpAdd), FQ("fp_dbl", OpDbl<FqParams>), FQ("fp_triple", OpTriple<FqParams>), BOTH("fp_normalize", OpNormalize),
    BOTH("fp_cond_sub", OpCondSub), BOTH("fp_is_canonical", OpIsCanonical),
    FQ("fp_sub<2>", OpSub<2, FqParams>), FQ("fp_sub<4>", OpSub<4, FqParams>), FQ("fp_sub<6>", OpSub<6, FqParams>),
    FQ("fp_sub<8>", OpSub<8, FqParams>),
    FR("fp_sub<1>", OpSub<1, FrParams>), FR("fp_sub<2>", OpSub<2, FrParams>), FR("fp_sub<3>", OpSub<3, FrParams>),
    FQ("fp_neg<2>", OpNeg<2, FqParams>), FQ("fp_neg<4>", OpNeg<4, FqParams>), FR("fp_neg<2>", OpNeg<2, FrParams>),
    FQ("fp_sub2<4>", OpSub2<4, FqParams>), FQ("fp_sub_sub2<6>", OpSubSub2<6, FqParams>),
    FQ("fp_sub_sgn<4,6>", OpSubSgn<4, 6, FqParams>), FQ("fp_sub_sgn<2,4>", OpSubSgn<2, 4, FqParams>),
    FQ("fp_sub_loose<10>", OpSubLoose<10, FqParams>),
    FQ("fp_neg_loose<8>", OpNegLoose<8, FqParams>), FQ("fp_neg_loose<4>", OpNegLoose<4, FqParams>),
    BOTH("fp_mul_ps", OpMulPs), BOTH("fp_mul_os", OpMulOs), BOTH("fp_sqr_ps", OpSqrPs), BOTH("fp_sqr_os", OpSqrOs),
    FQ("fp_mul2_ps", OpMul2Ps<FqParams>), FQ("fp_mul2_os", OpMul2Os<FqParams>), BOTH("fp_mul3_ps", OpMul3Ps),
    FQ("fp_mul_dual", OpMulDual<FqParams>), FQ("fp_sqr_dual", OpSqrDual<FqParams>), FQ("fp_mul2_mul_mul", OpMul2MulMul<FqParams>),
    FQ("fpa_mul_ip", OpaMulIp<FqParams>), FQ("fpa_mul", OpaMul<FqParams>), FQ("fpa_sqr", OpaSqr<FqParams>),
    FQ("fpa_mul2_ip1", OpaMul2Ip1<FqParams>), FQ("fpa_mul_dual_ip", OpaMulDualIp<FqParams>), FQ("fpa_sqr_dual", OpaSqrDual<FqParams>),
    FQ("fpa_mul2_ip", OpaMul2Ip<FqParams>),
    FQ("loose_tail<8,ip>", OpLooseTail<8, true, FqParams>), FQ("loose_tail<8,ip1>", OpLooseTail<8, false, FqParams>),
    FQ("loose_tail<4,ip>", OpLooseTail<4, true, FqParams>), FQ("loose_tail<4,ip1>", OpLooseTail<4, false, FqParams>),
    BOTH("fp_canonical", OpCanonical), BOTH("fp_to_mont", OpToMont), BOTH("fp_from_mont", OpFromMont),
    FQ("fp_maybe_zero_mod<4>", OpMaybeZero<4, FqParams>), FQ("fp_maybe_zero_mod<6>", OpMaybeZero<6, FqParams>),
    FQ("fp_maybe_zero_mod<10>", OpMaybeZero<10, FqParams>),
    FQ("fp_maybe_zero_mod2<4>", OpMaybeZero2<4, FqParams>), FQ("fp_maybe_zero_mod2<6>", OpMaybeZero2<6, FqParams>),
    FQ("fp_maybe_zero_mod2<10>", OpMaybeZero2<10, FqParams>),
    FQ("fp_is_zero_mod<2>", OpIsZero<2, FqParams>), FQ("fp_is_zero_mod<4>", OpIsZero<4, FqParams>),
    FQ("fp_is_zero_mod<6>", OpIsZero<6, FqParams>), FQ("fp_is_zero_mod<8>", OpIsZero<8, FqParams>),
    FQ("fp_is_zero_mod<10>", OpIsZero<10, FqParams>), FR("fp_is_zero_mod<2>", OpIsZero<2, FrParams>),
    BOTH("fp_unpack", OpUnpack), BOTH("fp_pack", OpPack),
    BOTH("fp_inv_int", OpInvInt), BOTH("fp_inv", OpInv),
};
constexpr int NTABLE = (int)(sizeof(TABLE) / sizeof(TABLE[0]));

// op ids: the distinct names of both tables, in order of appearance
constexpr int MAX_OPS = 256;
const char* g_names[MAX_OPS];
int g_nnames = -1;
void names_init() {
    if (g_nnames >= 0) return;
    int n = 0, ng = 0;
    const Entry* g = group_table(&ng);
    for (int pass = 0; pass < 2; ++pass) {
        const Entry* t = pass ? g : TABLE;
        const int cnt = pass ? ng : NTABLE;
        for (int i = 0; i < cnt; ++i) {
            bool seen = false;
            for (int j = 0; j < n; ++j) seen = seen || strcmp(g_names[j], t[i].name) == 0;
            if (!seen && n < MAX_OPS) g_names[n++] = t[i].name;
        }
    }
    g_nnames = n;
}
const Entry* lookup(int field, int op) {
    names_init();
    if (op < 0 || op >= g_nnames) return nullptr;
    if (const Entry* e = find(TABLE, NTABLE, field, g_names[op])) return e;
    int ng = 0;
    const Entry* g = group_table(&ng);
    return find(g, ng, field, g_names[op]);
}

}  // namespace
}  // namespace fp_probe

extern "C" {
int fp_probe_op_count() {
    fp_probe::names_init();
    return fp_probe::g_nnames;
}
const char* fp_probe_op_name(int op) {
    fp_probe::names_init();
    return (op >= 0 && op < fp_probe::g_nnames) ? fp_probe::g_names[op] : nullptr;
}
// 0 and the record sizes (in 32-bit words) when (field, op) is instantiated, -1 otherwise
int fp_probe_shape(int field, int op, int* in_words, int* out_words) {
    const fp_probe::Entry* e = fp_probe::lookup(field, op);
    if (!e) return -1;
    *in_words = e->in_words;
    *out_words = e->out_words;
    return 0;
}
int fp_probe_run(int field, int op, const uint32_t* host_in, uint32_t n, uint32_t* host_out) {
    const fp_probe::Entry* e = fp_probe::lookup(field, op);
    if (!e) return (int)hipErrorInvalidValue;
    return (int)e->run(host_in, n, host_out);
}
}
