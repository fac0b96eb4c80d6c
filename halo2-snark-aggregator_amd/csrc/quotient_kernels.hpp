// The quotient polynomial h(X) over Fr for gfx950: the device side of
//   h2agg_vk_expressions_eval   the expressions of a verifying key (gates, a lookup's input / table lists) on every row
//   h2agg_quotient              gates, permutation and lookup identities folded with y on the cosets of the extended domain;
//                               above 2^24 the pieces come from k_qe_cross_cosets (the coset-split ending, at the end of this file)
//   (halo2_proofs' evaluation of h(X) in create_proof: an unvendored git dependency of the reference, recalled — DESIGN.md
//    section 2; the yardstick is the definition in include/h2agg.h.  WHICH expressions, in which order, is pinned:
//    halo2-snark-aggregator-api/src/systems/halo2/params.rs:74-224, permutation.rs:54-136, lookup.rs:34-119, vanish.rs:18-72.)
// Columns are [columns][n] canonical 32-byte little-endian elements, n = 2^k; one thread per row, so consecutive threads read
// consecutive rows of every column, at every rotation (a rotation shifts the whole wave's window, it does not scatter it).
//
// k_qe_eval is an interpreter.  The host compiles a list of expressions (postfix bytecode of the key) into a program of
// three-word instructions — constants and challenges already in Montgomery form in a pool behind the code, leaves resolved
// to (slab, column, rotation mod n) — and every lane of a wave reads the same instruction (the words go through
// readfirstlane: control flow is scalar).  The operand stack: its top in registers, the values below it in LDS as
// [slot][limb][thread], so the 64 lanes of the one wave of a workgroup hit 64 different banks and no per-thread array is
// indexed dynamically (that would be scratch memory).  QE_DEPTH - 1 = 15 slots x 9 limbs x 64 threads x 4 B = 33.75 KiB.
// QE_END closes an expression: its value is stored to its own column, or folded into an accumulator in registers
// (acc = acc * fold + value: the first expression ends under the highest power), or — k_qe_eval<true> — only tested for zero.
//
// Number forms.  Everything on the stack is in Montgomery form.  A leaf costs one product (x * R^2 / R), the result one
// (value * 1 / R) and a conditional subtraction: stored values are canonical.  Bounds, in units of r: a leaf < 1.04 (a
// non-canonical input, < 5.3, raises FLAG_NONCANONICAL where `check` is set), a constant < 1, a product of two values <= 2 is
// < 1.03; a sum of two values <= 2 is <= 4 and goes through fr_fft_reduce2 (<= 2); a negation 2r - a is <= 2.  So every stack
// value is <= 2 whatever the expression, and the folded accumulator, (< 1.02) + (<= 2) reduced, as well.
// The fixed-form kernels (permutation, lookup) never add more than three values < 1.04 in front of a product, and every
// expression of theirs ends with a product by l_0, l_last or act = 1 - l_last - l_blind (< 4): a value < 1.1; their
// accumulator is < 1.02 + 1.1.
//
// Per-call scalars come BY VALUE in the kernel arguments, and what is too long for that — the program, the list of
// permutation columns — is written to device memory by k_qe_put, a kernel that carries the words in ITS arguments: the write
// is ordered on the stream like any launch, so a second queued call cannot rewrite what the first one's kernels have not
// read (fr_fft_kernels.hpp, prod_kernels.hpp).
#pragma once
#include "prod_kernels.hpp"

namespace h2agg {

constexpr unsigned QE_DEPTH = 16;        // operand stack: H2AGG_EXPR_MAX_DEPTH of include/h2agg.h
constexpr int QE_THREADS = 64;           // one wave per workgroup: the stack of a workgroup is 33.75 KiB of LDS
constexpr unsigned QE_PUT_WORDS = 896;   // words one k_qe_put launch carries (3.5 KiB of the 4 KiB of kernel arguments)
enum : uint32_t { QE_CONST = 0, QE_COLUMN = 1, QE_NEG = 2, QE_SUM = 3, QE_PRODUCT = 4, QE_SCALED = 5, QE_END = 6 };

struct QePutArgs {
    uint32_t w[QE_PUT_WORDS];
};

// dst[i] = w[i], i < count <= QE_PUT_WORDS
__global__ void __launch_bounds__(BLOCK) k_qe_put(const QePutArgs a, uint32_t* __restrict__ dst, uint32_t count) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < count && i < QE_PUT_WORDS) dst[i] = a.w[i];
}

struct QeArgs {
    uint32_t fold[8];         // folded: fold R mod r (Montgomery), canonical
    const uint32_t* prog;     // ninstr x {op | slab << 8, a, b}
    const uint32_t* consts;   // the pool: 8 words per constant, Montgomery, canonical
    const uint8_t* advice;    // slab 0, 1, 2: [columns][n]
    const uint8_t* fixed;
    const uint8_t* instance;
    const uint8_t* acc_in;    // folded: the column the fold continues from (plain, ours); null: from 0
    uint8_t* out;             // folded: [n]; otherwise [expressions][n]
    uint32_t* flags;
    uint32_t ninstr, n;
    uint32_t folded;
    uint32_t check;           // the slabs are the caller's: elements are checked for < r
    uint32_t* zflags;         // k_qe_eval<true>: [expressions][zwords], bit (i & 31) of word i >> 5 is row i (witness_kernels.hpp)
    uint32_t zwords;          //   2 ceil(n / 64): every wave owns the two words of its 64 rows
    uint32_t u;               //   rows from u up are never flagged
};

FP_INLINE uint32_t qe_slot(uint32_t slot, uint32_t limb, uint32_t tid) { return (slot * NL + limb) * QE_THREADS + tid; }

// One flag bit per row: the wave that holds the rows [i0, i0 + 64), i0 = i & ~63, stores their bits as the two words
// 2 (i0 >> 6) and 2 (i0 >> 6) + 1 of `line` — both < 2 ceil(n / 64) because row i0 < n.  Every thread of a workgroup of a
// multiple of 64 threads with i = blockIdx.x * blockDim.x + threadIdx.x < n calls it from converged code: lane 0 of a wave
// with a row below n is such a thread (i0 <= i), and a lane that has left (i >= n) votes 0.  No atomics: a word has one writer.
FP_INLINE void qe_put_flag(bool fails, uint32_t* __restrict__ line, uint32_t i) {
    const uint64_t m = __ballot(fails);
    if ((threadIdx.x & 63u) == 0u) {
        line[2u * (i >> 6)] = (uint32_t)m;
        line[2u * (i >> 6) + 1u] = (uint32_t)(m >> 32);
    }
}

// Program invariants (qe_compile, quotient.inc): every QE_COLUMN has a column inside its slab and b < n; every constant
// index is inside the pool; an operator finds its operands; at most QE_DEPTH values are live, so `cnt - 1 <= QE_DEPTH - 1`
// values sit in LDS, slots 0 .. QE_DEPTH - 2; QE_END finds exactly one value.  Rows: i < n, (i + b) & (n - 1) < n.
// FLAGS (the witness check's ending, witness_kernels.hpp): QE_END stores no value; it reduces the top of the stack (any
// representative of 0 below 2r — 0, r, 2r — becomes the integer 0) and sets bit i of line e of zflags where the value is not
// zero and i < u.  Line e < the program's expressions = the lines the host sized zflags for.  Nothing is written to `out`.
template <bool FLAGS>
__global__ void __launch_bounds__(QE_THREADS) k_qe_eval(const QeArgs a) {
    __shared__ uint32_t st[(QE_DEPTH - 1) * NL * QE_THREADS];
    const uint32_t tid = threadIdx.x;
    const uint32_t i = blockIdx.x * QE_THREADS + tid;
    if (i >= a.n) return;
    const uint32_t mask = a.n - 1u;
    const Fr foldM = fp_unpack<FrParams>(a.fold);
    Fr acc = Fr::zero(), tos = Fr::zero();
    if (a.folded && a.acc_in) acc = fp_to_mont<FrParams>(fp_load<FrParams>(a.acc_in + 32 * (size_t)i));
    uint32_t cnt = 0;   // live values: the top in `tos`, value j < cnt - 1 in slot j
    uint32_t e = 0;     // expressions closed so far
#pragma unroll 1
    for (uint32_t pc = 0; pc < a.ninstr; ++pc) {
        const uint32_t w0 = __builtin_amdgcn_readfirstlane(a.prog[3 * pc]);
        const uint32_t wa = __builtin_amdgcn_readfirstlane(a.prog[3 * pc + 1]);
        const uint32_t wb = __builtin_amdgcn_readfirstlane(a.prog[3 * pc + 2]);
        const uint32_t op = w0 & 0xffu;
        if (op == QE_CONST || op == QE_COLUMN) {
            if (cnt && cnt <= QE_DEPTH - 1u) {
#pragma unroll
                for (int l = 0; l < NL; ++l) st[qe_slot(cnt - 1u, l, tid)] = tos.l[l];
            }
            ++cnt;
            if (op == QE_CONST) {
                tos = fp_load<FrParams>(a.consts + 8 * (size_t)wa);
            } else {
                const uint32_t s = w0 >> 8;
                const uint8_t* slab = s == 0 ? a.advice : s == 1 ? a.fixed : a.instance;
                const Fr x = fp_load<FrParams>(slab + 32 * ((size_t)wa * a.n + ((i + wb) & mask)));
                if (a.check && !fp_is_canonical<FrParams>(x)) atomicOr(a.flags, FLAG_NONCANONICAL);
                tos = fp_to_mont<FrParams>(x);
            }
        } else if (op == QE_SUM || op == QE_PRODUCT) {
            Fr x;
            const uint32_t slot = cnt >= 2u && cnt <= QE_DEPTH ? cnt - 2u : 0u;
#pragma unroll
            for (int l = 0; l < NL; ++l) x.l[l] = st[qe_slot(slot, l, tid)];
            --cnt;
            tos = op == QE_SUM ? fr_fft_reduce2(fp_add<FrParams>(x, tos)) : fp_mul<FrParams>(x, tos);
        } else if (op == QE_NEG) {
            tos = fp_neg<2, FrParams>(tos);
        } else if (op == QE_SCALED) {
            tos = fp_mul<FrParams>(tos, fp_load<FrParams>(a.consts + 8 * (size_t)wa));
        } else {   // QE_END
            if constexpr (FLAGS) qe_put_flag(i < a.u && !fp_from_mont<FrParams>(tos).is_zero_int(), a.zflags + (size_t)e * a.zwords, i);
            else if (a.folded) acc = fr_fft_reduce2(fp_add<FrParams>(fp_mul<FrParams>(acc, foldM), tos));
            else fp_store<FrParams>(a.out + 32 * ((size_t)e * a.n + i), fp_from_mont<FrParams>(tos));
            ++e;
            cnt = 0;
        }
    }
    if (!FLAGS && a.folded) fp_store<FrParams>(a.out + 32 * (size_t)i, fp_from_mont<FrParams>(acc));
}

// The rows of l_0, l_last and l_blind in Lagrange form: dst[0][i] = (i == 0), dst[1][i] = (i == u), dst[2][i] = (i > u); i < n
__global__ void __launch_bounds__(BLOCK) k_qe_lagrange_rows(uint8_t* __restrict__ dst, uint32_t n, uint32_t u) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    Fr one = Fr::zero();
    one.l[0] = 1u;
    fp_store<FrParams>(dst + 32 * (size_t)i, i == 0 ? one : Fr::zero());
    fp_store<FrParams>(dst + 32 * ((size_t)n + i), i == u ? one : Fr::zero());
    fp_store<FrParams>(dst + 32 * (2 * (size_t)n + i), i > u ? one : Fr::zero());
}

// One coset's values (plain canonical: the transforms' output) and where the fixed-form kernels find their columns.  They
// live in two bases: `cos`, the slab [polys][n] the call transformed for this coset, and `key`, the slab that holds the
// key's own columns — sigma, l_0 / l_last / l_blind, and the fixed columns — on this coset.  A call without a proving key
// transforms everything into one slab and passes key = cos; with the coset form of a proving key (pk.inc) `key` is that
// object's slab [F + P + 3][n] of the coset, which no launch of the call writes.  A column place names its base: bit
// QE_IN_KEY set reads `key`, the low bits are the column there.  Every index below is < the columns of its base (qt_layout,
// quotient.inc).
constexpr uint32_t QE_IN_KEY = 1u << 31;
struct QeCoset {
    const uint8_t* cos;
    const uint8_t* key;
    const uint8_t* acc_in;   // the y-fold so far (plain, [n]); null: 0
    uint8_t* acc_out;        // may be acc_in: a thread reads its own row before it writes it
    uint32_t yM[8];          // y R
    uint32_t n;
    uint32_t l0;             // in `key`: l_0, then l_last, then l_blind
};

FP_INLINE Fr qe_col(const uint8_t* cos, uint32_t col, uint32_t n, uint32_t row) {
    return fp_to_mont<FrParams>(fp_load<FrParams>(cos + 32 * ((size_t)col * n + row)));
}
FP_INLINE Fr qe_fold(const Fr& acc, const Fr& yM, const Fr& ev) { return fp_add<FrParams>(fp_mul<FrParams>(acc, yM), ev); }

struct QePermArgs {
    QeCoset q;
    uint32_t betaR2[8];     // beta R^2: times a plain sigma gives beta sigma R
    uint32_t gammaM[8];     // gamma R
    uint32_t deltaM[8];     // delta R
    uint32_t bsM[8];        // beta s R: times w^i R gives beta X R on the coset of s
    const uint32_t* cols;   // [P]: the place of permutation column g (QE_IN_KEY: a fixed column that lives in `key`)
    const uint8_t* w_lo;    // Montgomery w^i, i < 2^wT (fr_fft_table's pair, 2^k entries in all)
    const uint8_t* w_hi;
    uint32_t wT;
    uint32_t P, chunk, n_sets;   // n_sets = ceil(P / chunk) >= 1
    uint32_t sigma0, z0;         // sigma_g at sigma0 + g of `key`, z_s at z0 + s of `cos`
    uint32_t rot_last;           // n - (blinding_factors + 1)
};

// The permutation argument's expressions on one coset, folded behind acc_in (permutation.rs:54-136): l_0 (1 - z_0),
// l_last (z_last^2 - z_last), l_0 (z_s - z_{s-1}(w^last X)) for s >= 1, and per set
// act (z_s(wX) prod (v_g + beta sigma_g + gamma) - z_s(X) prod (v_g + delta^g beta X + gamma)).  Rows (i + rot) & (n - 1) < n;
// g < P; table index i < n = 2^k.
__global__ void __launch_bounds__(BLOCK) k_qe_permutation(const QePermArgs a) {
    const uint32_t n = a.q.n, i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t mask = n - 1u;
    const uint8_t* cos = a.q.cos;
    const uint8_t* key = a.q.key;
    const Fr yM = fp_unpack<FrParams>(a.q.yM), one = Fr::one();
    const Fr l0 = qe_col(key, a.q.l0, n, i), ll = qe_col(key, a.q.l0 + 1u, n, i), lb = qe_col(key, a.q.l0 + 2u, n, i);
    const Fr act = fp_sub<3, FrParams>(one, fp_add<FrParams>(ll, lb));   // < 4
    Fr acc = a.q.acc_in ? fp_to_mont<FrParams>(fp_load<FrParams>(a.q.acc_in + 32 * (size_t)i)) : Fr::zero();
    {
        const Fr z = qe_col(cos, a.z0, n, i);
        acc = qe_fold(acc, yM, fp_mul<FrParams>(l0, fp_sub<2, FrParams>(one, z)));
        const Fr zl = qe_col(cos, a.z0 + a.n_sets - 1u, n, i);
        acc = qe_fold(acc, yM, fp_mul<FrParams>(ll, fp_sub<2, FrParams>(fp_mul<FrParams>(zl, zl), zl)));
    }
#pragma unroll 1
    for (uint32_t s = 1; s < a.n_sets; ++s) {
        const Fr z = qe_col(cos, a.z0 + s, n, i), zp = qe_col(cos, a.z0 + s - 1u, n, (i + a.rot_last) & mask);
        acc = qe_fold(acc, yM, fp_mul<FrParams>(l0, fp_sub<2, FrParams>(z, zp)));
    }
    const Fr betaR2 = fp_unpack<FrParams>(a.betaR2), gammaM = fp_unpack<FrParams>(a.gammaM), deltaM = fp_unpack<FrParams>(a.deltaM);
    const Fr wi = i ? fr_fft_table(a.w_lo, a.w_hi, a.wT, i) : one;   // w^i R, < 2
    Fr d = fp_mul<FrParams>(fp_unpack<FrParams>(a.bsM), wi);         // delta^g beta X R, g = 0
#pragma unroll 1
    for (uint32_t s = 0; s < a.n_sets; ++s) {
        Fr left = qe_col(cos, a.z0 + s, n, (i + 1u) & mask), right = qe_col(cos, a.z0 + s, n, i);
        const uint32_t g1 = (s + 1u) * a.chunk < a.P ? (s + 1u) * a.chunk : a.P;
#pragma unroll 1
        for (uint32_t g = s * a.chunk; g < g1; ++g) {
            const uint32_t place = a.cols[g];
            const Fr t = fp_add<FrParams>(qe_col(place & QE_IN_KEY ? key : cos, place & ~QE_IN_KEY, n, i), gammaM);
            const Fr sg = fp_mul<FrParams>(fp_load<FrParams>(key + 32 * ((size_t)(a.sigma0 + g) * n + i)), betaR2);
            left = fp_mul<FrParams>(left, fp_add<FrParams>(t, sg));
            right = fp_mul<FrParams>(right, fp_add<FrParams>(t, d));
            d = fp_mul<FrParams>(d, deltaM);
        }
        acc = qe_fold(acc, yM, fp_mul<FrParams>(act, fp_sub<2, FrParams>(left, right)));
    }
    fp_store<FrParams>(a.q.acc_out + 32 * (size_t)i, fp_from_mont<FrParams>(acc));
}

struct QeLookupArgs {
    QeCoset q;
    uint32_t betaM[8], gammaM[8];   // beta R, gamma R
    const uint8_t* in;              // the theta-folds of the lookup's input and table expressions on this coset (plain, [n])
    const uint8_t* table;
    uint32_t z, ap, sp;             // columns of `cos`
};

// One lookup's five expressions on one coset, folded behind acc_in (lookup.rs:34-119): l_0 (1 - z), l_last (z^2 - z),
// act (z(wX)(a' + beta)(s' + gamma) - z(X)(A + beta)(S + gamma)), l_0 (a' - s'), act (a' - s')(a' - a'(w^-1 X)).
__global__ void __launch_bounds__(BLOCK) k_qe_lookup(const QeLookupArgs a) {
    const uint32_t n = a.q.n, i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t mask = n - 1u;
    const uint8_t* cos = a.q.cos;
    const uint8_t* key = a.q.key;
    const Fr yM = fp_unpack<FrParams>(a.q.yM), one = Fr::one();
    const Fr l0 = qe_col(key, a.q.l0, n, i), ll = qe_col(key, a.q.l0 + 1u, n, i), lb = qe_col(key, a.q.l0 + 2u, n, i);
    const Fr act = fp_sub<3, FrParams>(one, fp_add<FrParams>(ll, lb));   // < 4
    Fr acc = a.q.acc_in ? fp_to_mont<FrParams>(fp_load<FrParams>(a.q.acc_in + 32 * (size_t)i)) : Fr::zero();
    const Fr betaM = fp_unpack<FrParams>(a.betaM), gammaM = fp_unpack<FrParams>(a.gammaM);
    const Fr z = qe_col(cos, a.z, n, i), zn = qe_col(cos, a.z, n, (i + 1u) & mask);
    const Fr ap = qe_col(cos, a.ap, n, i), apm = qe_col(cos, a.ap, n, (i + mask) & mask), sp = qe_col(cos, a.sp, n, i);
    acc = qe_fold(acc, yM, fp_mul<FrParams>(l0, fp_sub<2, FrParams>(one, z)));
    acc = qe_fold(acc, yM, fp_mul<FrParams>(ll, fp_sub<2, FrParams>(fp_mul<FrParams>(z, z), z)));
    {
        const Fr A = fp_to_mont<FrParams>(fp_load<FrParams>(a.in + 32 * (size_t)i));
        const Fr S = fp_to_mont<FrParams>(fp_load<FrParams>(a.table + 32 * (size_t)i));
        const Fr left = fp_mul<FrParams>(fp_mul<FrParams>(zn, fp_add<FrParams>(ap, betaM)), fp_add<FrParams>(sp, gammaM));
        const Fr right = fp_mul<FrParams>(fp_mul<FrParams>(z, fp_add<FrParams>(A, betaM)), fp_add<FrParams>(S, gammaM));
        acc = qe_fold(acc, yM, fp_mul<FrParams>(act, fp_sub<2, FrParams>(left, right)));
    }
    const Fr diff = fp_sub<2, FrParams>(ap, sp);   // < 4
    acc = qe_fold(acc, yM, fp_mul<FrParams>(l0, diff));
    acc = qe_fold(acc, yM, fp_mul<FrParams>(act, fp_mul<FrParams>(diff, fp_sub<2, FrParams>(ap, apm))));
    fp_store<FrParams>(a.q.acc_out + 32 * (size_t)i, fp_from_mont<FrParams>(acc));
}

// ext[(i << e) | coset] = acc[i] / (s^n - 1): row i of coset c' is the point zeta w_ext^(i 2^e + c').  (i << e) | coset < 2^(k + e).
struct QeScalar {
    uint32_t w[8];
};
__global__ void __launch_bounds__(BLOCK) k_qe_store_extended(const uint8_t* __restrict__ acc, const QeScalar invM /* R / (s^n - 1) */,
                                                             uint32_t n, uint32_t e, uint32_t coset, uint8_t* __restrict__ ext) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n || coset >= (1u << e)) return;
    const Fr v = fp_mul<FrParams>(fp_load<FrParams>(acc + 32 * (size_t)i), fp_unpack<FrParams>(invM.w));   // plain, < 1.01
    fp_store<FrParams>(ext + 32 * ((((size_t)i) << e) | coset), fp_cond_sub<FrParams>(v));
}

// The coset-split ending (quotient.inc, qt_queue): u[cosets][n] holds, per coset c', the size-n inverse transform at shift
// s = zeta w_ext^c' of that coset's fold column (plain canonical: the transform's output), NOT yet divided by s^n - 1.  The
// pieces are a small transform across the coset index, row by row:
//   h[i][l] = sum_c' u[c'][l] * T[i][c'],   T[i][c'] = zeta^(-n i) w_E^(-c' i) / (2^e (s_c'^n - 1)),   i < pieces <= cosets
// (the per-coset division is linear, so it rides in the constants).  tab[i][c'] is T[i][c'] R, canonical, eight words, written
// by k_qe_put.  One thread per row l and per group of LIVE pieces (blockIdx.y): a coset row is read along l by consecutive
// threads, the constant's address is the same for a whole workgroup, and the LIVE accumulators are a register file walked by
// fully unrolled loops (LIVE is a template parameter: a run-time count would turn them into an indexed array in scratch).
// The host launches k_qe_cross_cosets<QX_PIECES> over the full groups and one more instantiation over the rest.
// Bounds, in units of r: u < 1 times a constant < 1 is < 1.01 and plain; an accumulator < 2 plus that is < 4 and goes through
// fr_fft_reduce2 (< 2); fp_cond_sub makes the stored value canonical.
// Indices: l < n; c' < cosets; i0 + g < first + groups * LIVE <= pieces (the host's two launches), so the tab index is
// < pieces * cosets and the h row < pieces.
constexpr int QX_PIECES = 4;   // (eight accumulators: the compiler keeps the array in scratch; four stay in registers)
struct QeCrossArgs {
    const uint8_t* u;      // [cosets][n]
    const uint32_t* tab;   // [pieces][cosets][8]
    uint8_t* h;            // [pieces][n]
    uint32_t n, cosets, pieces;
    uint32_t first;        // the launch's first piece: workgroup row y holds pieces first + y LIVE .. first + y LIVE + LIVE - 1
};
template <int LIVE>
__global__ void __launch_bounds__(BLOCK) k_qe_cross_cosets(const QeCrossArgs a) {
    static_assert(LIVE >= 1 && LIVE <= QX_PIECES, "one instantiation per size of a group");
    const uint32_t l = blockIdx.x * BLOCK + threadIdx.x, i0 = a.first + blockIdx.y * LIVE;
    if (l >= a.n || i0 + LIVE > a.pieces) return;
    Fr acc[LIVE];
#pragma unroll
    for (int g = 0; g < LIVE; ++g) acc[g] = Fr::zero();
#pragma unroll 1
    for (uint32_t cs = 0; cs < a.cosets; ++cs) {
        const Fr x = fp_load<FrParams>(a.u + 32 * ((size_t)cs * a.n + l));
#pragma unroll
        for (int g = 0; g < LIVE; ++g) {
            const Fr t = fp_load<FrParams>(a.tab + 8 * ((size_t)(i0 + g) * a.cosets + cs));
            acc[g] = fr_fft_reduce2(fp_add<FrParams>(acc[g], fp_mul<FrParams>(x, t)));
        }
    }
#pragma unroll
    for (int g = 0; g < LIVE; ++g) fp_store<FrParams>(a.h + 32 * ((size_t)(i0 + g) * a.n + l), fp_cond_sub<FrParams>(acc[g]));
}

}  // namespace h2agg
