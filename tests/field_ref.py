"""TEST INFRASTRUCTURE ONLY — the reference for the field-layer probe (tests/fp_probe.py), in plain Python integers.

For every op of the probe this module holds
  * cases(field)          the inputs: (family, flat list of 32-bit words) pairs, every one asserted to meet the op's REQUIRES
                          before it leaves here (a red test then means the kernel, not the input);
  * check(field, w, out)  None, or what is wrong with the output record `out` for the input record `w`;
  * model(field, w)       an output record that satisfies check — what tests/test_field_ref_host.py mutates to show that the
                          checks can fail.

The value of a limb vector is sum(l[i] << 29*i), loose or tight, and every check is exact: an equation between integers, the
Montgomery identity r*R = T + q*m with 0 <= q < R, or the group law of oracle/bn254.py on the affine points the records stand for.
Congruence mod m alone would hide a lost carry that happens to be a multiple of m.
"""
from __future__ import annotations

import itertools
import os
import sys

from oracle import bn254 as O

NL = 9
M29 = (1 << 29) - 1
RBITS = 29 * NL
R = 1 << RBITS
FQ, FR = 0, 1
MOD = {FQ: O.P, FR: O.R}
NRANDOM = 4096
MAXCROSS = 10000


# --------------------------------------------------------------------------------------------------------- limbs and values
def val(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def tight(v):
    """the carry-normalised limbs of v (limbs 0..7 < 2^29, the top limb takes the rest)"""
    assert 0 <= v < (1 << (29 * 8 + 32)), v
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> (29 * 8)]


def is_tight(l):
    return all(0 <= x <= M29 for x in l[:8]) and 0 <= l[8] < (1 << 32)


def hexl(l):
    return "[" + " ".join("%08x" % x for x in l) + "]"


def km_borrowed(m, k):
    """csrc/fp.hpp km_limb_borrowed"""
    t = tight(k * m)
    return [t[i] + ((1 << 29) if i < 8 else 0) - (1 if i > 0 else 0) for i in range(NL)]


def lp_borrowed(k):
    """csrc/lp_kernels.hpp lp_const(): limb 0 + 2^29, limbs 1..7 + 2^29 - 1, limb 8 - 1"""
    t = tight(k * O.P)
    return [t[0] + (1 << 29)] + [t[i] + (1 << 29) - 1 for i in range(1, 8)] + [t[8] - 1]


def mont(m, T):
    """the r of r*R = T + q*m with 0 <= q < R: what a Montgomery reduction of the integer T returns"""
    q = (-T * pow(m, -1, R)) % R
    assert (T + q * m) % R == 0
    return (T + q * m) // R


def check_mont(m, T, r):
    """the Montgomery identity: r*R - T = q*m with 0 <= q < R (so r < T/R + m, the bound csrc/fp.hpp promises)"""
    d = r * R - T
    if d % m:
        return "r*R - T is not a multiple of m"
    if not 0 <= d // m < R:
        return "the quotient (r*R - T)/m = %#x is outside [0, 2^261)" % (d // m)
    return None


def need_tight(l, what="result"):
    return None if is_tight(l) else "%s limbs are not tight: %s" % (what, hexl(l))


# --------------------------------------------------------------------------------------------------------- operand families
def rng_value(rng, lim):
    """uniform-ish value < lim from 5 words of the generator"""
    v = 0
    for _ in range(5):
        v = (v << 64) | rng.next()
    return v % lim


def structured(m, B, inclusive=False, seed=1):
    """The edge values of an operand of bound B: (family, value) with value < B*m (<= B*m when inclusive)."""
    lim = B * m + (1 if inclusive else 0)
    low = (1 << 232) - 1
    out = []
    if lim - 1 >= low:
        out.append((ALL_ONES, low + (((lim - 1 - low) >> 232) << 232)))
    out += [("0", 0), ("1", 1), ("m-1", m - 1), ("m", m), ("m+1", m + 1), ("B*m-1", B * m - 1)]
    if inclusive:
        out.append(("B*m", B * m))
    out.append(("low limbs 0, largest top limb", ((lim - 1) >> 232) << 232))
    for i in range(NL):
        out.append(("limb %d all ones, rest 0" % i, M29 << (29 * i)))
    alt0 = sum(M29 << (29 * i) for i in range(0, 8, 2))
    alt1 = sum(M29 << (29 * i) for i in range(1, 8, 2))
    for nm, a in (("alternating ones / 0", alt0), ("alternating 0 / ones", alt1)):
        out.append((nm, a))
        if lim - 1 >= a:
            out.append((nm + ", largest top limb", a + (((lim - 1 - a) >> 232) << 232)))
    out.append(("R mod m", R % m))
    out.append(("R^2 mod m", R * R % m))
    rng = O.SplitMix64(0x66705f70726f6265 + seed)
    for x in (rng_value(rng, m), m - 2):
        for k in range(B):
            out.append(("x + %d*m" % k, x + k * m))
    seen, res = set(), []
    for fam, v in out:
        if 0 <= v < lim and v not in seen:
            seen.add(v)
            res.append((fam, v))
    return res


ALL_ONES = "limbs 0..7 all ones, largest top limb"
DIAGONAL = (ALL_ONES, "B*m-1", "B*m", "m-1", "low limbs 0, largest top limb", "alternating ones / 0", "alternating 0 / ones",
            "alternating ones / 0, largest top limb", "alternating 0 / ones, largest top limb", "R mod m")


def share(n):
    """the random cases of one of n sub-sets of an op, so that the op gets NRANDOM in all"""
    return -(-NRANDOM // n)


def operand_sets(m, bounds, seed, joint=None, nrandom=NRANDOM, maxcross=MAXCROSS):
    """Cases for operands with the given bounds: bounds[i] = (B, inclusive).  The cross product of the structured values where it
    stays under maxcross (an op with several bound sets shares MAXCROSS among them); otherwise the diagonal (one edge family in
    every operand), a one-at-a-time sweep and a seeded sample of it.  Then nrandom random in-contract tuples.  joint(values) -> bool
    filters tuples by a REQUIRES that ties operands together.  -> [(family, [values])]"""
    rng = O.SplitMix64(seed)
    lists = [structured(m, B, inc, seed=i) for i, (B, inc) in enumerate(bounds)]
    total = 1
    for l in lists:
        total *= len(l)
    res = []
    if total <= maxcross:
        combos = itertools.product(*lists)
    else:
        combos = []
        # the diagonal: the same edge family in every operand at once — all limbs of all operands at their maxima is what
        # fills the 64-bit columns of a multi-product block
        for fam in DIAGONAL:
            picks = [[e for e in l if e[0] == fam] for l in lists]
            if all(picks):
                combos.append(tuple(p[0] for p in picks))
        # every structured value of every operand at least once, against the others' all-ones vector and their last value
        ones = [next((e for e in l if e[0] == ALL_ONES), l[-1]) for l in lists]
        for i, l in enumerate(lists):
            for e in l:
                for anchor in (ones, [x[-1] for x in lists]):
                    c = list(anchor)
                    c[i] = e
                    combos.append(tuple(c))
        for _ in range(min(1000, maxcross)):
            combos.append(tuple(l[rng.next() % len(l)] for l in lists))
    for c in combos:
        vs = [v for _, v in c]
        if joint is None or joint(vs):
            res.append((" | ".join(f for f, _ in c), vs))
    n = 0
    while n < nrandom:
        vs = [rng_value(rng, B * m + (1 if inc else 0)) for B, inc in bounds]
        if joint is None or joint(vs):
            res.append(("random", vs))
            n += 1
    return res


def words_of(values):
    w = []
    for v in values:
        w += tight(v)
    return w


def ops_of(w, n):
    return [list(w[9 * i:9 * i + 9]) for i in range(n)]


# --------------------------------------------------------------------------------------------------------- the specs
class Spec:
    """cases(field) -> [(family, words)], check(field, words, out) -> None | message, model(field, words) -> out"""

    def __init__(self, cases, check, model):
        self.cases, self.check, self.model = cases, check, model


SPECS = {}


def exact_spec(nops, bounds, expr, seed, requires, joint=None, extra_words=None, limb_max=None):
    """An op whose result is the integer expr(m, values[, flag]) in tight limbs (or, with limb_max(m), in loose limbs under the
    stated per-limb maxima).  bounds: one list of per-operand (B, inclusive) per bound set.  extra_words: flag words to cross with.
    requires(m, values, flag) -> bool: the op's REQUIRES as csrc/fp.hpp states it, asserted on every case; joint: the part of it
    that ties operands together, as the filter of the generator."""

    def cases(field):
        m = MOD[field]
        res = []
        for bi, bs in enumerate(bounds):
            for flag in (extra_words or [None]):
                j = (lambda vs, flag=flag: joint(m, vs, flag)) if joint else None
                for fam, vs in operand_sets(m, bs, seed + 97 * bi + (flag or 0) % 7, joint=j, nrandom=share(len(bounds) * len(extra_words or [0])),
                                                maxcross=MAXCROSS // (len(bounds) * len(extra_words or [0]))):
                    assert requires(m, vs, flag), (fam, vs, flag)
                    assert 0 <= expr(m, vs, flag) < R if flag is not None else 0 <= expr(m, vs) < R     # the result fits the limbs
                    w = words_of(vs) + ([flag] if flag is not None else [])
                    res.append(("bounds %r%s: %s" % ([b for b, _ in bs], "" if flag is None else " flag %#x" % flag, fam), w))
        return res

    def expected(field, w):
        m = MOD[field]
        vs = [val(o) for o in ops_of(w, nops)]
        flag = w[9 * nops] if len(w) > 9 * nops else None
        return expr(m, vs, flag) if flag is not None else expr(m, vs)

    def check(field, w, out):
        m = MOD[field]
        want = expected(field, w)
        if limb_max is None:
            e = need_tight(out)
            if e:
                return e
        else:
            mx = limb_max(m)
            for i in range(NL):
                if not 0 <= out[i] <= mx[i]:
                    return "limb %d = %#x is above its stated maximum %#x" % (i, out[i], mx[i])
        if val(out) != want:
            return "value %#x, want the integer %#x (difference %#x)" % (val(out), want, val(out) - want)
        return None

    def model(field, w):
        want = expected(field, w)
        if limb_max is None:
            return tight(want)
        # the loose forms: limb by limb, as the comment in csrc/fp.hpp states them
        return None

    return Spec(cases, check, model)


def _b(*bs):
    return [(b, False) for b in bs]


def _bi(*bs):
    return [(b, True) for b in bs]


# ---- linear
SPECS["fp_add"] = exact_spec(2, [_b(1, 1), _b(2, 2), _b(8, 4), _b(84, 84)], lambda m, v: v[0] + v[1], 0x1001, lambda m, v, f: v[0] + v[1] < R)
SPECS["fp_dbl"] = exact_spec(1, [_b(1), _b(2), _b(4), _b(84)], lambda m, v: 2 * v[0], 0x1002, lambda m, v, f: 2 * v[0] < R)
SPECS["fp_triple"] = exact_spec(1, [_b(1), _b(2), _b(56)], lambda m, v: 3 * v[0], 0x1003, lambda m, v, f: 3 * v[0] < R)


def _cond_sub(m, v):
    return v[0] - m if v[0] >= m else v[0]


SPECS["fp_cond_sub"] = exact_spec(1, [_b(2)], _cond_sub, 0x1004, lambda m, v, f: v[0] < 2 * m)
# subtractions: K and the bound of the minuend at the call sites (and the largest that keeps the value under 2^261)
for K, AS in ((1, (1, 2)), (2, (2, 4)), (3, (2,)), (4, (2, 8)), (6, (2,)), (8, (2, 160))):
    SPECS["fp_sub<%d>" % K] = exact_spec(2, [[(A, False), (K, True)] for A in AS], lambda m, v, K=K: v[0] - v[1] + K * m, 0x2000 + K,
                                       lambda m, v, f, K=K: v[1] <= K * m)
for K in (2, 4):
    SPECS["fp_neg<%d>" % K] = exact_spec(1, [_bi(K)], lambda m, v, K=K: K * m - v[0], 0x2100 + K, lambda m, v, f, K=K: v[0] <= K * m)
SPECS["fp_sub2<4>"] = exact_spec(2, [[(2, False), (2, True)], [(160, False), (2, True)]], lambda m, v: v[0] - 2 * v[1] + 4 * m, 0x2200,
                                 lambda m, v, f: 2 * v[1] <= 4 * m)
SPECS["fp_sub_sub2<6>"] = exact_spec(
    3, [[(2, False), (2, True), (2, True)], [(2, False), (6, True), (3, True)]], lambda m, v: v[0] - v[1] - 2 * v[2] + 6 * m, 0x2300,
    lambda m, v, f: v[1] + 2 * v[2] <= 6 * m, joint=lambda m, v, f: v[1] + 2 * v[2] <= 6 * m)
SGN = 0xFFFFFFFF
for KP, KN, bs in ((4, 6, [[(2, False), (4, True)], [(6, True), (4, True)]]), (2, 4, [[(2, True), (2, True)], [(4, True), (2, True)]])):
    SPECS["fp_sub_sgn<%d,%d>" % (KP, KN)] = exact_spec(
        2, bs, lambda m, v, f, KP=KP, KN=KN: (v[0] - v[1] + KP * m) if f == 0 else (KN * m - v[0] - v[1]), 0x2400 + KP,
        lambda m, v, f, KP=KP, KN=KN: f in (0, SGN) and (v[1] <= KP * m if f == 0 else v[0] + v[1] <= KN * m),
        joint=lambda m, v, f, KP=KP, KN=KN: v[1] <= KP * m if f == 0 else v[0] + v[1] <= KN * m, extra_words=[0, SGN])


def _loose_sub_max(K):
    return lambda m: [x + (M29 if i < 8 else (1 << 29)) for i, x in enumerate(km_borrowed(m, K))]


SPECS["fp_sub_loose<10>"] = exact_spec(2, [[(2, False), (9, True)]], lambda m, v: v[0] - v[1] + 10 * m, 0x2500,
                                       lambda m, v, f: v[1] <= 9 * m,      # b tight with value <= (K - 1)*m
                                       limb_max=lambda m: [min(x, (1 << 29) + (1 << 30) - 1) if i < 8 else x for i, x in enumerate(_loose_sub_max(10)(m))])
for K in (8, 4):
    SPECS["fp_neg_loose<%d>" % K] = exact_spec(1, [_bi(K - 1)], lambda m, v, K=K: K * m - v[0], 0x2600 + K, lambda m, v, f, K=K: v[0] <= (K - 1) * m,
                                               limb_max=lambda m, K=K: [min(x, (1 << 30) - 1) if i < 8 else x for i, x in enumerate(km_borrowed(m, K))])


def _loose_model(name, K, sub):
    def model(field, w):
        b = km_borrowed(MOD[field], K)
        o = ops_of(w, 2 if sub else 1)
        return [o[0][i] + b[i] - o[1][i] for i in range(NL)] if sub else [b[i] - o[0][i] for i in range(NL)]
    SPECS[name].model = model


_loose_model("fp_sub_loose<10>", 10, True)
_loose_model("fp_neg_loose<8>", 8, False)
_loose_model("fp_neg_loose<4>", 4, False)


# ---- fp_normalize: signed limbs |x| < 2^31, total in [0, 2^261)
def _normalize_cases(field):
    m = MOD[field]
    rng = O.SplitMix64(0x3001 + field)
    res = []
    base = [(f, v) for f, v in structured(m, 160)] + [("random", rng_value(rng, 160 * m)) for _ in range(NRANDOM)]
    for fam, v in base:
        x = tight(v)
        res.append((fam + ", tight", [t & 0xFFFFFFFF for t in x]))
        # the same integer with carries pushed down: limb i + c*2^29, limb i+1 - c
        for c in (-2, 2):
            y = list(x)
            for i in range(8):
                ci = c if (rng.next() & 1) else -c
                y[i] += ci << 29
                y[i + 1] -= ci
            # limb i holds t + ci*2^29 - c(i-1): |.| < 2^29 + 2*2^29 + 2 < 2^31
            assert all(-(1 << 31) < t < (1 << 31) for t in y) and sum(t << (29 * i) for i, t in enumerate(y)) == v
            res.append((fam + ", carries of %d pushed down" % c, [t & 0xFFFFFFFF for t in y]))
    return res


def _signed(w):
    return [x - (1 << 32) if x >= (1 << 31) else x for x in w]


def _normalize_check(field, w, out):
    v = sum(t << (29 * i) for i, t in enumerate(_signed(w)))
    return need_tight(out) or (None if val(out) == v else "value %#x, want %#x" % (val(out), v))


SPECS["fp_normalize"] = Spec(_normalize_cases, _normalize_check, lambda field, w: tight(sum(t << (29 * i) for i, t in enumerate(_signed(w)))))


# ---- flags
def flag_spec(cases, expected):
    def check(field, w, out):
        want = expected(field, w)
        return None if out[0] == want else "returned %d, want %d" % (out[0], want)
    return Spec(cases, check, lambda field, w: [expected(field, w)])


def _is_canonical_cases(field):
    m = MOD[field]
    rng = O.SplitMix64(0x3100 + field)
    vs = [(f, v) for f, v in structured(m, 5) if v < (1 << 256)] + [("2^256-1", (1 << 256) - 1)]
    vs += [("random", rng_value(rng, 1 << 256)) for _ in range(NRANDOM)] + [("random near m", m - 8 + (rng.next() % 16)) for _ in range(64)]
    for _, v in vs:
        assert v < (1 << 256) and tight(v)[8] < (1 << 24)
    return [(f, tight(v)) for f, v in vs]


SPECS["fp_is_canonical"] = flag_spec(_is_canonical_cases, lambda field, w: int(val(w) < MOD[field]))


def _zero_test_cases(K):
    def cases(field):
        m = MOD[field]
        rng = O.SplitMix64(0x3200 + K)
        vs = []
        for k in range(K):
            vs.append(("%d*m" % k, k * m))
            vs.append(("%d*m + 2^29" % k, k * m + (1 << 29)))
            vs.append(("%d*m + 1" % k, k * m + 1))
            if k:
                vs.append(("%d*m - 1" % k, k * m - 1))
        vs += structured(m, K)
        vs += [("random", rng_value(rng, K * m)) for _ in range(NRANDOM)]
        for _, v in vs:
            assert 0 <= v < K * m
        return [(f, tight(v)) for f, v in vs]
    return cases


def _low_limbs_of_multiples(m, K, n):
    return {(k * m) & ((1 << (29 * n)) - 1) for k in range(K)}


for K in (4, 6, 10):
    # "maybe" = the low limb (two low limbs) is that of one of 0, m, .., (K-1)m: never misses a multiple, says "maybe" at k*m + 2^29
    SPECS["fp_maybe_zero_mod<%d>" % K] = flag_spec(_zero_test_cases(K), lambda field, w, K=K: int(w[0] in _low_limbs_of_multiples(MOD[field], K, 1)))
    SPECS["fp_maybe_zero_mod2<%d>" % K] = flag_spec(
        _zero_test_cases(K), lambda field, w, K=K: int((w[0] | (w[1] << 29)) in _low_limbs_of_multiples(MOD[field], K, 2)))
for K in (2, 4, 6, 8, 10):
    SPECS["fp_is_zero_mod<%d>" % K] = flag_spec(_zero_test_cases(K), lambda field, w: int(val(w) % MOD[field] == 0))


# ---- products.  terms: index pairs into the operands; sets: operand bounds per case set (call sites, then the largest allowed)
def product_spec(nops, results, bound_sets, seed, inplace=(), passthrough=(), loose_sets=None):
    """results: one list of (i, j) operand-index pairs per result (the result is the Montgomery reduction of their sum of products).
    Output record: the results, then the operands listed in passthrough, which must come back untouched."""

    def cases(field):
        m = MOD[field]
        res = []
        for bi, bs in enumerate(bound_sets):
            for fam, vs in operand_sets(m, _b(*bs), seed + 131 * bi, nrandom=share(len(bound_sets)), maxcross=MAXCROSS // len(bound_sets)):
                for v in vs:
                    assert v < R and tight(v)[8] <= M29     # every limb under 2^29: the products of a column are < 2^58
                res.append(("bounds %r: %s" % (list(bs), fam), words_of(vs)))
        for fam, ops in (loose_sets or []):
            res.append((fam, [x for o in ops for x in o]))
        return res

    def check(field, w, out):
        m = MOD[field]
        o = ops_of(w, nops)
        vs = [val(x) for x in o]
        for ri, terms in enumerate(results):
            r = out[9 * ri:9 * ri + 9]
            e = need_tight(r, "result %d" % ri) or check_mont(m, sum(vs[i] * vs[j] for i, j in terms), val(r))
            if e:
                return "result %d: %s" % (ri, e)
        for k, i in enumerate(passthrough):
            got = out[9 * (len(results) + k):9 * (len(results) + k) + 9]
            if got != o[i]:
                return "operand %d came back changed: %s" % (i, hexl(got))
        return None

    def model(field, w):
        m = MOD[field]
        o = ops_of(w, nops)
        vs = [val(x) for x in o]
        out = []
        for terms in results:
            out += tight(mont(m, sum(vs[i] * vs[j] for i, j in terms)))
        for i in passthrough:
            out += o[i]
        return out

    return Spec(cases, check, model)


MUL_BOUNDS = [(2, 2), (10, 2), (6, 12), (13, 13), (169, 169)]
SQR_BOUNDS = [(2,), (6,), (10,), (13,), (169,)]
MUL2_BOUNDS = [(6, 10, 4, 2), (8, 2, 6, 12), (4, 2, 4, 12), (169, 169, 169, 169)]


def _column_model_sets():
    """tools/fp_column_bounds.py CASES: the exact per-limb maxima the model multiplies out.  They exceed the value bounds slightly
    by construction; the product check (Montgomery identity, tight result) is what the model claims the hardware delivers."""
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import fp_column_bounds as CB
    assert CB.P == O.P
    return [("column model maxima of " + name, [list(a), list(b), list(c), list(d)]) for name, a, b, c, d in CB.CASES]


SPECS["fp_mul_ps"] = product_spec(2, [[(0, 1)]], MUL_BOUNDS, 0x4001)
SPECS["fp_mul_os"] = product_spec(2, [[(0, 1)]], MUL_BOUNDS, 0x4002)
SPECS["fp_sqr_ps"] = product_spec(1, [[(0, 0)]], SQR_BOUNDS, 0x4003)
SPECS["fp_sqr_os"] = product_spec(1, [[(0, 0)]], SQR_BOUNDS, 0x4004)
SPECS["fp_mul2_ps"] = product_spec(4, [[(0, 1), (2, 3)]], MUL2_BOUNDS, 0x4005)
SPECS["fp_mul2_os"] = product_spec(4, [[(0, 1), (2, 3)]], MUL2_BOUNDS, 0x4006)
SPECS["fp_mul3_ps"] = product_spec(6, [[(0, 1), (2, 3), (4, 5)]], [(2, 2) * 3, (13, 13) * 3, (169, 169) * 3], 0x4007)
SPECS["fp_mul_dual"] = product_spec(4, [[(0, 1)], [(2, 3)]], [(2, 2, 2, 2), (10, 2, 8, 2), (13, 13, 13, 13), (169, 169, 169, 169)], 0x4008)
SPECS["fp_sqr_dual"] = product_spec(2, [[(0, 0)], [(1, 1)]], [(10, 6), (4, 4), (13, 13), (169, 169)], 0x4009)
SPECS["fp_mul2_mul_mul"] = product_spec(8, [[(0, 1), (2, 3)], [(4, 5)], [(6, 7)]],
                                        [(6, 10, 4, 2, 2, 2, 2, 2), (4, 10, 2, 2, 2, 2, 2, 2), (13,) * 8, (169,) * 8], 0x400a)
SPECS["fpa_mul_ip"] = product_spec(2, [[(0, 1)]], MUL_BOUNDS, 0x4010, passthrough=(1,))
SPECS["fpa_mul"] = product_spec(2, [[(0, 1)]], MUL_BOUNDS, 0x4011, passthrough=(0, 1))
SPECS["fpa_sqr"] = product_spec(1, [[(0, 0)]], SQR_BOUNDS, 0x4012, passthrough=(0,))
SPECS["fpa_mul_dual_ip"] = product_spec(4, [[(0, 1)]], [], 0)   # replaced below (results interleaved with the operands)
SPECS["fpa_sqr_dual"] = product_spec(2, [[(0, 0)], [(1, 1)]], [(10, 6), (4, 4), (13, 13), (169, 169)], 0x4014, passthrough=(0, 1))
SPECS["fpa_mul2_ip1"] = product_spec(4, [[(0, 1), (2, 3)]], MUL2_BOUNDS, 0x4015, passthrough=(1, 2, 3), loose_sets=_column_model_sets())
SPECS["fpa_mul2_ip"] = product_spec(4, [[(0, 1), (2, 3)]], MUL2_BOUNDS, 0x4016, passthrough=(1, 2, 3), loose_sets=_column_model_sets())


def _dual_ip_spec():
    """fpa_mul_dual_ip(a, b, c, d): (a, c) <- (a*b, c*d); the probe stores a || b || c || d."""
    inner = product_spec(4, [[(0, 1)], [(2, 3)]], [(2, 2, 2, 2), (10, 2, 8, 2), (13, 13, 13, 13), (169, 169, 169, 169)], 0x4013,
                         passthrough=(1, 3))

    def reorder(out):    # a b c d -> r0 r1 b d
        return out[0:9] + out[18:27] + out[9:18] + out[27:36]

    def unorder(o):      # r0 r1 b d -> a b c d
        return o[0:9] + o[18:27] + o[9:18] + o[27:36]

    return Spec(inner.cases, lambda field, w, out: inner.check(field, w, reorder(out)), lambda field, w: unorder(inner.model(field, w)))


SPECS["fpa_mul_dual_ip"] = _dual_ip_spec()


# ---- the tail of the lean insertion: (Y1, PPP, r, Q, X3) at their bounds -> fp_neg_loose<KNY> / fp_sub_loose<10> -> the block
def loose_tail_spec(KNY, ybound, rbound, seed):
    bounds = [(ybound, True), (2, False), (rbound, False), (2, False), (9, True)]

    def cases(field):
        m = MOD[field]
        res = []
        for fam, vs in operand_sets(m, bounds, seed):
            assert vs[0] <= (KNY - 1) * m and vs[4] <= 9 * m
            res.append((fam, words_of(vs)))
        return res

    def check(field, w, out):
        m = MOD[field]
        y1, ppp, r, q, x3 = [val(x) for x in ops_of(w, 5)]
        y3, ny, d = out[0:9], out[9:18], out[18:27]
        if val(ny) != KNY * m - y1:
            return "ny: value %#x, want %d*m - Y1" % (val(ny), KNY)
        if val(d) != q - x3 + 10 * m:
            return "d: value %#x, want Q - X3 + 10*m" % val(d)
        if any(x >= (1 << 30) for x in ny[:8]) or any(x >= (1 << 29) + (1 << 30) for x in d[:8]):
            return "loose limbs above their stated maxima: ny %s d %s" % (hexl(ny), hexl(d))
        e = need_tight(y3) or check_mont(m, val(ny) * ppp + r * val(d), val(y3))
        if e:
            return e
        if val(y3) >= 2 * m:
            return "Y3 = %#x is not below 2m" % val(y3)
        return None

    def model(field, w):
        m = MOD[field]
        o = ops_of(w, 5)
        y1, ppp, r, q, x3 = [val(x) for x in o]
        bn, bd = km_borrowed(m, KNY), km_borrowed(m, 10)
        ny = [bn[i] - o[0][i] for i in range(NL)]
        d = [o[3][i] + bd[i] - o[4][i] for i in range(NL)]
        return tight(mont(m, val(ny) * ppp + r * val(d))) + ny + d

    return Spec(cases, check, model)


for tag in ("ip", "ip1"):
    SPECS["loose_tail<8,%s>" % tag] = loose_tail_spec(8, 4, 6, 0x4100)
    SPECS["loose_tail<4,%s>" % tag] = loose_tail_spec(4, 2, 4, 0x4101)


# ---- reduction
def _single_cases(B, seed, lim=None, inclusive=False):
    def cases(field):
        m = MOD[field]
        res = [(f, v) for f, v in operand_sets(m, [(B, inclusive)], seed) if lim is None or v[0] < lim]
        assert all(0 <= v[0] < B * m + inclusive and v[0] < R for f, v in res)     # "any value < 2^261" / canonical in (B = 1)
        return [(f, words_of(v)) for f, v in res]
    return cases


def value_spec(cases, expected, extra=None):
    def check(field, w, out):
        want = expected(field, w)
        e = need_tight(out)
        if e:
            return e
        if extra:
            return extra(field, w, out)
        return None if val(out) == want else "value %#x, want %#x" % (val(out), want)
    return Spec(cases, check, lambda field, w: tight(expected(field, w)))


SPECS["fp_canonical"] = value_spec(_single_cases(169, 0x5001), lambda field, w: val(w) % MOD[field])
SPECS["fp_from_mont"] = value_spec(_single_cases(169, 0x5002), lambda field, w: val(w) * pow(R, -1, MOD[field]) % MOD[field])


def _to_mont_extra(field, w, out):
    m = MOD[field]
    return check_mont(m, val(w) * (R * R % m), val(out)) or (None if val(out) < 2 * m else "result is not below 2m")


SPECS["fp_to_mont"] = value_spec(_single_cases(1, 0x5003), lambda field, w: mont(MOD[field], val(w) * (R * R % MOD[field])), extra=_to_mont_extra)


def _unpack_cases(field):
    rng = O.SplitMix64(0x5100 + field)
    vs = [("0", 0), ("2^256-1", (1 << 256) - 1), ("m", MOD[field]), ("m-1", MOD[field] - 1)]
    vs += [("word %d all ones" % i, 0xFFFFFFFF << (32 * i)) for i in range(8)]
    vs += [("bit %d" % i, 1 << i) for i in range(256)]
    vs += [("random", rng_value(rng, 1 << 256)) for _ in range(NRANDOM)]
    return vs


def _words256(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


SPECS["fp_unpack"] = Spec(lambda field: [(f, _words256(v)) for f, v in _unpack_cases(field)],
                          lambda field, w, out: (None if (is_tight(out) and out[8] < (1 << 24) and val(out) == sum(x << (32 * i) for i, x in enumerate(w)))
                                                 else "value %#x limbs %s" % (val(out), hexl(out))),
                          lambda field, w: tight(sum(x << (32 * i) for i, x in enumerate(w))))
SPECS["fp_pack"] = Spec(lambda field: [(f, tight(v)) for f, v in _unpack_cases(field)],
                        lambda field, w, out: None if list(out) == _words256(val(w)) else "words %s" % hexl(out),
                        lambda field, w: _words256(val(w)))


# ---- inversion
def _inv_values(field, seed):
    m = MOD[field]
    rng = O.SplitMix64(seed + field)
    vs = [("0", 0), ("1", 1), ("2", 2), ("m-1", m - 1), ("m-2", m - 2), ("(m-1)/2", (m - 1) // 2), ("(m+1)/2", (m + 1) // 2)]
    for k in range(254):
        vs.append(("2^%d" % k, 1 << k))
        vs.append(("2^%d-1" % k, (1 << k) - 1))
    vs += [("limb %d all ones" % i, M29 << (29 * i)) for i in range(NL)]
    vs += [("random", rng_value(rng, m)) for _ in range(2048)]
    return [(f, v) for f, v in vs if v < m]


def _inv_int_check(field, w, out):
    m = MOD[field]
    x, y = val(w), val(out)
    if not is_tight(out) or y >= m:
        return "result %#x is not canonical" % y
    if x == 0:
        return None if y == 0 else "inv(0) = %#x, want 0" % y
    return None if x * y % m == 1 else "x * inv = %#x (mod m), want 1" % (x * y % m)


SPECS["fp_inv_int"] = Spec(lambda field: [(f, tight(v)) for f, v in _inv_values(field, 0x6001)], _inv_int_check,
                           lambda field, w: tight(pow(val(w), -1, MOD[field]) if val(w) else 0))


def _inv_cases(field):
    """Montgomery in, any in-contract representative: x*R mod m + k*m for the k a tight value under 2^261 allows"""
    m = MOD[field]
    res = []
    for i, (f, v) in enumerate(_inv_values(field, 0x6002)):
        k = (0, 1, 2, 7, 167)[i % 5]
        res.append(("%s, representative + %d*m" % (f, k), tight(v * R % m + k * m)))
    return res


def _inv_check(field, w, out):
    m = MOD[field]
    rinv = pow(R, -1, m)
    x, y = val(w) * rinv % m, val(out)
    if not is_tight(out) or y >= 2 * m:
        return "result %#x is not a tight value below 2m" % y
    y = y * rinv % m
    if x == 0:
        return None if y == 0 else "inv(0) != 0"
    return None if x * y % m == 1 else "x * inv != 1 (mod m)"


def _inv_model(field, w):
    m = MOD[field]
    x = val(w) * pow(R, -1, m) % m
    return tight((pow(x, -1, m) if x else 0) * R % m)


SPECS["fp_inv"] = Spec(_inv_cases, _inv_check, _inv_model)


# --------------------------------------------------------------------------------------------------------- group law
P = O.P
RINV = pow(R, -1, P)
R1 = R % P
XYZZ_BOUNDS = (8, 4, 2, 2)      # csrc/g1.hpp:30-33, in multiples of p
AFF_BOUND = 2


def to_mont(x):
    return x * R % P


def rec_affine(rec):
    """the affine point an XYZZ record (36 limbs) stands for: de-Montgomery, X/ZZ, Y/ZZZ; ZZ the integer 0 is the identity"""
    x, y, zz, zzz = [val(rec[9 * i:9 * i + 9]) for i in range(4)]
    if zz == 0:
        return O.INF
    x, y, zz, zzz = [c * RINV % P for c in (x, y, zz, zzz)]
    return (x * pow(zz, -1, P) % P, y * pow(zzz, -1, P) % P)


def aff_point(w):
    """18 limbs, Montgomery; the integers (0, 0) are the identity"""
    x, y = val(w[0:9]), val(w[9:18])
    if x == 0 and y == 0:
        return O.INF
    return (x * RINV % P, y * RINV % P)


def check_record(rec, bounds=XYZZ_BOUNDS, limb_ok=is_tight, what="tight"):
    """invariant of a stored point: coordinates under their bounds, limbs tight, ZZ^3 = ZZZ^2"""
    cs = [rec[9 * i:9 * i + 9] for i in range(4)]
    for name, c, b in zip(("X", "Y", "ZZ", "ZZZ"), cs, bounds):
        if not limb_ok(c):
            return "%s limbs are not %s: %s" % (name, what, hexl(c))
        if val(c) >= b * P:
            return "%s = %#x is not below %d*p" % (name, val(c), b)
    zz, zzz = val(cs[2]) * RINV % P, val(cs[3]) * RINV % P
    if val(cs[2]) and pow(zz, 3, P) != zzz * zzz % P:
        return "ZZ^3 != ZZZ^2 (mod p)"
    return None


def check_point(out_rec, want, **kw):
    e = check_record(out_rec, **kw)
    if e:
        return e
    got = rec_affine(out_rec)
    if got != want:
        return "the record stands for %s, the oracle says %s" % (O.debug_fmt(got), O.debug_fmt(want))
    return None


def model_record(pt):
    if pt is O.INF:
        return tight(0) + tight(R1) + tight(0) + tight(0)
    return tight(to_mont(pt[0])) + tight(to_mont(pt[1])) + tight(R1) + tight(R1)


_POINTS = None


def base_points():
    """a few dozen multiples of G"""
    global _POINTS
    if _POINTS is None:
        rng = O.SplitMix64(0x7001)
        ks = [1, 2, 3, 4, 5, 7, 8, 15, 16, O.R - 1, O.R - 2, (O.R - 1) // 2] + [rng.fr() for _ in range(12)]
        _POINTS = [O.scalar_mul(k, O.G1) for k in ks]
    return _POINTS


def xyzz_base(pt, z):
    """canonical Montgomery coordinates (X, Y, ZZ, ZZZ) of pt with ZZ = z^2, ZZZ = z^3; z = 1: from_affine"""
    zz, zzz = z * z % P, z * z * z % P
    return [to_mont(pt[0] * zz % P), to_mont(pt[1] * zzz % P), to_mont(zz), to_mont(zzz)]


def aff_reps(pt, ks):
    cs = [to_mont(pt[0]) + ks[0] * P, to_mont(pt[1]) + ks[1] * P]
    assert all(c < AFF_BOUND * P for c in cs) and cs != [0, 0]
    return words_of(cs)


IDENT_XYZZ = tight(0) + tight(R1) + tight(0) + tight(0)
IDENT_AFF = tight(0) + tight(0)
ALL_AFF_KS = list(itertools.product(range(2), range(2)))


def xyzz_operands(seed, xbound=8):
    """(family, record, point): every base point as from_affine and with a random ZZ, in sampled representatives; the first point
    in EVERY representative the invariant allows; everything at the top of its range at once"""
    rng = O.SplitMix64(seed)
    allks = list(itertools.product(range(xbound), range(4), range(2), range(2)))
    res = []
    for i, pt in enumerate(base_points()):
        for z in (1, 1 + rng.fr() % (P - 1)):
            kss = allks if i < 1 else [(0, 0, 0, 0), (xbound - 1, 3, 1, 1)] + [allks[rng.next() % len(allks)] for _ in range(4)]
            for ks in kss:
                cs = [c + k * P for c, k in zip(xyzz_base(pt, z), ks)]
                assert all(c < b * P for c, b in zip(cs, (xbound, 4, 2, 2)))      # the invariant of a stored point
                res.append(("point %d, %s, representatives %r" % (i, "ZZ = ZZZ = 1" if z == 1 else "random ZZ", ks), words_of(cs), pt))
    return res


def aff_operands():
    return [("point %d, representatives %r" % (i, ks), aff_reps(pt, ks), pt) for i, pt in enumerate(base_points()) for ks in ALL_AFF_KS]


def _sample(rng, l, n):
    return l if len(l) <= n else [l[rng.next() % len(l)] for _ in range(n)]


def group_spec(cases, want, out_check=check_point):
    """want(words) -> the oracle's affine result"""
    def check(field, w, out):
        return out_check(out[:36], want(w))
    return Spec(cases, check, lambda field, w: model_record(want(w)))


def _double_cases(field):
    return [(f, r) for f, r, _ in xyzz_operands(0x7101)] + [("identity", IDENT_XYZZ)]


SPECS["xyzz_double"] = group_spec(_double_cases, lambda w: O.double(rec_affine(w[:36])))
SPECS["xyzz_double_affine"] = group_spec(lambda field: [(f, r) for f, r, _ in aff_operands()], lambda w: O.double(aff_point(w[:18])))


def _related(pt, others, rng, n=3):
    """the second operands that matter for a first operand pt: itself, its negation, and a few others"""
    rest = [o for o in others if o[0] != pt[0]]
    return [("same point", pt), ("opposite point", O.neg(pt))] + [("other point", rest[rng.next() % len(rest)]) for _ in range(n)]


def _add_affine_cases(field, lean=None):
    """(acc XYZZ, q affine[, sgn]).  lean: None for xyzz_add_affine (identities allowed on both sides), else the VAR bits"""
    rng = O.SplitMix64(0x7200 + (lean or 0))
    pts = base_points()
    res = []
    n = 0
    for fam, rec, pt in xyzz_operands(0x7201):
        for rel, q in _related(pt, pts, rng, 1):
            n += 1
            for ks in (ALL_AFF_KS[n % 4], ALL_AFF_KS[(n + 1 + n // 4 % 3) % 4]):   # two of the four, all four over neighbouring cases
                if lean is None:
                    res.append(("%s + %s %r" % (fam, rel, ks), rec + aff_reps(q, ks)))
                else:
                    # sgn applies to q as stored: the stored base is q or -q, so that +-q is the related point
                    for sgn in (0, SGN):
                        stored = q if sgn == 0 else O.neg(q)
                        res.append(("%s + (sgn %#x) %s %r" % (fam, sgn, rel, ks), rec + aff_reps(stored, ks) + [sgn]))
    if lean is None:
        for fam, rec, pt in xyzz_operands(0x7202)[:40]:
            res.append((fam + " + identity", rec + IDENT_AFF))
        for fam, r, _ in aff_operands():
            res.append(("identity + " + fam, IDENT_XYZZ + r))
        res.append(("identity + identity", IDENT_XYZZ + IDENT_AFF))
    elif lean & 1:    # LEAN_ID: the identity base must be refused
        for fam, rec, pt in xyzz_operands(0x7203)[:64]:
            for sgn in (0, SGN):
                res.append((fam + " + identity base (sgn %#x)" % sgn, rec + IDENT_AFF + [sgn]))
    return res


SPECS["xyzz_add_affine"] = group_spec(_add_affine_cases, lambda w: O.add(rec_affine(w[:36]), aff_point(w[36:54])))


def _signed_q(w, off):
    q = aff_point(w[off:off + 18])
    return O.neg(q) if w[off + 18] == SGN else q


def lean_spec(var, affine_affine):
    """The lean forms: true and the sum, or false — REQUIRED when q = +-acc or q is the identity (VAR & LEAN_ID) — with acc as it was"""
    noff = 18 if affine_affine else 36

    def first(w):
        return aff_point(w[:18]) if affine_affine else rec_affine(w[:36])

    def must_refuse(w):
        a, q = first(w), aff_point(w[noff:noff + 18])
        return q is O.INF or a[0] == q[0]

    def cases(field):
        if not affine_affine:
            res = _add_affine_cases(field, lean=var)
        else:
            rng = O.SplitMix64(0x7300 + var)
            pts = base_points()
            res = []
            for fam, r, pt in aff_operands():
                for rel, q in _related(pt, pts, rng):
                    for ks in ALL_AFF_KS:
                        for sgn in (0, SGN):
                            res.append(("%s + (sgn %#x) %s %r" % (fam, sgn, rel, ks), r + aff_reps(q if sgn == 0 else O.neg(q), ks) + [sgn]))
                if var & 1:
                    res.append((fam + " + identity base", r + IDENT_AFF + [0]))
        for fam, w in res:
            assert w[-1] in (0, SGN) and first(w) is not O.INF
            assert (var & 1) or aff_point(w[noff:noff + 18]) is not O.INF     # no identity to an instantiation without LEAN_ID
        return res

    def check(field, w, out):
        ok = out[36]
        if must_refuse(w):
            if ok != 0:
                return "returned true for q = +-acc or an identity base: the general formula was needed"
            if not affine_affine and list(out[:36]) != list(w[:36]):
                return "returned false with acc changed: %s" % hexl(out[:36])
            return None
        if ok != 1:
            return "returned false for an ordinary pair"
        return check_point(out[:36], O.add(first(w), _signed_q(w, noff)))

    def model(field, w):
        if must_refuse(w):
            return (list(w[:36]) if not affine_affine else IDENT_XYZZ) + [0]
        return model_record(O.add(first(w), _signed_q(w, noff))) + [1]

    return Spec(cases, check, model)


for _d in (1, 0):
    for _v in range(4):
        SPECS["xyzz_add_affine_lean<%d,%d>" % (_d, _v)] = lean_spec(_v, False)
        SPECS["xyzz_add_affine_affine_lean<%d,%d>" % (_d, _v)] = lean_spec(_v, True)


def _aa_cases(field):
    rng = O.SplitMix64(0x7400)
    pts = base_points()
    res = []
    for fam, r, pt in aff_operands():
        for rel, q in _related(pt, pts, rng):
            for ks in ALL_AFF_KS:
                res.append(("%s + %s %r" % (fam, rel, ks), r + aff_reps(q, ks)))
    return res


SPECS["xyzz_add_affine_affine"] = group_spec(_aa_cases, lambda w: O.add(aff_point(w[:18]), aff_point(w[18:36])))


def _add_cases(field, xbound=8, seed=0x7500):
    rng = O.SplitMix64(seed)
    pts = base_points()
    ops = xyzz_operands(seed + 1, xbound)
    by_pt = {}
    for fam, rec, pt in ops:
        by_pt.setdefault(pt, []).append((fam, rec))
    res = []
    for fam, rec, pt in ops:
        for rel, q in _related(pt, pts, rng, 1):
            if rel == "opposite point":
                # -pt in a representative of its own: X as pt's, Y = k*p - Y for every k that stays inside the invariant
                x, y, zz, zzz = [val(rec[9 * i:9 * i + 9]) for i in range(4)]
                for k in range(1, 5):
                    if 0 <= k * P - y < 4 * P:
                        res.append(("%s + its negation (Y -> %d*p - Y)" % (fam, k), rec + words_of([x, k * P - y, zz, zzz])))
            else:
                for f2, r2 in _sample(rng, by_pt[q], 2 if rel == "same point" else 1):
                    res.append(("%s + %s: %s" % (fam, rel, f2), rec + r2))
    for fam, rec, pt in ops[:40]:
        res.append((fam + " + identity", rec + IDENT_XYZZ))
        res.append(("identity + " + fam, IDENT_XYZZ + rec))
    res.append(("identity + identity", IDENT_XYZZ + IDENT_XYZZ))
    return res


for _n in ("xyzz_add", "xyzz_add_chains"):
    SPECS[_n] = group_spec(_add_cases, lambda w: O.add(rec_affine(w[:36]), rec_affine(w[36:72])))


# --------------------------------------------------------------------------------------------------------- limb-parallel
LP_SLACK = 3          # "nearly tight" (csrc/lp_kernels.hpp:14): 29 bits plus at most a few units; lp_carry yields limbs < 2^29 + 4
LP_BOUNDS = (9, 4, 2, 2)


def is_nearly_tight(l):
    return all(0 <= x <= M29 + 1 + LP_SLACK for x in l[:8]) and 0 <= l[8] < (1 << 32)


def nearly(rng, v):
    """the integer v in nearly tight limbs: one unit of limb i + 1 moved down into a small limb i"""
    l = tight(v)
    # a limb may exceed 2^29 - 1 by at most LP_SLACK + 1 units: borrow one 2^29 from above only where the limb is small enough
    for i in range(8):
        if l[i] <= LP_SLACK and l[i + 1] > 0 and (rng.next() & 1):
            l[i] += 1 << 29
            l[i + 1] -= 1
    assert val(l) == v and is_nearly_tight(l)
    return l


def lp_top_vectors(B, inclusive):
    """The top of the limb-parallel contract for an operand of bound B: every limb 0..7 at 2^29 + LP_SLACK (and alternating with
    2^29 - 1), under the largest top limb that keeps the value inside the bound — the worst columns of lp_mul."""
    lim = B * P + (1 if inclusive else 0)
    res = []
    for fam, low in (("limbs 0..7 at 2^29+%d" % LP_SLACK, [M29 + 1 + LP_SLACK] * 8),
                     ("limbs 0..7 alternating 2^29-1 / 2^29+%d" % LP_SLACK, [M29, M29 + 1 + LP_SLACK] * 4),
                     ("limbs 0..7 alternating 2^29+%d / 2^29-1" % LP_SLACK, [M29 + 1 + LP_SLACK, M29] * 4)):
        lv = val(low)
        l = low + [(lim - 1 - lv) >> 232]
        assert lv <= val(l) < lim and is_nearly_tight(l)
        res.append((fam + ", largest top limb", l))
    return res


def lp_rows(out):
    rows = [list(out[9 * i:9 * i + 9]) for i in range(4)]
    return rows[0], (None if all(r == rows[0] for r in rows) else "the four rows disagree: " + " ".join(hexl(r) for r in rows))


def lp_value_spec(nops, bounds, expr, seed, product=False, cover=None):
    def cases(field):
        rng = O.SplitMix64(seed ^ 0x55)
        res = []
        for bi, bs in enumerate(bounds):
            for fam, vs in operand_sets(P, bs, seed + bi, nrandom=share(len(bounds)), maxcross=MAXCROSS // (4 * len(bounds))):
                res.append(("bounds %r: %s" % ([b for b, _ in bs], fam), words_of(vs)))
                nl = [nearly(rng, v) for v in vs]
                if nl != [tight(v) for v in vs]:
                    res.append(("bounds %r: %s, nearly tight" % ([b for b, _ in bs], fam), [x for l in nl for x in l]))
            # every operand at the top of the nearly tight contract at once, and each against the others' tight all-ones vector
            tops = [lp_top_vectors(B, inc) for B, inc in bs]
            ones = [tight(next(v for f, v in structured(P, B, inc) if f == ALL_ONES)) for B, inc in bs]
            for combo in itertools.product(*tops):
                res.append(("bounds %r: %s" % ([b for b, _ in bs], " | ".join(f for f, _ in combo)), [x for _, l in combo for x in l]))
            for i in range(len(bs)):
                for f, l in tops[i]:
                    ops = list(ones)
                    ops[i] = l
                    res.append(("bounds %r: operand %d %s, the rest tight all ones" % ([b for b, _ in bs], i, f), [x for o in ops for x in o]))
        if cover:
            for fam, w in res:
                cover(ops_of(w, nops))
        return res

    def check(field, w, out):
        r, e = lp_rows(out)
        if e:
            return e
        if not is_nearly_tight(r):
            return "result limbs are not nearly tight: %s" % hexl(r)
        vs = [val(o) for o in ops_of(w, nops)]
        if product:
            return check_mont(P, vs[0] * vs[1], val(r))
        return None if val(r) == expr(vs) else "value %#x, want the integer %#x" % (val(r), expr(vs))

    def model(field, w):
        vs = [val(o) for o in ops_of(w, nops)]
        return tight(mont(P, vs[0] * vs[1]) if product else expr(vs)) * 4

    return Spec(cases, check, model)


def _lp_cover(K, idx):
    """REQUIRES of the borrowed subtraction: no limb difference goes negative — every limb of the subtrahend is covered by the
    borrowed constant's (csrc/lp_kernels.hpp:15-16)"""
    c = lp_borrowed(K)

    def cover(ops):
        assert all(ops[idx][i] <= c[i] for i in range(NL)), "lp borrowed %d*p does not cover %s" % (K, hexl(ops[idx]))
    return cover


SPECS["lp_mul"] = lp_value_spec(2, [_b(2, 2), _b(9, 2), _b(8, 8), _b(5, 13), _b(6, 11), _b(13, 13)], None, 0x8001, product=True)
for K, AS in ((3, (2,)), (5, (2,)), (7, (2,)), (9, (2,)), (11, (2,))):
    SPECS["lp_sub<%d>" % K] = lp_value_spec(2, [[(A, False), (K - 1, True)] for A in AS], lambda v, K=K: v[0] - v[1] + K * P, 0x8100 + K,
                                            cover=_lp_cover(K, 1))
for K in (3, 5):
    SPECS["lp_neg<%d>" % K] = lp_value_spec(1, [[(K - 1, True)]], lambda v, K=K: K * P - v[0], 0x8200 + K, cover=_lp_cover(K, 0))
SPECS["lp_triple"] = lp_value_spec(1, [_b(2), _b(8)], lambda v: 3 * v[0], 0x8300)


def _lp_point_check(rec, want):
    return check_point(rec, want, bounds=LP_BOUNDS, limb_ok=is_nearly_tight, what="nearly tight")


def _lp_double_cases(field):
    return [(f, r) for f, r, _ in xyzz_operands(0x8401, xbound=9)] + [("identity", IDENT_XYZZ)]


SPECS["lp_double"] = group_spec(_lp_double_cases, lambda w: O.double(rec_affine(w[:36])), out_check=_lp_point_check)
SPECS["lp_add_points"] = group_spec(lambda field: _add_cases(field, xbound=9, seed=0x8500),
                                    lambda w: O.add(rec_affine(w[:36]), rec_affine(w[36:72])), out_check=_lp_point_check)


# --------------------------------------------------------------------------------------------------------- running a check
_CASES = {}


def cases(field, name):
    """the case set of (field, op): computed once, shared, never changed"""
    key = (field, name)
    if key not in _CASES:
        _CASES[key] = SPECS[name].cases(field)
    return _CASES[key]


def verify(field, name, case_list, outs):
    """Raises AssertionError naming the op, the case family and the first failing case's limbs in hex."""
    spec = SPECS[name]
    bad = []
    for (fam, w), out in zip(case_list, outs):
        e = spec.check(field, w, list(out))
        if e:
            bad.append((fam, w, out, e))
    if bad:
        fam, w, out, e = bad[0]
        raise AssertionError("%s (%s): %d of %d cases wrong; first: family '%s': %s\n  in : %s\n  out: %s" % (
            name, "Fq" if field == FQ else "Fr", len(bad), len(case_list), fam, e,
            " ".join(hexl(w[i:i + 9]) for i in range(0, len(w), 9)), " ".join(hexl(out[i:i + 9]) for i in range(0, len(out), 9))))
