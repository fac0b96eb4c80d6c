#!/usr/bin/env python3
"""Worst-case 64-bit column sums of the two-product Montgomery blocks (csrc/fp_asm.inc fpa_mul2_ip / fpa_mul2_ip1) for the operand
limb bounds the bucket insertion hands them (csrc/msm_kernels.hpp xyzz_add_affine_lean / xyzz_add_affine_affine_lean).

The blocks are generated for TIGHT operands (limbs 0..7 < 2^29): "27 products of < 2^58 per column fit 64 bits".  The insertion
passes two operands LOOSE — d = Q - X3 + 10p and ny = Kp - Y1 formed limb by limb against a borrowed-form multiple of p, without
the carry sweep (csrc/fp.hpp fp_sub_loose / fp_neg_loose) — one per product.  This multiplies the schedule out: it walks the
very term lists tools/gen_fp_asm.py emits (cols_mul, the reduction terms, their split over the two partial sums), with every
limb at its largest possible value, and reports the largest value any 64-bit accumulator can reach.

    python3 tools/fp_column_bounds.py          table of the cases the code uses; exit 1 if one does not fit
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_fp_asm as G  # noqa: E402

NL = G.NL
P = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
M29 = (1 << 29) - 1


def km_limbs(k):
    """tight limbs of k * p (fp.hpp km_limb)"""
    v = k * P
    return [(v >> (29 * i)) & M29 if i < 8 else v >> (29 * 8) for i in range(NL)]


def km_limbs_borrowed(k):
    """fp.hpp km_limb_borrowed: 2^29 added to every limb below the top one, paid for by the limb above"""
    t = km_limbs(k)
    b = [t[i] + ((1 << 29) if i < 8 else 0) - (1 if i > 0 else 0) for i in range(NL)]
    assert sum(x << (29 * i) for i, x in enumerate(b)) == k * P
    assert all(x >= M29 for x in b[:8])          # covers any tight limb
    return b


def tight(bound):
    """largest limbs of a carry-normalised value < bound * p"""
    return [M29] * 8 + [(bound * P) >> (29 * 8)]


def neg_loose(k, bound_a):
    """limbs of fp_neg_loose<k>(a), a tight with value <= bound_a * p <= (k - 1) * p: largest where a's limb is 0"""
    assert bound_a <= k - 1
    b = km_limbs_borrowed(k)
    assert b[8] >= tight(bound_a)[8]             # the top limb cannot go negative
    return b


def sub_loose(k, bound_a, bound_b):
    """limbs of fp_sub_loose<k>(a, b): a tight < bound_a * p added, b tight <= bound_b * p <= (k - 1) * p subtracted"""
    assert bound_b <= k - 1
    b = km_limbs_borrowed(k)
    assert b[8] >= tight(bound_b)[8]
    return [x + y for x, y in zip(b, tight(bound_a))]


def mul2_column_max(a, b, c, d, two_sums):
    """largest accumulator value over all columns of a*b + c*d with one reduction; a..d: per-limb maxima.
    two_sums: fpa_mul2_ip (reduction terms balanced over two partial sums, folded per column); else fpa_mul2_ip1 (one chain).
    -> (largest 64-bit accumulator value, value in front of the last v_alignbit)"""
    mod = km_limbs(1)
    val = {}
    for base, limbs in ((0, a), (9, b), (18, c), (27, d), (36, mod)):
        for i in range(NL):
            val[f"%{base + i}"] = limbs[i]
    for m in G.C0.m:
        val[m] = M29                              # quotient digits are masked to 29 bits
    cols_a, cols_b = G.cols_mul(G.ops(0), G.ops(9)), G.cols_mul(G.ops(18), G.ops(27))
    worst = 0
    carry = 0
    for k in range(2 * NL - 1):
        ta, tb = list(cols_a[k]), list(cols_b[k])
        red = [(G.C0.m[i], f"%{36 + k - i}") for i in range(NL) if i < k and 0 <= k - i < NL]
        if two_sums:
            for r in red:                         # as montgomery_2sum balances them
                (ta if len(ta) <= len(tb) else tb).append(r)
        else:
            ta = ta + tb + red
            tb = []
        sa = carry + sum(val[x] * val[y] for x, y in ta)
        sb = sum(val[x] * val[y] for x, y in tb)
        t = sa + sb                               # v_lshl_add_u64 fold (or the single chain)
        if k < NL:
            t += M29 * mod[0]                     # + m_k * p_0
        worst = max(worst, sa, sb, t)
        last = t
        carry = t >> 29
    return worst, last


# (name, a, b, c, d): the operands of fpa_mul2_ip(ny, PPP, r, d) as the insertion forms them
CASES = [
    # mixed addition: ny = 8p - Y1 (Y1 <= [4]) loose, PPP [2], r [6], d = Q - X3 + 10p (Q [2], X3 [8]) loose
    ("xyzz_add_affine_lean", neg_loose(8, 4), tight(2), tight(6), sub_loose(10, 2, 8)),
    # second point of a bucket: ny = 4p - y1 (y1 <= [2]) loose, PPP [2], r [4], d as above
    ("xyzz_add_affine_affine_lean", neg_loose(4, 2), tight(2), tight(4), sub_loose(10, 2, 8)),
]


def check(verbose=False):
    ok = True
    for name, a, b, c, d in CASES:
        for two in (True, False):
            worst, last = mul2_column_max(a, b, c, d, two)
            fits = worst < (1 << 64) and (last >> 29) < (1 << 32)
            ok &= fits
            if verbose:
                print("%-30s %-13s largest accumulator 2^%.3f  (%.1f %% of 2^64)  %s" % (
                    name, "fpa_mul2_ip" if two else "fpa_mul2_ip1", math.log2(worst),
                    100.0 * worst / (1 << 64), "fits" if fits else "OVERFLOWS"))
    return ok


if __name__ == "__main__":
    sys.exit(0 if check(verbose=True) else 1)
