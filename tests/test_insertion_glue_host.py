"""CPU tests for the bucket insertion's glue: which instantiation a call takes (host logic of csrc/h2agg.hip, through the C ABI —
no device needed), and the 64-bit column bound of the product block that takes two loose operands (tools/fp_column_bounds.py)."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fp_column_bounds as B  # noqa: E402

LEAN_ID, LEAN_ENDO = 1, 2


@pytest.mark.parametrize("no_identity,glv,want", [(0, 0, LEAN_ID), (0, 1, LEAN_ID | LEAN_ENDO), (1, 0, 0), (1, 1, LEAN_ENDO),
                                                  (7, -3, LEAN_ENDO)])
def test_lean_variant_of_a_call(pkg, no_identity, glv, want):
    """the identity test stays unless the table is KNOWN to hold none; the endomorphism select stays when the plan splits scalars"""
    lib = ctypes.CDLL(pkg.LIB_PATH)
    lib.h2agg_debug_lean_variant.restype = ctypes.c_int
    assert lib.h2agg_debug_lean_variant(ctypes.c_int(no_identity), ctypes.c_int(glv)) == want


def test_borrowed_multiples_of_p():
    for k in (4, 8, 10):
        b = B.km_limbs_borrowed(k)
        assert sum(x << (29 * i) for i, x in enumerate(b)) == k * B.P
        assert all(B.M29 <= x < (1 << 30) for x in b[:8])            # covers a tight limb; the difference stays < 2^30
        assert b[8] >= ((k - 1) * B.P) >> (29 * 8)                    # the top limb covers a subtrahend <= (k - 1) p


def test_loose_operands_fit_the_columns_of_the_two_product_block():
    """the worst-case accumulator of fpa_mul2_ip / fpa_mul2_ip1 for the operand bounds the insertion claims (CASES) stays below
    2^64 — and the check is not vacuous: with BOTH operands of a product loose, or with unmasked 32-bit limbs, it does not"""
    assert B.check()
    for name, a, b, c, d in B.CASES:
        for two in (True, False):
            worst, last = B.mul2_column_max(a, b, c, d, two)
            assert worst < 1 << 64 and (last >> 29) < 1 << 32, name
            assert worst > 27 * (1 << 58)                             # more than the tight-operand bound the block was generated for
    loose = B.sub_loose(10, 2, 8)
    assert B.mul2_column_max(B.neg_loose(8, 4), loose, loose, loose, True)[0] >= 1 << 64
    full = [(1 << 32) - 1] * 9
    assert B.mul2_column_max(full, B.tight(2), B.tight(6), full, True)[0] >= 1 << 64


def test_tight_operands_reproduce_the_generator_comment():
    """27 products of < 2^58 per column (tools/gen_fp_asm.py): the model reproduces that bound for tight operands"""
    t = B.tight(2)
    worst, _ = B.mul2_column_max(t, t, t, t, True)
    assert worst < 27 * (1 << 58) + (1 << 40)
