"""GPU: the batched Fourier transform over Fr — h2agg_fr_fft_batch (a slab [m][2^k] in one call) and poly.columns_* over it.

The yardstick is that of tests/test_gpu_fr_fft.py: ntt_py, which that file ties to the definition in include/h2agg.h, on
random_input columns.  Every column of a slab has a seed of its own, so a swapped or a repeated column is seen; column j of a
given k is the same in every slab, so its reference is computed once.  Results are exact and compared byte for byte."""
import functools
import importlib
import random

import pytest

import __graft_entry__ as entry
from oracle import bn254 as O
from oracle import verifier as V
from tests.fr_bytes import dec, enc
from tests.test_gpu_fr_fft import BIG_SHIFT, ntt_py, random_input

pytestmark = pytest.mark.gpu

R = O.R


@pytest.fixture(scope="module")
def poly(pkg):
    return importlib.import_module(entry.PKG_NAME + ".poly")


@functools.lru_cache(maxsize=None)
def column(k, j):
    return tuple(random_input(9000 + 32 * k + j, k))


@functools.lru_cache(maxsize=None)
def reference(k, j, inverse, shift):
    """the bytes h2agg_fr_fft owes for column(k, j)"""
    return enc(ntt_py(column(k, j), k, inverse, shift))


def slab(k, m):
    return b"".join(enc(column(k, j)) for j in range(m))


def want(k, m, inverse, shift):
    return b"".join(reference(k, j, inverse, shift) for j in range(m))


def fe(shift):
    return None if shift is None else shift.to_bytes(32, "little")


def check(eng, k, m, inverse, shift, what=None):
    got = eng.fr_fft_batch(slab(k, m), k, inverse, fe(shift))
    ref = want(k, m, inverse, 1 if shift is None else shift)
    col = 32 << k
    for j in range(m):
        assert got[j * col:(j + 1) * col] == ref[j * col:(j + 1) * col], (what, k, m, inverse, shift, "column", j)
    assert len(got) == m * col
    return got


# ---------------------------------------------------------------------------------------------- 1. small k, all shifts
@pytest.mark.parametrize("k,ms", [(k, (1, 2, 3, 5)) for k in range(0, 13)] + [(7, (17,)), (10, (3,))])
def test_small_k_every_shift(eng, poly, k, ms):
    """k = 7, m = 17: a workgroup of 16 whole transforms and one that is nearly empty; k = 10, m = 3: two transforms in a
    workgroup and one left over"""
    for m in ms:
        for inverse in (False, True):
            for sh in (None, poly.ZETA_INT, BIG_SHIFT):
                check(eng, k, m, inverse, sh)


# ---------------------------------------------------------------------------------------------- 2. pass boundaries
@pytest.mark.parametrize("local,k,m", [(1, 3, 3), (2, 5, 3), (3, 7, 5), (3, 10, 3)])
def test_pass_boundaries_at_the_smallest_size(eng, local, k, m):
    try:
        eng.debug_configure("fr_fft_local", local)
        for inverse in (False, True):
            check(eng, k, m, inverse, BIG_SHIFT, ("local", local))
    finally:
        eng.debug_configure("fr_fft_local", 0)


# ---------------------------------------------------------------------------------------------- 3. forced chunks
@pytest.mark.parametrize("local,k", [(0, 11), (3, 7)])
def test_forced_chunks(eng, local, k):
    """m = 5 in chunks of 1, 2 (2, 2 and a last chunk of one) and 4 (4 and one), two passes at k = 11 and three at k = 7"""
    m = 5
    try:
        eng.debug_configure("fr_fft_local", local)
        for inverse in (False, True):
            unforced = check(eng, k, m, inverse, BIG_SHIFT, "unforced")
            for chunk in (1, 2, 4):
                eng.debug_configure("fr_fft_batch_chunk", chunk)
                assert check(eng, k, m, inverse, BIG_SHIFT, ("chunk", chunk)) == unforced
                buf = bytearray(slab(k, m))                    # in place, chunk by chunk
                assert eng.fr_fft_batch(buf, k, inverse, fe(BIG_SHIFT)) is buf and bytes(buf) == unforced, (chunk, "in place")
                eng.debug_configure("fr_fft_batch_chunk", 0)
    finally:
        eng.debug_configure("fr_fft_batch_chunk", 0)
        eng.debug_configure("fr_fft_local", 0)


def test_forced_chunk_refuses_a_negative_size(eng, pkg):
    with pytest.raises(pkg.H2AggError) as ei:
        eng.debug_configure("fr_fft_batch_chunk", -1)
    assert ei.value.code == pkg.ERR_INVALID
    check(eng, 4, 3, False, BIG_SHIFT)


# ---------------------------------------------------------------------------------------------- 4. default-plan boundaries
@pytest.mark.parametrize("k", [9, 10, 11, 20, 21])
def test_default_plan_boundaries_against_the_single_transform(eng, pkg, poly, k):
    """k = 11 = FR_FFT_TILE_LOG is the first size at which a workgroup holds less than a column; 20 and 21: two and three
    passes.  The slab is random bytes as in test_default_plan_boundaries_round_trip, the reference the per-column call."""
    assert pkg.FR_FFT_LOCAL == 10
    m, n = 2, 1 << k
    buf = bytearray(random.Random(9400 + k).randbytes(32 * n * m))
    buf[31::32] = bytes(b & 0x1F for b in buf[31::32])      # every element < 2^253 < r
    for pos, v in ((0, 0), (n // 2 + 1, 1), (n - 1, R - 1), (n, R - 1), (2 * n - 1, 0)):
        buf[32 * pos:32 * pos + 32] = v.to_bytes(32, "little")
    data = bytes(buf)
    assert data[:32 * n] != data[32 * n:]
    for sh in (None, poly.ZETA, BIG_SHIFT.to_bytes(32, "little")):
        mid = eng.fr_fft_batch(data, k, False, sh)
        for j in range(m):
            assert mid[32 * n * j:32 * n * (j + 1)] == eng.fr_fft(data[32 * n * j:32 * n * (j + 1)], k, False, sh), (k, sh, j)
        assert eng.fr_fft_batch(mid, k, True, sh) == data, (k, sh)


# ---------------------------------------------------------------------------------------------- 5. in place, refusals
def test_in_place(eng):
    for k, m in ((6, 3), (11, 3), (12, 2)):                 # one workgroup for all, a workgroup per column, two passes
        buf = bytearray(slab(k, m))
        assert eng.fr_fft_batch(buf, k, False, fe(BIG_SHIFT)) is buf
        assert bytes(buf) == want(k, m, False, BIG_SHIFT), (k, m)
        assert eng.fr_fft_batch(buf, k, True, fe(BIG_SHIFT)) is buf
        assert bytes(buf) == slab(k, m), (k, m)


def test_refusals_leave_the_context_usable(eng, pkg):
    k, m = 4, 3
    good = slab(k, m)

    def still_works():
        assert eng.fr_fft_batch(good, k, False, fe(BIG_SHIFT)) == want(k, m, False, BIG_SHIFT)

    for code, args in ((pkg.ERR_INVALID, (b"", k)),                                        # m == 0
                       (pkg.ERR_INVALID, (bytes(32), 25)),
                       (pkg.ERR_INVALID, (good, k, False, bytes(32))),                     # shift == 0
                       (pkg.ERR_INVALID, (good, k, True, bytes(32))),
                       (pkg.ERR_NONCANONICAL, (good, k, False, R.to_bytes(32, "little"))),
                       (pkg.ERR_NONCANONICAL, (good, k, True, (R + 5).to_bytes(32, "little")))):
        with pytest.raises(pkg.H2AggError) as ei:
            eng.fr_fft_batch(*args)
        assert ei.value.code == code, (args[1:], ei.value)
        still_works()
    for kk, mm in ((5, 3), (12, 2)):                        # an element >= r in the last column only
        bad = bytearray(slab(kk, mm))
        at = 32 * ((mm - 1) * (1 << kk) + 13)
        bad[at:at + 32] = R.to_bytes(32, "little")
        for inverse in (False, True):
            with pytest.raises(pkg.H2AggError) as ei:
                eng.fr_fft_batch(bytes(bad), kk, inverse)
            assert ei.value.code == pkg.ERR_NONCANONICAL, (kk, inverse)
            still_works()
    with pytest.raises(ValueError):
        eng.fr_fft_batch(good + bytes(32), k)               # not a whole number of columns


# ---------------------------------------------------------------------------------------------- 6. poly.columns_*
def test_poly_columns_equal_the_per_column_functions(eng, poly):
    k, ek, m = 5, 7, 3
    cols = [enc(column(k, j)) for j in range(m)]
    wide = [enc(column(ek, j)) for j in range(m)]
    assert poly.columns_coeff_to_lagrange(eng, cols, k) == [poly.coeff_to_lagrange(eng, c, k) for c in cols]
    assert poly.columns_coeff_to_lagrange(eng, cols, k) == [reference(k, j, False, 1) for j in range(m)]
    assert poly.columns_lagrange_to_coeff(eng, cols, k) == [poly.lagrange_to_coeff(eng, c, k) for c in cols]
    assert poly.columns_lagrange_to_coeff(eng, poly.columns_coeff_to_lagrange(eng, cols, k), k) == cols
    ext = poly.columns_coeff_to_extended(eng, cols, k, ek)
    assert ext == [poly.coeff_to_extended(eng, c, k, ek) for c in cols]
    assert poly.columns_coeff_to_extended(eng, cols, k, ek, fe(BIG_SHIFT)) == [poly.coeff_to_extended(eng, c, k, ek, fe(BIG_SHIFT)) for c in cols]
    assert poly.columns_extended_to_coeff(eng, wide, ek) == [poly.extended_to_coeff(eng, c, ek) for c in wide]
    assert poly.columns_extended_to_coeff(eng, ext, ek) == [c + bytes((32 << ek) - (32 << k)) for c in cols]
    w = V.omega_for_k(ek)
    for j in range(m):                                       # Horner, as test_poly_extended_domain
        got = dec(ext[j])
        for i in (0, 1, 2, 31, 32, 77, 126, 127):
            x, v = poly.ZETA_INT * pow(w, i, R) % R, 0
            for c in reversed(column(k, j)):
                v = (v * x + c) % R
            assert got[i] == v, (j, i)
    # a list of bytearrays is accepted and left alone
    arrays = [bytearray(c) for c in cols]
    assert poly.columns_coeff_to_lagrange(eng, arrays, k) == [reference(k, j, False, 1) for j in range(m)]
    assert [bytes(a) for a in arrays] == cols
