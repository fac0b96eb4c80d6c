"""The coset-split ending of h2agg_quotient, with Python integers: the decomposition itself and the constants
the host code has to produce.

Write a coefficient index of H as j = i n + l, l < n: H = sum_i X^(n i) h_i.  Coset c' of the extended domain is the points
s w^r, s = zeta w_ext^c', w = w_ext^(2^e) the root for k.  Two steps give the pieces back from H's values on the cosets:
  1. u_c' = the size-n inverse transform at shift s (include/h2agg.h's inverse) of H's values on coset c':
     u_c'[l] = sum_i (zeta^n)^i w_E^(c' i) h_i[l],  w_E = w_ext^n a primitive 2^e-th root of unity;
  2. h_i[l] = zeta^(-n i) / 2^e * sum_c' u_c'[l] w_E^(-c' i).
The library transforms the numerator N = H (X^n - 1), not H: on coset c' that is H's values times the scalar s^n - 1, and the
transform is linear, so the division moves into the constants: T[i][c'] = zeta^(-n i) w_E^(-c' i) / (2^e (s_c'^n - 1)).
Both forms are held here, with poly.ZETA and the root convention of tests/quotient_ref.py (the library's: oracle/verifier.py).

quotient_work_bytes: the sum DESIGN.md states, and (a key needs a context, so this one test is marked gpu) the binding."""
import importlib
import random

import pytest

import __graft_entry__ as entry
from tests import quotient_ref as Q

R = Q.R
MAX_K = 24   # FFT_MAX_K: the largest single transform


@pytest.fixture(scope="module")
def poly(pkg):
    return importlib.import_module(entry.PKG_NAME + ".poly")


def inv(x):
    return pow(x % R, R - 2, R)


def coset_values(H, k, e):
    """H: 2^(k+e) coefficients -> [coset c'][row r] = H(zeta w_ext^c' w^r), from ONE transform of size 2^(k+e)"""
    values = Q.ntt(H, k + e, Q.ZETA)
    return [[values[(r << e) | c] for r in range(1 << k)] for c in range(1 << e)]


def cross_table(zeta, k, e, pieces, divide):
    """T[i][c'] = zeta^(-n i) w_E^(-c' i) / 2^e, and with `divide` also / (s_c'^n - 1)"""
    n, cosets = 1 << k, 1 << e
    zn, w_E = pow(zeta, n, R), pow(Q.omega(k + e), n, R)
    assert pow(w_E, cosets, R) == 1 and (e == 0 or pow(w_E, cosets // 2, R) == R - 1), "w_E is a primitive 2^e-th root"
    table = []
    for i in range(pieces):
        row = []
        for c in range(cosets):
            t = inv(pow(zn, i, R)) * inv(pow(w_E, c * i, R)) % R * inv(cosets) % R
            if divide:
                t = t * inv(zn * pow(w_E, c, R) - 1) % R
            row.append(t)
        table.append(row)
    return table


def cross_cosets(u, table):
    """what k_qe_cross_cosets computes: h[i][l] = sum_c' u[c'][l] T[i][c']"""
    return [[sum(u[c][l] * row[c] for c in range(len(u))) % R for l in range(len(u[0]))] for row in table]


@pytest.mark.parametrize("e", [0, 1, 2, 3])
@pytest.mark.parametrize("k", [3, 4])
def test_the_two_steps_reproduce_the_pieces(poly, k, e):
    assert poly.ZETA_INT == Q.ZETA
    rng = random.Random(0xE50 + 8 * k + e)
    n, cosets = 1 << k, 1 << e
    H = [rng.choice((0, R - 1)) if rng.randrange(8) == 0 else rng.randrange(R) for _ in range(n << e)]
    h = [H[i * n:(i + 1) * n] for i in range(cosets)]
    w_ext = Q.omega(k + e)
    assert pow(w_ext, cosets, R) == Q.omega(k)
    shifts = [poly.ZETA_INT * pow(w_ext, c, R) % R for c in range(cosets)]
    on_cosets = coset_values(H, k, e)
    # step 1
    u = [Q.ntt(on_cosets[c], k, shifts[c], inverse=True) for c in range(cosets)]
    zn, w_E = pow(poly.ZETA_INT, n, R), pow(w_ext, n, R)
    for c in range(cosets):
        assert pow(shifts[c], n, R) == zn * pow(w_E, c, R) % R
        assert u[c] == [sum(pow(zn, i, R) * pow(w_E, c * i, R) % R * h[i][l] for i in range(cosets)) % R for l in range(n)]
    # step 2: all 2^e pieces, and any smaller number of them (degree - 1 need not be a power of two)
    assert cross_cosets(u, cross_table(poly.ZETA_INT, k, e, cosets, False)) == h
    for pieces in {1, cosets - 1, (cosets + 1) // 2} - {0}:
        assert cross_cosets(u, cross_table(poly.ZETA_INT, k, e, pieces, False)) == h[:pieces]
    # the library's form: the numerator's values go through step 1, the division by s^n - 1 rides in the constants
    numer = [[v * (pow(shifts[c], n, R) - 1) % R for v in on_cosets[c]] for c in range(cosets)]
    u_numer = [Q.ntt(numer[c], k, shifts[c], inverse=True) for c in range(cosets)]
    assert cross_cosets(u_numer, cross_table(poly.ZETA_INT, k, e, cosets, True)) == h


def test_a_missing_factor_is_seen():
    """the 1 / 2^e and the zeta^(-n i) of the constants: without the first every piece differs, without the second every
    piece whose index is no multiple of three"""
    k, e = 3, 2
    rng = random.Random(0xE51)
    n, cosets = 1 << k, 1 << e
    H = [rng.randrange(R) for _ in range(n << e)]
    h = [H[i * n:(i + 1) * n] for i in range(cosets)]
    w_ext = Q.omega(k + e)
    on_cosets = coset_values(H, k, e)
    u = [Q.ntt(on_cosets[c], k, Q.ZETA * pow(w_ext, c, R) % R, inverse=True) for c in range(cosets)]
    good = cross_table(Q.ZETA, k, e, cosets, False)
    assert cross_cosets(u, good) == h
    unscaled = [[t * cosets % R for t in row] for row in good]
    assert all(a != b for a, b in zip(cross_cosets(u, unscaled), h))
    zn = pow(Q.ZETA, n, R)
    no_zeta = [[t * pow(zn, i, R) % R for t in row] for i, row in enumerate(good)]
    got = cross_cosets(u, no_zeta)
    assert [a == b for a, b in zip(got, h)] == [True, False, False, True]   # zeta^n is a cube root of unity: (zeta^n)^3 = 1


# ---------------------------------------------------------------------------------------------- work memory
def work_bytes(k, degree, inputs):
    """(input polynomials + 9) n + 2^(k+e) elements, and the transforms' work array, max(W, min((input
    polynomials + 3) n, 2^23)) elements with W = 2^(k+e), on the split route (k + e > 24) n; 32 bytes each"""
    n, e = 1 << k, Q.extended_k(k, degree)
    largest = n if k + e > MAX_K else n << e
    return 32 * ((inputs + 9) * n + (n << e) + max(largest, min((inputs + 3) * n, 1 << 23)))


def test_the_sum_at_the_sizes_the_documents_name():
    assert work_bytes(24, 6, 34) == 52 << 29                      # 51 + 1 columns of 512 MiB: 26 GiB
    assert work_bytes(20, 4, 31) == (40 << 25) + (128 << 20) + (256 << 20)   # the measured shape: 1.4 GiB, and 2^23 elements of work


@pytest.mark.gpu
def test_quotient_work_bytes_through_the_binding(pkg, eng, poly):
    verifier = importlib.import_module(entry.PKG_NAME + ".verifier")
    from oracle import bn254 as O
    rng = random.Random(0xE52)

    def key(k, degree, n_perm, n_lookups):
        cs = Q.random_shape(rng, k, degree, n_perm, n_lookups, True)
        inputs = 3 + 2 + 1 + n_perm + cs.num_permutation_sets + 3 * n_lookups
        return verifier.VerifyingKey(eng, verifier.encode_vk(cs, O.aff_to_bytes)), inputs

    # either side of 2^24: k + e = 24 (one transform of 2^24 ends the call), 25 and 27 (the split ending: nothing above 2^k)
    for k, degree, n_perm, n_lookups in ((22, 4, 5, 2), (23, 4, 5, 2), (24, 9, 0, 1), (10, 3, 1, 0)):
        vk, inputs = key(k, degree, n_perm, n_lookups)
        assert eng.quotient_work_bytes(vk) == poly.quotient_work_bytes(eng, vk) == work_bytes(k, degree, inputs), (k, degree)
        vk.close()
    for k, degree in ((24, 34), (23, 66), (25, 3)):               # k + e = 30, 29; k above 24
        vk, _inputs = key(k, degree, 0, 0)
        with pytest.raises(pkg.H2AggError) as ei:
            eng.quotient_work_bytes(vk)
        assert ei.value.code == pkg.ERR_INVALID
        vk.close()
