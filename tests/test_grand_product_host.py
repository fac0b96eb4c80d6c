"""CPU: the Python yardstick of the grand-product tests (tests/grand_product_ref.py) against the identities the reference's
verifier checks — halo2-snark-aggregator-api/src/systems/halo2/permutation.rs:70-133 and lookup.rs:98-113, evaluated row by
row on the domain instead of at one point x — and the eight entry points in the header, the library and the binding."""
import ctypes
import importlib
import re

import pytest

import __graft_entry__ as entry
from tests.grand_product_ref import (DELTA, R, batch_invert_py, grand_product_py, lookup_product_py, omega, permutation_chain_py,
                                     permuted_pair, satisfied_permutation)

NEW_SYMBOLS = ["h2agg_fr_batch_invert", "h2agg_fr_grand_product", "h2agg_permutation_product", "h2agg_lookup_product"]
NEW_SYMBOLS += [s + "_device" for s in NEW_SYMBOLS]


def test_batch_invert_and_grand_product_restatements():
    xs = [0, 1, R - 1, 5, 0, 7]
    inv = batch_invert_py(xs)
    assert [x * y % R for x, y in zip(xs, inv)] == [0, 1, 1, 1, 0, 1]
    assert grand_product_py([2, 3, 4], None, 3, 5) == [5, 10, 30, 120]
    assert grand_product_py([2, 3, 4], [2, 0, 4], 3, 1) == [1, 1, 0, 0]          # inv(0) = 0: everything behind it is 0
    assert grand_product_py([2, 3, 4], [2, 3, 4], 0, 9) == [9]


def test_permutation_chain_satisfies_the_verifiers_identities():
    """k = 4, m = 5 columns in three sets (chunk_len = 2), u = n - 6"""
    k, m, c = 4, 5, 2
    n, u, w = 1 << k, (1 << k) - 6, omega(k)
    beta, gamma = 0x1234567 * 0x89ABCDEF % R, 0xFEDCBA987 * 0x13579BDF % R
    values, sigmas = satisfied_permutation(0x6A0, k, m, u)
    zs = permutation_chain_py(values, sigmas, k, u, beta, gamma, DELTA, c)
    assert len(zs) == 3 and all(len(z) == u + 1 for z in zs)
    assert zs[0][0] == 1                                               # l_0 (1 - z_0)                       permutation.rs:70-78
    assert zs[-1][u] == 1 and (zs[-1][u] ** 2 - zs[-1][u]) % R == 0     # l_last (z^2 - z) on the last set     :79-85
    for s in range(1, 3):
        assert zs[s][0] == zs[s - 1][u]                                # l_0 (z_i - z_{i-1}(w^last X))        :86-93
    for s, z in enumerate(zs):                                         # the row identity                     :94-133
        for i in range(u):
            left, right = z[i + 1], z[i]
            d = beta * pow(w, i, R) % R * pow(DELTA, s * c, R) % R     # t0 * delta^(chunk_index * chunk_len) at X = w^i
            for j in range(s * c, min(m, s * c + c)):
                t2 = (values[j][i] + gamma) % R
                left = (t2 + beta * sigmas[j][i]) % R * left % R
                right = (t2 + d) % R * right % R
                d = DELTA * d % R
            assert left == right, (s, i)
    # an unsatisfied assignment does not end at 1
    values[3][2] = (values[3][2] + 1) % R
    assert permutation_chain_py(values, sigmas, k, u, beta, gamma, DELTA, c)[-1][u] != 1


def test_lookup_product_satisfies_the_verifiers_identity():
    k = 4
    u = (1 << k) - 6
    beta, gamma = 0x2468ACE * 0x7654321 % R, 0x1B2D3F * 0xFFFFFFFB % R
    a, s, ap, sp = permuted_pair(0x6A1, k, u)
    z = lookup_product_py(a, s, ap, sp, u, beta, gamma)
    assert z[0] == 1 and z[u] == 1 and len(z) == u + 1                  # l_0 (1 - z), l_last (z^2 - z)        lookup.rs:98-105
    for i in range(u):                                                 # lookup.rs:106-113
        assert z[i + 1] * (ap[i] + beta) % R * (sp[i] + gamma) % R == z[i] * (a[i] + beta) % R * (s[i] + gamma) % R
        assert ap[i] == sp[i] or ap[i] == ap[i - 1]                    # (what permute_expression_pair promises: :114-119)
    assert ap[0] == sp[0]


def test_the_entry_points_exist(pkg):
    header = re.sub(r"/\*.*?\*/", "", open(pkg.HEADER_PATH).read(), flags=re.S)
    lib = ctypes.CDLL(pkg.LIB_PATH)
    names = set(pkg.exported_symbols())
    for fn in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % fn, header), fn
        assert hasattr(lib, fn), fn
        assert fn in names and getattr(pkg.load_library(), fn).argtypes is not None, fn
    for method in ("fr_batch_invert", "fr_grand_product", "permutation_product", "lookup_product"):
        assert callable(getattr(pkg.H2Agg, method)) and callable(getattr(pkg.H2Agg, method + "_device")), method
    assert "fr_scan_chunk" in open(pkg.HEADER_PATH).read()
    assert pkg.FR_SCAN_CHUNK == 11
    poly = importlib.import_module(entry.PKG_NAME + ".poly")
    for fn in ("batch_invert", "permutation_products", "lookup_product"):
        assert callable(getattr(poly, fn)), fn
