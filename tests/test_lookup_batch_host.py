"""CPU: the batched lookup entry points — h2agg_lookup_batch_permute / _batch_product, h2agg_lookup_store_permute /
_store_product, h2agg_lookup_configure — in the header, the library, the binding and poly.py; the chunk rule of
csrc/lookup.inc recomputed by hand; and the restatement (tests/lookup_batch_ref.py) against the conditions the reference's
verifier checks (halo2-snark-aggregator-api/src/systems/halo2/lookup.rs:98-113), lookup by lookup."""
import ctypes
import importlib
import os
import random
import re
from collections import Counter

import pytest

import __graft_entry__ as entry
from tests.grand_product_ref import R
from tests.lookup_batch_ref import (BATCH_MAX, BATCH_ROWS, FLAG_NONCANONICAL, FLAG_NOT_IN_TABLE, MAX_LOOKUPS, batch_chunk,
                                    batch_permute_py, batch_product_py, chunk_split, first_failure)

NEW_SYMBOLS = ["h2agg_lookup_batch_permute", "h2agg_lookup_batch_product", "h2agg_lookup_store_permute",
               "h2agg_lookup_store_product", "h2agg_lookup_configure", "h2agg_lookup_chunk_rule"]
BETA, GAMMA = 0x2468ACE * 0x7654321 % R, 0x1B2D3F * 0xFFFFFFFB % R


def test_the_entry_points_exist(pkg):
    header = re.sub(r"/\*.*?\*/", "", open(pkg.HEADER_PATH).read(), flags=re.S)
    lib = ctypes.CDLL(pkg.LIB_PATH)
    names = set(pkg.exported_symbols())
    for fn in NEW_SYMBOLS:
        assert re.search(r"\b(?:int|size_t)\s+%s\s*\(" % fn, header), fn
        assert hasattr(lib, fn), fn
        assert fn in names and getattr(pkg.load_library(), fn).argtypes is not None, fn
    for method in ("lookup_batch_permute", "lookup_batch_product", "lookup_store_permute", "lookup_store_product", "lookup_configure",
                   "lookup_chunk_rule"):
        assert callable(getattr(pkg.H2Agg, method)), method
    poly = importlib.import_module(entry.PKG_NAME + ".poly")
    for fn in ("permute_expression_pairs", "lookup_products", "lookup_arguments", "resident_lookup_permute", "resident_lookup_product",
               "lookup_argument"):
        assert callable(getattr(poly, fn)), fn


def test_the_status_bits_are_named_once(pkg):
    """the header's two constants, the package's, the restatement's and the kernels' are one pair of values"""
    text = open(pkg.HEADER_PATH).read()
    named = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define H2AGG_LOOKUP_STATUS_(\w+) (\d+)u", text)}
    assert named == {"NONCANONICAL": 1, "NOT_IN_TABLE": 8}
    assert (pkg.LOOKUP_STATUS_NONCANONICAL, pkg.LOOKUP_STATUS_NOT_IN_TABLE) == (FLAG_NONCANONICAL, FLAG_NOT_IN_TABLE) == (1, 8)
    csrc = os.path.join(os.path.dirname(pkg.LIB_PATH), "csrc")
    assert re.search(r"FLAG_NONCANONICAL = 1u\b", open(os.path.join(csrc, "batch_kernels.hpp")).read())
    assert re.search(r"FLAG_NOT_IN_TABLE = 8u\b", open(os.path.join(csrc, "lookup_kernels.hpp")).read())
    assert "static_assert(H2AGG_LOOKUP_STATUS_NONCANONICAL == FLAG_NONCANONICAL" in open(os.path.join(csrc, "lookup.inc")).read()
    # the prose of the header's block gives the same two values
    assert "H2AGG_LOOKUP_STATUS_NONCANONICAL (1)" in text and "H2AGG_LOOKUP_STATUS_NOT_IN_TABLE (8)" in text


def test_no_new_name_claims_the_device_or_the_store_family():
    for fn in NEW_SYMBOLS:
        assert not re.search(r"_device|_async", fn) and not fn.startswith("h2agg_columns_"), fn


def test_the_signatures_are_the_headers(pkg):
    """the argument counts of the binding against the declarations"""
    header = re.sub(r"/\*.*?\*/", "", open(pkg.HEADER_PATH).read(), flags=re.S)
    lib = pkg.load_library()
    for fn in NEW_SYMBOLS:
        args = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*)\)\s*;" % fn, header).group(1)
        assert len(getattr(lib, fn).argtypes) == args.count(",") + 1, fn


def test_chunk_rule_by_hand(pkg):
    src = open(os.path.join(os.path.dirname(pkg.LIB_PATH), "csrc", "lookup.inc")).read()
    assert re.search(r"LK_BATCH_ROWS = \(size_t\)1 << (\d+);", src).group(1) == "24" and BATCH_ROWS == 1 << 24
    assert int(re.search(r"LK_BATCH_MAX = (\d+);", src).group(1)) == BATCH_MAX == 1024
    assert int(re.search(r"LK_MAX_LOOKUPS = (\d+);", src).group(1)) == MAX_LOOKUPS == 65535
    # B(u, forced) at the edges: no rows, one row, the last u that still gets 1024 lookups, the first that does not, the largest u
    by_hand = {0: 1024, 1: 1024, 1 << 14: 1024, (1 << 14) + 1: 1023, (1 << 24) - 1: 1}
    for u, want in by_hand.items():
        assert batch_chunk(u) == want, u
        assert batch_chunk(u) * max(u, 1) <= 1 << 24
        assert pkg.H2Agg.lookup_chunk_rule(u) == want, u          # the library's own arithmetic (host code, no context)
        for forced, forced_want in ((1, 1), (2, min(2, want)), (3, min(3, want)), (1024, want), (0, want)):
            assert batch_chunk(u, forced) == forced_want, (u, forced)
            assert pkg.H2Agg.lookup_chunk_rule(u, forced) == forced_want, (u, forced)
    assert (1 << 24) // ((1 << 14) + 1) == 1023 and 1024 * ((1 << 14) + 1) > 1 << 24
    # 2 B sort columns stay inside a grid's second dimension; the histograms of a chunk: 2 B x 32 x 256 words = 64 MiB
    assert 2 * BATCH_MAX <= 65535 and 2 * BATCH_MAX * 32 * 256 * 4 == 64 << 20
    assert chunk_split(5, 100, 2) == [(0, 2), (2, 2), (4, 1)] and chunk_split(5, 100) == [(0, 5)]
    assert chunk_split(1025, 1) == [(0, 1024), (1024, 1)]
    assert chunk_split(3, (1 << 24) - 1) == [(0, 1), (1, 1), (2, 1)]


def three_lookups(seed, u, n):
    rng = random.Random(seed)
    a_cols, s_cols = [], []
    for j, below in enumerate((7, 1 << 16, R)):
        s = [rng.randrange(below) for _ in range(n)]
        a_cols.append([s[rng.randrange(u)] for _ in range(u)] + [rng.randrange(below) for _ in range(n - u)])
        s_cols.append(s)
    return a_cols, s_cols


@pytest.mark.parametrize("u", [1, 2, 29, 64, 100])
def test_restatement_satisfies_the_verifiers_conditions_per_lookup(u):
    n = u + 3
    a_cols, s_cols = three_lookups(0xB00 + u, u, n)
    aps, sps, status = batch_permute_py(a_cols, s_cols, u)
    assert status == [0, 0, 0] and first_failure(status) == 0
    zs, last = batch_product_py(a_cols, s_cols, aps, sps, u, BETA, GAMMA)
    assert last == [1, 1, 1]
    for a, s, ap, sp, z in zip(a_cols, s_cols, aps, sps, zs):
        assert Counter(ap) == Counter(a[:u]) and Counter(sp) == Counter(s[:u]) and ap == sorted(a[:u])
        assert z[0] == 1 and z[u] == 1 and len(z) == u + 1                           # lookup.rs:98-105
        assert ap[0] == sp[0]
        for i in range(u):                                                           # lookup.rs:106-119
            assert z[i + 1] * (ap[i] + BETA) % R * (sp[i] + GAMMA) % R == z[i] * (a[i] + BETA) % R * (s[i] + GAMMA) % R
            assert ap[i] == sp[i] or (i and ap[i] == ap[i - 1])


def test_status_words_of_the_restatement():
    u, n = 20, 23
    a_cols, s_cols = three_lookups(0xB10, u, n)
    absent = max(s_cols[1]) + 1
    a_cols[1][4] = absent
    a_cols[2][u] = R                                      # above the usable rows: not read
    aps, sps, status = batch_permute_py(a_cols, s_cols, u)
    assert status == [0, FLAG_NOT_IN_TABLE, 0] and aps[1] is None and aps[0] and aps[2]
    s_cols[0][3] = R + 5
    status = batch_permute_py(a_cols, s_cols, u)[2]
    assert status[0] & FLAG_NONCANONICAL and status[1] == FLAG_NOT_IN_TABLE and first_failure(status) == status[0]
    assert batch_permute_py([[1, 2]], [[3, 4]], 0) == ([[]], [[]], [0])
