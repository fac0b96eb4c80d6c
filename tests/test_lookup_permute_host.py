"""CPU: the Python yardstick of the lookup-permutation tests (tests/lookup_permute_ref.py) against the conditions the
reference's verifier checks (halo2-snark-aggregator-api/src/systems/halo2/lookup.rs:98-113, row by row), the restatement of
the device's sort and rank arithmetic against sorted() and the definition, and the four entry points in the header, the
library and the binding."""
import ctypes
import importlib
import os
import random
import re
from collections import Counter

import pytest

import __graft_entry__ as entry
from tests.grand_product_ref import BIG, R, lookup_product_py
from tests.lookup_permute_ref import (NotInTable, compress_py, digit_hist_py, geometry, key_patterns, lookup_permute_py,
                                      loop_counts, only_byte, permute_model_py, prefix_py, radix_sort_py, scan_row_py)

NEW_SYMBOLS = ["h2agg_lookup_permute", "h2agg_fr_columns_compress"]
NEW_SYMBOLS += [s + "_device" for s in NEW_SYMBOLS]
BETA, GAMMA = 0x2468ACE * 0x7654321 % R, 0x1B2D3F * 0xFFFFFFFB % R


def check_pair(a, s, ap, sp, u):
    assert len(ap) == u and len(sp) == u
    assert Counter(ap) == Counter(a[:u]) and Counter(sp) == Counter(s[:u])          # permutations: what makes z[u] = 1
    if u:
        assert ap[0] == sp[0]
    for i in range(1, u):
        assert ap[i] == sp[i] or ap[i] == ap[i - 1], i
    assert ap == sorted(a[:u])


def drawn(seed, u, below):
    rng = random.Random(seed)
    n = u + 3
    s = [rng.randrange(below) for _ in range(n)]
    a = [s[rng.randrange(u)] for _ in range(u)] + [rng.randrange(below) for _ in range(n - u)]
    return a, s


@pytest.mark.parametrize("below", [7, R], ids=["small", "254-bit"])
def test_restatement_satisfies_the_verifiers_conditions(below):
    for u in list(range(0, 40)) + [63, 64, 65, 127, 200, 300]:
        a, s = drawn(0x900 + u, u, below) if u else ([1, 2, 3], [4, 5, 6])
        ap, sp = lookup_permute_py(a, s, u)
        check_pair(a, s, ap, sp, u)
        z = lookup_product_py(a, s, ap, sp, u, BETA, GAMMA)
        assert z[0] == 1 and z[u] == 1, u                                            # lookup.rs:98-105
        for i in range(u):                                                           # lookup.rs:106-113
            assert z[i + 1] * (ap[i] + BETA) % R * (sp[i] + GAMMA) % R == z[i] * (a[i] + BETA) % R * (s[i] + GAMMA) % R


def test_leftover_rule_on_a_hand_written_example():
    """8 rows.  a sorted: 3 3 3 5 5 5 5 9 -> heads at rows 0, 3, 7; the table gives 3, 5, 9 to them and keeps 2, 7, 7, 8, 11:
    ascending, they go to the non-head rows 6, 5, 4, 2, 1 in that order (highest row first)."""
    a = [5, 3, 9, 5, 3, 5, 3, 5]
    s = [7, 11, 3, 2, 9, 7, 5, 8]
    ap, sp = lookup_permute_py(a, s, 8)
    assert ap == [3, 3, 3, 5, 5, 5, 5, 9]
    assert sp == [3, 11, 8, 5, 7, 7, 2, 9]
    check_pair(a, s, ap, sp, 8)
    # rows from u up are not read: the same pair from longer columns
    assert lookup_permute_py(a + [1], s + [1], 8) == (ap, sp)


def test_a_value_only_above_the_usable_rows_counts_as_absent():
    a, s = [4, 6, 4, 6, 0], [4, 9, 9, 1, 6]
    with pytest.raises(NotInTable):
        lookup_permute_py(a, s, 4)                       # 6 sits in s at row 4 only
    assert lookup_permute_py([4, 6, 4, 6, 9], s, 5)[0] == [4, 4, 6, 6, 9]   # ... and is found once row 4 is usable
    for absent in (0, 5, 10):                            # below, between and above the table's values
        with pytest.raises(NotInTable):
            lookup_permute_py([4, absent, 9, 1], [4, 9, 9, 1], 4)
    assert lookup_permute_py([], [], 0) == ([], [])


def test_compress_restatement():
    cols = [[1, 2], [3, 4], [5, 6]]
    assert compress_py(cols, 10) == [135, 246]            # the first column under theta^2
    assert compress_py(cols, 0) == [5, 6] and compress_py(cols, 1) == [9, 12]
    assert compress_py([[R - 1]], BIG) == [R - 1]


# ---------------------------------------------------------------------------------------------- the device's arithmetic
@pytest.mark.parametrize("t,u", [(4, 1), (4, 2), (4, 15), (4, 16), (4, 17), (4, 65), (5, 63), (5, 64), (5, 65), (5, 513), (8, 700),
                                 (9, 257), (11, 2049)])
def test_offset_arithmetic_of_the_sort_against_sorted(t, u):
    """every store position of every pass is inside [0, u) and hit once (asserted inside radix_sort_py), and the result is
    sorted(); passes whose byte is the same in every key move nothing"""
    rng = random.Random(0x910 + 64 * t + u)
    cases = {
        "random": ([rng.randrange(R) for _ in range(u)], None),
        "16-bit": ([rng.randrange(1 << 16) for _ in range(u)], 2),
        "byte 31": (only_byte(7, 31, u), 1),
        "byte 13": (only_byte(8, 13, u), 1),
        "equal": ([BIG] * u, 0),
        "specials": (([0, 1, R - 1, BIG] * u)[:u], None),
    }
    for name, (keys, max_moves) in cases.items():
        got, moved, state = radix_sort_py(keys, t)
        assert got == sorted(keys), name
        if max_moves is not None:
            assert len(moved) <= max_moves, (name, moved)
        if u == 1 or name == "equal":
            assert moved == [] and state == 0, name      # the caller's column is the sorted one
        if name == "byte 13" and u > 1:
            assert moved == [13]
        if name == "random" and u >= 513:
            assert len(moved) == 32


@pytest.mark.parametrize("t,n", [(4, 1), (4, 16), (4, 17), (4, 100), (11, 2048), (11, 2049), (11, 5000)])
def test_prefix_sums_of_the_rank_step(t, n):
    rng = random.Random(0x920 + n)
    flags = [rng.randrange(2) for _ in range(n)]
    assert prefix_py(flags, t) == [sum(flags[:i]) for i in range(n + 1)]


def test_the_debug_tile_reaches_the_step_and_stride_loops_below_1024_rows():
    """at the default tile the scan takes a second step from 2^19 rows (count matrix) and 2^21 rows (tile sums) up, the byte
    histogram a second stride from 2^18 rows up; under the debug key the geometry shrinks with the tile, so the sizes the GPU
    tests run at the two smallest tiles walk all three loops at least twice"""
    assert geometry(11) == (1024, 256, 1024)
    assert loop_counts((1 << 13) - 1, 11) == (1, 1, 1)
    assert loop_counts((1 << 20) - 6, 11) == (2, 1, 4) and loop_counts((1 << 22) - 6, 11) == (8, 2, 16)
    assert geometry(4) == (4, 4, 2) and geometry(5) == (8, 8, 2) and geometry(10) == (256, 256, 2)
    assert loop_counts(65, 4) == (5, 2, 9)
    for t, u in [(4, 65), (4, 513), (4, 1000), (4, 1023), (5, 513), (5, 1000), (5, 1023)]:
        assert min(loop_counts(u, t)) >= 2, (t, u)


@pytest.mark.parametrize("step,ncols", [(4, 1), (4, 4), (4, 5), (4, 20), (8, 17), (256, 700), (1024, 1024), (1024, 1025), (1024, 2500)])
def test_stepped_scan_of_a_row(step, ncols):
    """k_lk_scan_rows restated: the carry from step to step, a ragged last step, the default step of 1024 entries over rows of
    one, two and three steps"""
    rng = random.Random(0x940 + step + ncols)
    row = [rng.randrange(5) for _ in range(ncols)]
    base = rng.randrange(1000)
    assert scan_row_py(list(row), step, base) == [base + sum(row[:i]) for i in range(ncols)]


@pytest.mark.parametrize("t,u", [(4, 1), (4, 8), (4, 9), (4, 65), (5, 100), (10, 513), (11, 300)])
def test_strided_byte_histogram(t, u):
    """k_lk_digit_hist restated: every key counted once (asserted inside) whatever the grid and the lanes that take keys"""
    rng = random.Random(0x950 + u)
    keys = [rng.randrange(R) for _ in range(u)]
    hist = digit_hist_py(keys, t)
    for p in (0, 13, 31):
        want = Counter((x >> (8 * p)) & 0xFF for x in keys)
        assert hist[p] == [want[d] for d in range(256)]


@pytest.mark.parametrize("t,u", [(4, 65), (5, 65), (5, 200), (11, 300)])
def test_device_route_equals_the_definition(t, u):
    for name, a, s in key_patterns(0x930 + u, u):
        if name.startswith("byte") and int(name.split()[1]) % 8:
            continue                                      # (bytes 0, 8, 16, 24 here; the GPU test runs all 32)
        ap, sp, absent = permute_model_py(a, s, u, t)
        assert not absent and (ap, sp) == lookup_permute_py(a, s, u), name
    a, s = [4, 6, 4, 6] * 20, [4, 9, 9, 1] * 20
    assert permute_model_py(a, s, 80, t)[2]                # an absent head raises the flag; every index stayed in range


# ---------------------------------------------------------------------------------------------- header, library, binding
def test_the_entry_points_exist(pkg):
    header = re.sub(r"/\*.*?\*/", "", open(pkg.HEADER_PATH).read(), flags=re.S)
    lib = ctypes.CDLL(pkg.LIB_PATH)
    names = set(pkg.exported_symbols())
    for fn in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % fn, header), fn
        assert hasattr(lib, fn), fn
        assert fn in names and getattr(pkg.load_library(), fn).argtypes is not None, fn
    assert pkg.ERR_NOT_IN_TABLE == 9 and re.search(r"H2AGG_ERR_NOT_IN_TABLE = 9\b", header)
    for method in ("lookup_permute", "fr_columns_compress"):
        assert callable(getattr(pkg.H2Agg, method)) and callable(getattr(pkg.H2Agg, method + "_device")), method
    assert "fr_sort_tile" in open(pkg.HEADER_PATH).read()
    assert pkg.FR_SORT_TILE == 11 and pkg.FR_SORT_TILE_MIN == 4
    kernels = open(os.path.join(os.path.dirname(pkg.LIB_PATH), "csrc", "lookup_kernels.hpp")).read()
    assert int(re.search(r"LK_TILE_LOG = (\d+);", kernels).group(1)) == pkg.FR_SORT_TILE
    assert int(re.search(r"LK_TILE_LOG_MIN = (\d+);", kernels).group(1)) == pkg.FR_SORT_TILE_MIN
    poly = importlib.import_module(entry.PKG_NAME + ".poly")
    for fn in ("compress_expressions", "permute_expression_pair", "lookup_argument"):
        assert callable(getattr(poly, fn)), fn
