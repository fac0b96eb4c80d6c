"""GPU: every lookup of a circuit in one call — h2agg_lookup_batch_permute / _batch_product, h2agg_lookup_store_permute /
_store_product, h2agg_lookup_configure, and poly.py over them.

Two yardsticks, both exact and compared byte for byte: the definition restated with Python integers
(tests/lookup_batch_ref.py over tests/lookup_permute_ref.py and tests/grand_product_ref.py), and the loop of single calls
(h2agg_lookup_permute / h2agg_lookup_product), which the existing suites hold against the same restatements."""
import ctypes as C
import importlib
import random

import pytest

import __graft_entry__ as entry
from tests.fr_bytes import dec, enc, fe
from tests.grand_product_ref import R, lookup_product_py
from tests.lookup_batch_ref import batch_permute_py, batch_product_py, chunk_split
from tests.lookup_permute_ref import compress_py, key_patterns, lookup_permute_py, loop_counts

pytestmark = pytest.mark.gpu

_pkg = entry.load_package()
FLAG_NONCANONICAL, FLAG_NOT_IN_TABLE = _pkg.LOOKUP_STATUS_NONCANONICAL, _pkg.LOOKUP_STATUS_NOT_IN_TABLE   # include/h2agg.h's names

T = 1 << 11
SMALL = (4, 5)                                            # the two smallest values of the debug key fr_sort_tile
BETA, GAMMA = 0x1234567 * 0x89ABCDEF0123 % R, (R - 0xFEDCBA987 * 0x13579BDF)
JUNK = (1 << 256) - 1                                     # a sentinel that is not canonical: never read, never written


@pytest.fixture(scope="module")
def poly(pkg):
    return importlib.import_module(entry.PKG_NAME + ".poly")


class key:
    """a debug key for the length of a with-block"""

    def __init__(self, eng, name, value):
        self.eng, self.name, self.value = eng, name, value

    def __enter__(self):
        self.eng.debug_configure(self.name, self.value)

    def __exit__(self, *exc):
        self.eng.debug_configure(self.name, 0)


class chunk:
    """h2agg_lookup_configure for the length of a with-block"""

    def __init__(self, eng, b):
        self.eng, self.b = eng, b

    def __enter__(self):
        self.eng.lookup_configure(self.b)

    def __exit__(self, *exc):
        self.eng.lookup_configure(0)


def drawn(seed, u):
    rng = random.Random(seed)
    s = [rng.randrange(R) for _ in range(u)]
    if u > 2:
        s[1] = s[0]
    return [s[rng.randrange(u)] for _ in range(u)], s


def slab(cols, n, u, above=JUNK):
    """columns of n rows: the first u of each column of cols, `above` from row u up"""
    return b"".join(enc(list(c[:u]) + [above] * (n - u)) for c in cols)


def check_permute(eng, a_cols, s_cols, k, u, what=None, singles=True):
    """the batch against the restatement and against the loop of single calls; rows from u up keep their sentinel"""
    n, count = 1 << k, len(a_cols)
    a, s = slab(a_cols, n, u), slab(s_cols, n, u)
    pre = enc([JUNK]) * (n * count)
    ap, sp, status = eng.lookup_batch_permute(a, s, count, k, u, pre, pre)
    want_ap, want_sp, want_status = batch_permute_py(a_cols, s_cols, u)
    assert status == want_status == [0] * count, what
    col = 32 * n
    for j in range(count):
        tail = enc([JUNK]) * (n - u)
        assert ap[col * j:col * (j + 1)] == enc(want_ap[j]) + tail, (what, j, u, "ap")
        assert sp[col * j:col * (j + 1)] == enc(want_sp[j]) + tail, (what, j, u, "sp")
        if singles:
            one = eng.lookup_permute(a[col * j:col * (j + 1)], s[col * j:col * (j + 1)], k, u)
            assert (ap[col * j:col * j + 32 * u], sp[col * j:col * j + 32 * u]) == one, (what, j, u, "single call")
    return ap, sp


# ---------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("u", [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5])
def test_permute_default_tile(eng, pkg, u):
    assert 1 << pkg.FR_SORT_TILE == T
    for count in (1, 2, 5):
        pairs = [drawn(0xC00 + 8 * u + j, u) for j in range(count)]
        check_permute(eng, [p[0] for p in pairs], [p[1] for p in pairs], 13, u, singles=count == 5)


@pytest.mark.parametrize("t", SMALL)
@pytest.mark.parametrize("u", [65, 513, 1023])
def test_permute_small_tiles(eng, t, u):
    """several tiles per column, ragged last tiles, the stepped scan and the strided histogram per column"""
    if u >= 513 or t == SMALL[0]:
        assert min(loop_counts(u, t)) >= 2
    pairs = [drawn(0xC10 + 16 * t + u + j, u) for j in range(3)]
    with key(eng, "fr_sort_tile", t):
        check_permute(eng, [p[0] for p in pairs], [p[1] for p in pairs], 10, u)


# ---------------------------------------------------------------------------------------------- diverging plans in one launch
def diverging(seed, k, u):
    """-> [(name, a, s)]: lookups whose sorts skip different passes, side by side in one chunk"""
    rng = random.Random(seed)
    n = 1 << k
    out = []
    s = [rng.randrange(1 << 16) for _ in range(u)]
    out.append(("16-bit table: 30 passes skipped", [s[rng.randrange(u)] for _ in range(u)], s))
    theta = rng.randrange(R)
    tables = [[rng.randrange(1 << 253, R) for _ in range(n)] for _ in range(3)]
    rows = [rng.randrange(u) for _ in range(n)]
    inputs = [[col[r] for r in rows] for col in tables]
    out.append(("theta-compressed 254-bit keys: none skipped", compress_py(inputs, theta)[:u], compress_py(tables, theta)[:u]))
    v = rng.randrange(R)
    out.append(("all keys equal: every pass skipped, the caller's column is the sorted one", [v] * u, [v] * u))
    s = [rng.randrange(R) for _ in range(u)]
    out.append(("an input that skips where its table moves", [s[u // 3]] * u, s))
    return out + key_patterns(seed + 1, u)


@pytest.mark.parametrize("t,k,u", [(SMALL[0], 7, 65), (0, 13, 3 * T + 5)], ids=["smallest-tile-65", "default-tile-3T+5"])
def test_diverging_plans_in_one_launch(eng, t, k, u):
    lookups = diverging(0xC20 + u, k, u)
    assert len(lookups) == 45
    with key(eng, "fr_sort_tile", t):
        check_permute(eng, [l[1] for l in lookups], [l[2] for l in lookups], k, u, [l[0] for l in lookups])


# ---------------------------------------------------------------------------------------------- chunks
def test_chunks_are_invisible(eng):
    k, u, count = 9, 300, 5
    pairs = [drawn(0xC30 + j, u) for j in range(count)]
    a_cols, s_cols = [p[0] for p in pairs], [p[1] for p in pairs]
    outs = []
    for forced in (1, 2, 3, 0):
        assert len(chunk_split(count, u, forced)) == {1: 5, 2: 3, 3: 2, 0: 1}[forced]
        with chunk(eng, forced):
            ap, sp = check_permute(eng, a_cols, s_cols, k, u, forced, singles=False)
            n = 1 << k
            z, last = eng.lookup_batch_product(slab(a_cols, n, u), slab(s_cols, n, u), ap, sp, count, k, u, fe(BETA), fe(GAMMA))
            assert last == [fe(1)] * count
            outs.append((ap, sp, z))
    assert outs[0] == outs[1] == outs[2] == outs[3]


def test_the_built_in_cap_of_1024_lookups_per_chunk(eng, pkg):
    k, u, count = 1, 1, 1025
    assert chunk_split(count, u) == [(0, 1024), (1024, 1)]
    assert eng.lookup_chunk_rule(u) == 1024 and eng.lookup_chunk_rule(0) == 1024   # the library's own rule, not its restatement
    a_cols = [[(j * 0x9E3779B97F4A7C15 + 5) % R, JUNK] for j in range(count)]
    ap, sp = check_permute(eng, a_cols, [list(c) for c in a_cols], k, u, singles=False)
    z, last = eng.lookup_batch_product(slab(a_cols, 2, u), slab(a_cols, 2, u), ap, sp, count, k, u, fe(BETA), fe(GAMMA),
                                       enc([JUNK]) * (2 * count))
    assert z == b"".join(fe(1) + fe(1) for _ in range(count)) and last == [fe(1)] * count
    with pytest.raises(pkg.H2AggError) as ei:
        eng.lookup_configure(1025)
    assert ei.value.code == pkg.ERR_INVALID
    eng.lookup_configure(1024)
    eng.lookup_configure(0)


# ---------------------------------------------------------------------------------------------- failures in one lookup only
@pytest.mark.parametrize("which,bit", [(1, FLAG_NOT_IN_TABLE), (2, FLAG_NONCANONICAL)], ids=["absent-head-in-1", "noncanonical-in-2"])
def test_a_failure_in_one_lookup_only(eng, pkg, poly, which, bit):
    k, u, count = 6, 50, 3
    n = 1 << k
    pairs = [drawn(0xC40 + j, u) for j in range(count)]
    a_cols, s_cols = [list(p[0]) for p in pairs], [list(p[1]) for p in pairs]
    good = batch_permute_py(a_cols, s_cols, u)
    if bit == FLAG_NOT_IN_TABLE:
        a_cols[which][7] = max(s_cols[which]) + 1 if max(s_cols[which]) + 1 < R else 3
        assert a_cols[which][7] not in s_cols[which]
        code = pkg.ERR_NOT_IN_TABLE
    else:
        assert s_cols[which][1] == s_cols[which][0]       # (a duplicate: every input value stays in the table)
        s_cols[which][1] = R
        code = pkg.ERR_NONCANONICAL
    want_status = [bit if j == which else 0 for j in range(count)]
    assert batch_permute_py(a_cols, s_cols, u)[2] == want_status
    a, s = slab(a_cols, n, u), slab(s_cols, n, u)
    col = 32 * n
    # the single call's code for the failing lookup
    with pytest.raises(pkg.H2AggError) as single:
        eng.lookup_permute(a[col * which:col * (which + 1)], s[col * which:col * (which + 1)], k, u)
    assert single.value.code == code
    with pytest.raises(pkg.H2AggError) as ei:
        eng.lookup_batch_permute(a, s, count, k, u)
    assert ei.value.code == code
    ap, sp, status = ei.value.partial
    assert status == want_status
    for j in range(count):
        if j != which:
            assert ap[col * j:col * j + 32 * u] == enc(good[0][j]) and sp[col * j:col * j + 32 * u] == enc(good[1][j]), j
    # the failing lookup in a later chunk (forced 1: chunk `which`; forced 2: lookup 2 opens the second chunk, lookup 1 is
    # the second word of the first): the words and the bytes are those of the one-chunk call
    for forced in (1, 2):
        assert len(chunk_split(count, u, forced)) == (3, 2)[forced - 1]
        with chunk(eng, forced):
            with pytest.raises(pkg.H2AggError) as ei:
                eng.lookup_batch_permute(a, s, count, k, u)
        assert ei.value.code == code and ei.value.partial[2] == want_status, forced
        for j in range(count):
            if j != which:
                lo, hi = col * j, col * j + 32 * u
                assert ei.value.partial[0][lo:hi] == ap[lo:hi] and ei.value.partial[1][lo:hi] == sp[lo:hi], (forced, j)
    # the context is usable afterwards
    check_permute(eng, [p[0] for p in pairs], [p[1] for p in pairs], k, u, singles=False)
    if bit == FLAG_NONCANONICAL:
        return                                            # (a store holds no element >= r: h2agg_columns_write refuses it)
    # the store forms: synchronous with the words; queued, the context's device status is raised once
    with poly.ColumnStore(eng, 4 * count, k) as st:
        st.write(0, slab(a_cols, n, u, 0))
        st.write(count, slab(s_cols, n, u, 0))
        v = [st.view(count * i, count) for i in range(4)]
        with pytest.raises(pkg.H2AggError) as ei:
            poly.resident_lookup_permute(eng, v[0], v[1], u, v[2], v[3])
        assert ei.value.code == code and ei.value.partial == want_status
        with chunk(eng, 1):
            with pytest.raises(pkg.H2AggError) as ei:
                poly.resident_lookup_permute(eng, v[0], v[1], u, v[2], v[3])
        assert ei.value.code == code and ei.value.partial == want_status
        got = st.read(2 * count, 2 * count)
        for j in range(count):
            if j != which:
                assert got[j][:32 * u] == enc(good[0][j]) and got[count + j][:32 * u] == enc(good[1][j]), j
        eng.synchronize()
        assert poly.resident_lookup_permute(eng, v[0], v[1], u, v[2], v[3], status=False) is None
        with pytest.raises(pkg.H2AggError) as ei:
            eng.synchronize()
        assert ei.value.code == code
        eng.synchronize()
    check_permute(eng, [p[0] for p in pairs], [p[1] for p in pairs], k, u, singles=False)


# ---------------------------------------------------------------------------------------------- product
def honest(seed, count, u, n):
    """-> (a, s, ap, sp) column lists of n rows (JUNK from row u up)"""
    pairs = [drawn(seed + j, u) for j in range(count)]
    a_cols, s_cols = [p[0] for p in pairs], [p[1] for p in pairs]
    perm = [lookup_permute_py(a, s, u) for a, s in pairs]
    return a_cols, s_cols, [p[0] for p in perm], [p[1] for p in perm]


def check_product(eng, cols, k, u, what=None, honest_pairs=True):
    n, count = 1 << k, len(cols[0])
    slabs = [slab(c, n, u) for c in cols]
    pre = enc([JUNK]) * (n * count)
    z, last = eng.lookup_batch_product(*slabs, count, k, u, fe(BETA), fe(GAMMA), pre)
    want, want_last = batch_product_py(*cols, u, BETA, GAMMA)
    col = 32 * n
    for j in range(count):
        assert z[col * j:col * (j + 1)] == enc(want[j]) + enc([JUNK]) * (n - u - 1), (what, j, u)
        assert last[j] == fe(want_last[j]), (what, j)
        if honest_pairs:
            assert want[j][0] == 1 and want_last[j] == 1
        one = eng.lookup_product(*[sl[col * j:col * (j + 1)] for sl in slabs], k, u, fe(BETA), fe(GAMMA))
        assert (z[col * j:col * j + 32 * (u + 1)], last[j]) == one, (what, j, "single call")
    return z


@pytest.mark.parametrize("count", [1, 3, 5])
def test_product_sizes(eng, count):
    k = 8
    n = 1 << k
    for u in (0, 1, n - 1):
        check_product(eng, honest(0xC50 + u, count, u, n), k, u)
    # three levels of the sweeps (chunks of 8 elements, more than 64 positions), u + 1 on both sides of a chunk multiple
    with key(eng, "fr_scan_chunk", 3):
        for u in (126, 127, 128):
            assert 64 < u + 1 <= 512 and 128 % 8 == 0
            check_product(eng, honest(0xC58 + u, count, u, n), k, u, "three levels")


def test_product_zero_denominator_in_one_column_only(eng):
    k, u, count = 7, 100, 3
    cols = honest(0xC60, count, u, 1 << k)
    cols[2][1] = list(cols[2][1])
    cols[2][1][40] = (R - BETA) % R                      # ap[40] + beta = 0 in lookup 1: inv(0) = 0, z is 0 from row 41 up
    z = check_product(eng, cols, k, u, "zero denominator", honest_pairs=False)
    col = 32 << k
    assert dec(z[col + 32 * 41:col + 32 * (u + 1)]) == [0] * (u - 40) and dec(z[col:col + 32 * 41])[-1] != 0
    assert z[32 * u:32 * (u + 1)] == fe(1) and z[2 * col + 32 * u:2 * col + 32 * (u + 1)] == fe(1)


# ---------------------------------------------------------------------------------------------- stores
def test_store_forms_equal_the_host_forms_in_one_store(eng, poly):
    """one store holds all five ranges, with a guard column between them; the rows above and the guards stay as they were (a
    canonical sentinel here: h2agg_columns_write takes no other)"""
    k, u, count = 8, 200, 3
    n = 1 << k
    a_cols, s_cols, ap_cols, sp_cols = honest(0xC70, count, u, n)
    a, s = slab(a_cols, n, u, R - 1), slab(s_cols, n, u, R - 1)
    fill = enc([R - 1]) * n
    ap, sp, status = eng.lookup_batch_permute(a, s, count, k, u, fill * count, fill * count)
    z, last = eng.lookup_batch_product(a, s, ap, sp, count, k, u, fe(BETA), fe(GAMMA), fill * count)
    assert status == [0] * count and last == [fe(1)] * count
    stride = count + 1
    with poly.ColumnStore(eng, 5 * stride, k) as st:
        st.write(0, fill * (5 * stride))
        v = [st.view(stride * i, count) for i in range(5)]
        v[0].write(a)
        v[1].write(s)
        for queued in (False, True):
            st.write(2 * stride, fill * (3 * stride))
            got_status = poly.resident_lookup_permute(eng, v[0], v[1], u, v[2], v[3], status=not queued)
            got_last = poly.resident_lookup_product(eng, v[0], v[1], v[2], v[3], u, fe(BETA), fe(GAMMA), v[4], last=not queued)
            if queued:
                assert got_status is None and got_last is None
                eng.synchronize()
            else:
                assert got_status == status and got_last == last
            assert b"".join(v[2].read()) == ap and b"".join(v[3].read()) == sp and b"".join(v[4].read()) == z
            assert b"".join(v[0].read()) == a and b"".join(v[1].read()) == s, "an input changed"
            for i in range(5):
                assert st.read(stride * i + count, 1) == [fill], ("guard column", i)


def test_refusals_leave_the_context_usable(eng, pkg, poly):
    lib, ctx = eng._lib, eng._ctx
    k, u, count = 5, 26, 2
    n = 1 << k
    cols = honest(0xC80, count, u, n)
    a, s, ap, sp = [slab(c, n, u, 0) for c in cols]
    want_z = eng.lookup_batch_product(a, s, ap, sp, count, k, u, fe(BETA), fe(GAMMA))

    def refused(code, fn, *args):
        with pytest.raises(pkg.H2AggError) as ei:
            fn(*args)
        assert ei.value.code == code, ei.value
        assert eng.lookup_batch_permute(a, s, count, k, u)[:2] == (ap, sp)

    raw = lambda rc: eng._check(rc)
    buf = [C.create_string_buffer(32 * n * count) for _ in range(5)]
    p = [C.cast(b, C.c_void_p) for b in buf]
    words = (C.c_uint32 * count)()
    b32, g32 = fe(BETA), fe(GAMMA)
    # the single calls' refusals
    refused(pkg.ERR_INVALID, lambda: raw(lib.h2agg_lookup_batch_permute(ctx, p[0], p[1], count, 25, u, p[2], p[3], words)))
    refused(pkg.ERR_INVALID, lambda: raw(lib.h2agg_lookup_batch_permute(ctx, p[0], p[1], count, k, n, p[2], p[3], words)))
    refused(pkg.ERR_INVALID, lambda: raw(lib.h2agg_lookup_batch_product(ctx, p[0], p[1], p[2], p[3], count, k, n, b32, g32, p[4], None)))
    for hole in range(4):
        args = list(p[:4])
        args[hole] = None
        refused(pkg.ERR_INVALID, lambda: raw(lib.h2agg_lookup_batch_permute(ctx, args[0], args[1], count, k, u, args[2], args[3], None)))
    for hole in range(5):
        args = list(p)
        args[hole] = None
        refused(pkg.ERR_INVALID, lambda: raw(lib.h2agg_lookup_batch_product(ctx, args[0], args[1], args[2], args[3], count, k, u, b32, g32,
                                                                           args[4], None)))
    for bad_b, bad_g in ((enc([R]), g32), (b32, enc([JUNK]))):
        refused(pkg.ERR_NONCANONICAL, eng.lookup_batch_product, a, s, ap, sp, count, k, u, bad_b, bad_g)
    # the batch's own: count, overlapping outputs
    for bad in (0, 65536):
        refused(pkg.ERR_INVALID, lambda: raw(lib.h2agg_lookup_batch_permute(ctx, p[0], p[1], bad, k, u, p[2], p[3], None)))
        refused(pkg.ERR_INVALID, lambda: raw(lib.h2agg_lookup_batch_product(ctx, p[0], p[1], p[2], p[3], bad, k, u, b32, g32, p[4], None)))
    for outs in ((p[0], p[3]), (p[2], p[1]), (p[2], p[2])):
        refused(pkg.ERR_INVALID, lambda: raw(lib.h2agg_lookup_batch_permute(ctx, p[0], p[1], count, k, u, outs[0], outs[1], None)))
    for hole in range(4):
        refused(pkg.ERR_INVALID, lambda: raw(lib.h2agg_lookup_batch_product(ctx, p[0], p[1], p[2], p[3], count, k, u, b32, g32, p[hole], None)))
    # the store family's
    with poly.ColumnStore(eng, 5 * count, k) as st, poly.ColumnStore(eng, count, k + 1) as other:
        st.write(0, a + s)
        h, o = st.handle, other.handle
        c = count
        permute = lambda *x: eng.lookup_store_permute(*x)
        product = lambda *x: eng.lookup_store_product(*x)
        good_pm = (h, 0, h, c, c, u, h, 2 * c, h, 3 * c)
        good_pr = (h, 0, h, c, h, 2 * c, h, 3 * c, c, u, b32, g32, h, 4 * c)

        def with_(args, at, value):
            args = list(args)
            args[at] = value
            return args

        for at in (0, 2, 6, 8):
            refused(pkg.ERR_INVALID, permute, *with_(good_pm, at, 0xDEAD))             # an unknown handle
            refused(pkg.ERR_INVALID, permute, *with_(good_pm, at, o))                  # a store of another k
            refused(pkg.ERR_INVALID, permute, *with_(good_pm, at + 1, 4 * c + 1))      # a range outside its store
        for at in (0, 2, 4, 6, 12):
            refused(pkg.ERR_INVALID, product, *with_(good_pr, at, 0xDEAD))
            refused(pkg.ERR_INVALID, product, *with_(good_pr, at, o))
            refused(pkg.ERR_INVALID, product, *with_(good_pr, at + 1, 4 * c + 1))
        for bad in (0, 65536):
            refused(pkg.ERR_INVALID, permute, *with_(good_pm, 4, bad))
            refused(pkg.ERR_INVALID, product, *with_(good_pr, 8, bad))
        refused(pkg.ERR_INVALID, permute, *with_(good_pm, 5, n))                       # u >= 2^k
        refused(pkg.ERR_INVALID, product, *with_(good_pr, 9, n))
        refused(pkg.ERR_NONCANONICAL, product, *with_(good_pr, 10, enc([R])))
        refused(pkg.ERR_NONCANONICAL, product, *with_(good_pr, 11, enc([R])))
        for ap_at, sp_at in ((c - 1, 3 * c), (2 * c - 1, 3 * c), (2 * c, 1), (2 * c, c + 1), (2 * c, 3 * c - 1)):
            refused(pkg.ERR_INVALID, permute, *with_(with_(good_pm, 7, ap_at), 9, sp_at))
        for z_at in (c - 1, 2 * c - 1, 3 * c - 1, 4 * c - 1):
            refused(pkg.ERR_INVALID, product, *with_(good_pr, 13, z_at))
        # nothing was written; adjacent ranges are fine
        assert b"".join(st.read(2 * c, 3 * c)) == bytes(32 * n * 3 * c)
        assert permute(*good_pm) == [0] * c
        assert product(*good_pr) == want_z[1]
        assert b"".join(st.read(2 * c, c)) == ap and b"".join(st.read(4 * c, c)) == want_z[0]


# ---------------------------------------------------------------------------------------------- phases
def test_phases_of_the_batch_calls(eng):
    k, u, count = 6, 50, 2
    cols = honest(0xC90, count, u, 1 << k)
    slabs = [slab(c, 1 << k, u, 0) for c in cols]
    with key(eng, "phases", 1):
        eng.lookup_batch_permute(slabs[0], slabs[1], count, k, u)
        assert [w.split("=")[0] for w in eng.last_phases().split()] == ["stage", "sort", "rank"]
        eng.lookup_batch_product(*slabs, count, k, u, fe(BETA), fe(GAMMA))
        assert [w.split("=")[0] for w in eng.last_phases().split()] == ["stage", "terms", "invert", "scan"]


# ---------------------------------------------------------------------------------------------- through the verifier
def test_lookup_arguments_satisfy_the_verifiers_identity(eng, poly):
    """poly.lookup_arguments on three three-column lookups at k = 7: Z, ap and sp against lookup.rs:98-113, row by row"""
    k = 7
    n, u = 1 << k, (1 << k) - 6
    rng = random.Random(0xCA0)
    theta = rng.randrange(R)
    inputs, tables = [], []
    for j in range(3):
        tab = [[rng.randrange(R) for _ in range(n)] for _ in range(3)]
        rows = [rng.randrange(u) for _ in range(n)]
        tables.append(tab)
        inputs.append([[col[r] for r in rows] for col in tab])
    blind = ([enc([0xD000 + 16 * j + i for i in range(n - u)]) for j in range(3)],
             [enc([0xE000 + 16 * j + i for i in range(n - u)]) for j in range(3)],
             [enc([0xF000 + 16 * j + i for i in range(n - u - 1)]) for j in range(3)])
    as_bytes = lambda lookups: [[enc(c) for c in cols] for cols in lookups]
    aps, sps, zs = poly.lookup_arguments(eng, as_bytes(inputs), as_bytes(tables), k, u, fe(theta), fe(BETA), fe(GAMMA), blinding=blind)
    for j in range(3):
        assert aps[j][32 * u:] == blind[0][j] and sps[j][32 * u:] == blind[1][j] and zs[j][32 * (u + 1):] == blind[2][j]
        one = poly.lookup_argument(eng, [enc(c) for c in inputs[j]], [enc(c) for c in tables[j]], k, u, fe(theta), fe(BETA), fe(GAMMA),
                                   blinding=(blind[0][j], blind[1][j], blind[2][j]))
        assert one == (aps[j], sps[j], zs[j]), j
        ap, sp, z = dec(aps[j]), dec(sps[j]), dec(zs[j])
        a, s = compress_py(inputs[j], theta), compress_py(tables[j], theta)
        assert z[0] == 1 and z[u] == 1                                                 # lookup.rs:98-105
        for i in range(u):                                                             # lookup.rs:106-113
            assert z[i + 1] * (ap[i] + BETA) % R * (sp[i] + GAMMA) % R == z[i] * (a[i] + BETA) % R * (s[i] + GAMMA) % R, (j, i)
            assert ap[i] == sp[i] or (i and ap[i] == ap[i - 1]), (j, i)                # :114-119
        assert ap[0] == sp[0]
    bare = poly.lookup_arguments(eng, as_bytes(inputs), as_bytes(tables), k, u, fe(theta), fe(BETA), fe(GAMMA))
    assert bare[0][1][32 * u:] == bytes(32 * (n - u)) and bare[2][2][:32 * (u + 1)] == zs[2][:32 * (u + 1)]
