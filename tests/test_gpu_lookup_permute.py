"""GPU: the lookup argument in front of its grand product — h2agg_lookup_permute, h2agg_fr_columns_compress, their _device
twins, and poly.py over them.

halo2_proofs is not vendored in the reference, so the yardstick is the definition in include/h2agg.h, restated with Python
integers in tests/lookup_permute_ref.py, which tests/test_lookup_permute_host.py ties to the conditions the reference's
verifier checks (lookup.rs:98-113).  Everything is exact and compared byte for byte."""
import ctypes as C
import importlib
import random

import pytest

import __graft_entry__ as entry
from tests.fr_bytes import dec, enc, fe
from tests.grand_product_ref import BIG, R, lookup_product_py
from tests.lookup_permute_ref import compress_py, key_patterns, lookup_permute_py, loop_counts

pytestmark = pytest.mark.gpu

T = 1 << 11
SMALL = (4, 5)                                            # the two smallest values of the debug key fr_sort_tile
BETA, GAMMA = 0x1234567 * 0x89ABCDEF0123 % R, (R - 0xFEDCBA987 * 0x13579BDF)
JUNK = (1 << 256) - 1                                     # in the rows from u up: not canonical, not in any table — never read


@pytest.fixture(scope="module")
def poly(pkg):
    return importlib.import_module(entry.PKG_NAME + ".poly")


class tile:
    """the debug key fr_sort_tile for the length of a with-block"""

    def __init__(self, eng, t):
        self.eng, self.t = eng, t

    def __enter__(self):
        self.eng.debug_configure("fr_sort_tile", self.t)

    def __exit__(self, *exc):
        self.eng.debug_configure("fr_sort_tile", 0)


def check(eng, a, s, k, u, what=None):
    """a, s: u rows; the columns handed over have 2^k rows, JUNK above u"""
    n = 1 << k
    want = lookup_permute_py(a, s, u)
    got = eng.lookup_permute(enc(a[:u] + [JUNK] * (n - u)), enc(s[:u] + [JUNK] * (n - u)), k, u)
    assert got[0] == enc(want[0]), (what, u, "ap")
    assert got[1] == enc(want[1]), (what, u, "sp")


def drawn(seed, u):
    rng = random.Random(seed)
    s = [rng.randrange(R) for _ in range(u)]
    if u > 2:
        s[1] = s[0]
    return [s[rng.randrange(u)] for _ in range(u)], s


# ---------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("u", [0, 1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5, (1 << 13) - 1])
def test_permute_default_tile(eng, pkg, u):
    assert 1 << pkg.FR_SORT_TILE == T
    check(eng, *drawn(0xA00 + u, u), 13, u)


@pytest.mark.parametrize("t", SMALL)
@pytest.mark.parametrize("u", [63, 64, 65, 513, 1000, 1023])
def test_permute_small_tiles(eng, pkg, t, u):
    assert SMALL[0] == pkg.FR_SORT_TILE_MIN
    if u >= 513 or (t, u) == (SMALL[0], 65):
        # the step loop of k_lk_scan_rows (count matrix, tile sums) and the stride loop of k_lk_digit_hist all go round again
        assert min(loop_counts(u, t)) >= 2
    with tile(eng, t):
        check(eng, *drawn(0xA10 + 16 * t + u, u), 10, u)


# ---------------------------------------------------------------------------------------------- key patterns
@pytest.mark.parametrize("t,k,u", [(SMALL[0], 7, 65), (0, 13, 3 * T + 5)], ids=["smallest-tile-65", "default-tile-3T+5"])
def test_permute_key_patterns(eng, t, k, u):
    names = []
    assert loop_counts(u, t or 11) == ((5, 2, 9) if t else (1, 1, 1))
    with tile(eng, t):
        for name, a, s in key_patterns(0xA20 + u, u):
            check(eng, a, s, k, u, name)
            names.append(name)
    assert sum(n.startswith("byte") for n in names) == 32 and len(names) == 41


# ---------------------------------------------------------------------------------------------- refusals
def test_permute_refusals_leave_the_context_usable(eng, pkg):
    import torch
    dev = torch.device("cuda:0")
    lib, ctx = eng._lib, eng._ctx
    k, u, n = 5, 26, 32
    a, s = drawn(0xA30, u)
    good = lookup_permute_py(a, s, u)

    def still_works():
        assert eng.lookup_permute(enc(a), enc(s), k, u) == (enc(good[0]), enc(good[1]))

    def refused(code, fn, *args):
        with pytest.raises(pkg.H2AggError) as ei:
            fn(*args)
        assert ei.value.code == code, ei.value
        still_works()

    srt = sorted(set(s))
    lo, mid, hi = srt[0], srt[len(srt) // 2], srt[-1]
    assert lo > 0 and hi < R - 1
    for absent in (lo - 1, mid + 1, hi + 1):              # a head that is the smallest, a middle and the largest key
        assert absent not in s
        b = list(a)
        b[7] = absent
        refused(pkg.ERR_NOT_IN_TABLE, eng.lookup_permute, enc(b), enc(s), k, u)
    only_above = 0x5EED
    b = list(a)
    b[3] = only_above                                     # present in the table, but only at a row >= u
    refused(pkg.ERR_NOT_IN_TABLE, eng.lookup_permute, enc(b + [0] * (n - u)), enc(s + [only_above] * (n - u)), k, u)
    for bad in (R, JUNK):                                 # an element >= r, in a and in s
        b = list(a)
        b[5] = bad
        refused(pkg.ERR_NONCANONICAL, eng.lookup_permute, enc(b), enc(s), k, u)
        b = list(s)
        b[5] = bad
        refused(pkg.ERR_NONCANONICAL, eng.lookup_permute, enc(a), enc(b), k, u)
    buf = C.create_string_buffer(32 * n)
    p = C.cast(buf, C.c_void_p)
    refused(pkg.ERR_INVALID, eng.lookup_permute, enc(a), enc(s), 25, u)
    refused(pkg.ERR_INVALID, eng.lookup_permute, enc(a + [0] * 6), enc(s + [0] * 6), k, n)
    refused(pkg.ERR_INVALID, eng.lookup_permute, enc(a + [0] * 6), enc(s + [0] * 6), k, n + 1)
    for hole in range(4):
        args = [p, p, p, p]
        args[hole] = None
        refused(pkg.ERR_INVALID, lambda: eng._check(lib.h2agg_lookup_permute(ctx, args[0], args[1], k, u, args[2], args[3])))
        refused(pkg.ERR_INVALID, lambda: eng._check(lib.h2agg_lookup_permute_device(ctx, args[0], args[1], k, u, args[2], args[3])))
    # device ranges: ap / sp overlapping a, s or each other
    d = torch.zeros(32 * 5 * n, dtype=torch.uint8, device=dev)
    at = lambda rows: d.data_ptr() + 32 * rows
    d[:32 * u] = torch.frombuffer(bytearray(enc(a)), dtype=torch.uint8).to(dev)
    d[32 * n:32 * (n + u)] = torch.frombuffer(bytearray(enc(s)), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    for ap_at, sp_at in ((0, 3 * n), (u - 1, 3 * n), (2 * n, n), (2 * n, n + u - 1), (2 * n, 2 * n + u - 1), (2 * n, 2 * n)):
        refused(pkg.ERR_INVALID, eng.lookup_permute_device, at(0), at(n), k, u, at(ap_at), at(sp_at))
    # ... adjacent ranges are fine, and the rows from u up stay as they were
    d[32 * 2 * n:] = 0xA5
    torch.cuda.synchronize()
    eng.lookup_permute_device(at(0), at(n), k, u, at(2 * n), at(2 * n + u))
    eng.synchronize()
    out = bytes(d[32 * 2 * n:32 * (2 * n + 2 * u + 1)].cpu().numpy())
    assert out == enc(good[0]) + enc(good[1]) + bytes([0xA5]) * 32
    # the _device twin reports an absent value at synchronize, once; the context then works
    b = list(a)
    b[7] = hi + 1
    d_b = torch.frombuffer(bytearray(enc(b)), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    eng.lookup_permute_device(d_b.data_ptr(), at(n), k, u, at(2 * n), at(3 * n))
    with pytest.raises(pkg.H2AggError) as ei:
        eng.synchronize()
    assert ei.value.code == pkg.ERR_NOT_IN_TABLE
    eng.synchronize()
    eng.lookup_permute_device(at(0), at(n), k, u, at(2 * n), at(3 * n))
    eng.synchronize()
    assert bytes(d[32 * 2 * n:32 * (2 * n + u)].cpu().numpy()) == enc(good[0])
    assert bytes(d[32 * 3 * n:32 * (3 * n + u)].cpu().numpy()) == enc(good[1])
    assert bytes(d[:32 * u].cpu().numpy()) == enc(a) and bytes(d[32 * n:32 * (n + u)].cpu().numpy()) == enc(s), "an input changed"
    still_works()


# ---------------------------------------------------------------------------------------------- compression
@pytest.mark.parametrize("k", [0, 3, 11, 12])
def test_columns_compress(eng, pkg, poly, k):
    rng = random.Random(0xA40 + k)
    n = 1 << k
    for m in (1, 2, 5):
        cols = [[rng.randrange(R) for _ in range(n)] for _ in range(m)]
        cols[0][0], cols[-1][n - 1] = R - 1, BIG
        for theta in (0, 1, rng.randrange(2, R)):
            want = enc(compress_py(cols, theta))
            assert eng.fr_columns_compress(b"".join(enc(c) for c in cols), m, k, fe(theta)) == want, (m, theta)
            assert poly.compress_expressions(eng, [enc(c) for c in cols], k, fe(theta)) == want
    # the first column under the highest power
    theta = 0xABCDEF
    cols = [[1] * n, [0] * n, [0] * n]
    assert eng.fr_columns_compress(b"".join(enc(c) for c in cols), 3, k, fe(theta)) == enc([theta * theta % R] * n)
    for code, call in ((pkg.ERR_NONCANONICAL, lambda: eng.fr_columns_compress(enc([R] + [0] * (2 * n - 1)), 2, k, fe(theta))),
                       (pkg.ERR_NONCANONICAL, lambda: eng.fr_columns_compress(enc([0] * n), 1, k, enc([R]))),
                       (pkg.ERR_INVALID, lambda: eng.fr_columns_compress(enc([0] * n), 0, k, fe(theta))),
                       (pkg.ERR_INVALID, lambda: eng.fr_columns_compress(enc([0] * n), 1, 25, fe(theta))),
                       (pkg.ERR_INVALID, lambda: eng.fr_columns_compress_device(0, 1, k, fe(theta), 0))):
        with pytest.raises(pkg.H2AggError) as ei:
            call()
        assert ei.value.code == code, ei.value
        assert eng.fr_columns_compress(enc([7] * n), 1, k, fe(theta)) == enc([7] * n)


# ---------------------------------------------------------------------------------------------- the queued chain
def lookup_columns(seed, k, u, m=3):
    """m table columns of random values and m input columns whose usable rows are usable rows of the table"""
    rng = random.Random(seed)
    n = 1 << k
    tables = [[rng.randrange(R) for _ in range(n)] for _ in range(m)]
    rows = [rng.randrange(u) for _ in range(n)]
    inputs = [[col[r] for r in rows] for col in tables]
    return inputs, tables


@pytest.mark.parametrize("k,t,chunk", [(7, SMALL[0], 3), (12, 0, 0)], ids=["k7-smallest", "k12-default"])
def test_compress_permute_product_queued_back_to_back(eng, k, t, chunk):
    """fr_columns_compress_device twice, lookup_permute_device, lookup_product_device on one context, each output the next
    call's input, nothing synchronised in between"""
    import torch
    dev = torch.device("cuda:0")
    n, u = 1 << k, (1 << k) - 6
    theta = 0x13579BDF02468ACE * 0xFEDCBA9876543 % R
    inputs, tables = lookup_columns(0xA50 + k, k, u)
    a, s = compress_py(inputs, theta), compress_py(tables, theta)
    ap, sp = lookup_permute_py(a, s, u)
    z = lookup_product_py(a, s, ap, sp, u, BETA, GAMMA)
    assert z[u] == 1
    up = lambda cols: torch.frombuffer(bytearray(b"".join(enc(c) for c in cols)), dtype=torch.uint8).to(dev)
    d_in, d_tab = up(inputs), up(tables)
    fill = bytes([0xA5]) * 32
    d_a, d_s = torch.zeros(32 * n, dtype=torch.uint8, device=dev), torch.zeros(32 * n, dtype=torch.uint8, device=dev)
    d_ap, d_sp, d_z = [torch.frombuffer(bytearray(fill * n), dtype=torch.uint8).to(dev) for _ in range(3)]
    d_last = torch.zeros(32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eng.debug_configure("fr_sort_tile", t)
    eng.debug_configure("fr_poly_chunk", chunk)
    eng.debug_configure("fr_scan_chunk", chunk)
    try:
        eng.fr_columns_compress_device(d_in.data_ptr(), 3, k, fe(theta), d_a.data_ptr())
        eng.fr_columns_compress_device(d_tab.data_ptr(), 3, k, fe(theta), d_s.data_ptr())
        eng.lookup_permute_device(d_a.data_ptr(), d_s.data_ptr(), k, u, d_ap.data_ptr(), d_sp.data_ptr())
        eng.lookup_product_device(d_a.data_ptr(), d_s.data_ptr(), d_ap.data_ptr(), d_sp.data_ptr(), k, u, fe(BETA), fe(GAMMA),
                                  d_z.data_ptr(), d_last.data_ptr())
        eng.synchronize()
    finally:
        eng.debug_configure("fr_sort_tile", 0)
        eng.debug_configure("fr_poly_chunk", 0)
        eng.debug_configure("fr_scan_chunk", 0)
    assert bytes(d_a.cpu().numpy()) == enc(a) and bytes(d_s.cpu().numpy()) == enc(s)
    assert bytes(d_ap.cpu().numpy()) == enc(ap) + fill * (n - u)
    assert bytes(d_sp.cpu().numpy()) == enc(sp) + fill * (n - u)
    assert bytes(d_z.cpu().numpy()) == enc(z) + fill * (n - u - 1)
    assert bytes(d_last.cpu().numpy()) == fe(1)


# ---------------------------------------------------------------------------------------------- through the verifier
def test_lookup_argument_satisfies_the_verifiers_identity(eng, poly):
    """poly.lookup_argument on a three-column lookup at k = 8: Z, ap and sp against lookup.rs:98-113, row by row"""
    k = 8
    n, u = 1 << k, (1 << k) - 6
    rng = random.Random(0xA60)
    theta = rng.randrange(R)
    inputs, tables = lookup_columns(0xA61, k, u)
    blind = (enc([0xD000 + i for i in range(n - u)]), enc([0xE000 + i for i in range(n - u)]), enc([0xF000 + i for i in range(n - u - 1)]))
    ap_b, sp_b, z_b = poly.lookup_argument(eng, [enc(c) for c in inputs], [enc(c) for c in tables], k, u, fe(theta), fe(BETA), fe(GAMMA),
                                           blinding=blind)
    assert ap_b[32 * u:] == blind[0] and sp_b[32 * u:] == blind[1] and z_b[32 * (u + 1):] == blind[2]
    bare = poly.lookup_argument(eng, [enc(c) for c in inputs], [enc(c) for c in tables], k, u, fe(theta), fe(BETA), fe(GAMMA))
    assert [b[:32 * u] for b in bare] == [ap_b[:32 * u], sp_b[:32 * u], z_b[:32 * u]] and bare[0][32 * u:] == bytes(32 * (n - u))
    ap, sp, z = dec(ap_b), dec(sp_b), dec(z_b)
    a, s = compress_py(inputs, theta), compress_py(tables, theta)
    assert z[0] == 1 and z[u] == 1                                                 # l_0 (1 - z), l_last (z^2 - z)   lookup.rs:98-105
    for i in range(u):                                                             # lookup.rs:106-113
        assert z[i + 1] * (ap[i] + BETA) % R * (sp[i] + GAMMA) % R == z[i] * (a[i] + BETA) % R * (s[i] + GAMMA) % R, i
        assert ap[i] == sp[i] or (i and ap[i] == ap[i - 1]), i                     # :114-119
    assert ap[0] == sp[0]
    with pytest.raises(ValueError):
        poly.permute_expression_pair(eng, enc(a), enc(s), k, u, blinding=(blind[0], blind[1][:-32]))
