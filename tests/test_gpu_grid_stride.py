"""GPU: the grid-stride loops whose workgroup cap goes by the CU count, walked more than once.

On the device these kernels take their second trip above half a million elements (csrc/host.inc launch_cap: 8 workgroups of
256 elements for each of 256 compute units); the debug key launch_cus = 1 makes the cap that of ONE compute unit, so that
inputs of a few thousand elements run the stride step, the clamps of a later trip and the barriers between rounds.  The key
sizes grids and nothing else: every plan, route and kernel is the one that ships.

Everything here runs on a context of its own with launch_cus = 1 (the session's engine never holds the key), every comparison
is byte for byte against the reference the entry point's own tests use, and every test asserts the trip count it is about
with tests/launch_ref.py.  Expected values for thousands of points are tiled from a few oracle results."""
import importlib
import random

import pytest

import __graft_entry__ as entry
from oracle import bn254 as O
from oracle import cref
from oracle import poseidon as P
from tests import keygen_ref as K
from tests import launch_ref
from tests.test_gpu_parity import _edge_pairs, _msm_case
from tests.util import bases_from_coefficients, fr_bytes, msm_want, norm, points_from_scalars, rand_frs

pytestmark = pytest.mark.gpu

CUS = 1
T = 8 * 256            # elements per trip of a grid_for kernel at launch_cus = 1
ID_AFF = bytes(64)
ID_JAC = O.jac_to_bytes(O.INF, 1)


@pytest.fixture(scope="module")
def own(pkg):
    assert pkg.LAUNCH_ELEMENTWISE[0] * pkg.LAUNCH_ELEMENTWISE[1] * CUS == T
    e = pkg.H2Agg(0)
    e.debug_configure("launch_cus", CUS)
    yield e
    e.close()


@pytest.fixture(scope="module")
def geo(pkg):
    """trip counts at launch_cus = 1, from the package's constants"""
    class Geo:
        @staticmethod
        def elementwise(n, share=1):
            per_cu, per_wg = pkg.LAUNCH_ELEMENTWISE
            return launch_ref.trips(n, per_wg, per_cu, CUS, share=share)

        @staticmethod
        def scalar_mul(n):
            per_cu, per_wg = pkg.LAUNCH_SCALAR_MUL
            return launch_ref.trips(n, per_wg, per_cu, CUS)

        @staticmethod
        def size_order(buckets):
            per_cu, per_wg = pkg.LAUNCH_SIZE_ORDER
            return launch_ref.trips(buckets, per_wg, per_cu, CUS, sized_by=8 * per_wg)

        @staticmethod
        def fix(entries):
            per_cu, per_wg = pkg.LAUNCH_MSM_FIX
            return launch_ref.trips(entries, per_wg, per_cu, CUS)

        @staticmethod
        def big(entries):
            per_cu, _lanes = pkg.LAUNCH_MSM_BIG      # one list entry per one-wave workgroup
            return launch_ref.trips(entries, 1, per_cu, CUS)
    return Geo


@pytest.fixture(scope="module")
def pool():
    """64 oracle points g * G with their coefficients: (gs, affine bytes per point)"""
    rng = O.SplitMix64(0x6D5)
    gs = rand_frs(rng, 64)
    aff = points_from_scalars(gs)
    return gs, [aff[64 * i:64 * i + 64] for i in range(64)]


def refused(pkg, call, code):
    with pytest.raises(pkg.H2AggError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)


def rand_z(rng):
    return rng.fr() % O.P or 1


def jac_bytes(aff64, z):
    """(x z^2, y z^3, z) of an affine point given as 64 bytes; (0, 1, 0) for 64 zero bytes, (x, y, 0) for z = 0"""
    if aff64 == ID_AFF:
        return ID_JAC
    if z == 0:
        return aff64 + bytes(32)
    x, y = int.from_bytes(aff64[:32], "little"), int.from_bytes(aff64[32:], "little")
    z2 = z * z % O.P
    return (x * z2 % O.P).to_bytes(32, "little") + (y * z2 * z % O.P).to_bytes(32, "little") + z.to_bytes(32, "little")


# ---------------------------------------------------------------------------------------------- Fr element-wise
def fr_operands(n, seed):
    rng = O.SplitMix64(seed)
    a, b = rand_frs(rng, n), [x or 3 for x in rand_frs(rng, n)]
    for at, va, vb in zip((T - 1, T, 2 * T - 1, 2 * T), (0, 1, O.R - 1, O.R - 2), (O.R - 2, O.R - 1, 1, 2)):
        if at < n:
            a[at], b[at] = va, vb
    return a, b


@pytest.mark.parametrize("n", [T, 2 * T + 1])
def test_fr_batch_op_and_pow_constant(own, pkg, geo, n):
    assert geo.elementwise(n) == (1 if n == T else 3)
    assert geo.elementwise(n - 1) == geo.elementwise(n) - (0 if n == T else 1), "the last trip holds one live lane"
    a, b = fr_operands(n, 0xF0 + n)
    ab, bb = fr_bytes(a), fr_bytes(b)
    inv = lambda x: pow(x, -1, O.R)
    nz = [x or 2 for x in a]
    want = {0: [(x + y) % O.R for x, y in zip(a, b)], 1: [(x - y) % O.R for x, y in zip(a, b)],
            2: [x * y % O.R for x, y in zip(a, b)], 3: [x * x % O.R for x in a], 4: [inv(x) for x in nz],
            5: [x * inv(y) % O.R for x, y in zip(a, b)]}
    for op in range(6):
        first = fr_bytes(nz) if op == 4 else ab
        got = own.fr_batch_op(op, first, bb if op in (0, 1, 2, 5) else None)
        bad = [i for i in range(n) if got[32 * i:32 * i + 32] != O.fe_to_bytes(want[op][i])]
        assert not bad, (op, bad[:8])
    for e in (1, 3, (1 << 64) - 1):
        assert own.fr_batch_pow_constant(ab, e) == fr_bytes([pow(x, e, O.R) for x in a]), e
    if n > 2 * T:
        at = 32 * 2 * T                                       # the one live lane of the third trip
        zero_div, big = bb[:at] + bytes(32), ab[:at] + O.R.to_bytes(32, "little")
        with pytest.raises(pkg.DivisionByZero):
            own.fr_batch_op(5, ab, zero_div)
        assert own.fr_batch_op(5, ab, bb) == fr_bytes(want[5])
        with pytest.raises(pkg.DivisionByZero):
            own.fr_batch_op(4, zero_div)
        assert own.fr_batch_op(4, fr_bytes(nz)) == fr_bytes(want[4])
        for op in (0, 3):
            refused(pkg, lambda: own.fr_batch_op(op, big, bb if op == 0 else None), pkg.ERR_NONCANONICAL)
            assert own.fr_batch_op(op, ab, bb if op == 0 else None) == fr_bytes(want[op])
        refused(pkg, lambda: own.fr_batch_pow_constant(big, 5), pkg.ERR_NONCANONICAL)
        assert own.fr_batch_pow_constant(ab, 5) == fr_bytes([pow(x, 5, O.R) for x in a])


# ---------------------------------------------------------------------------------------------- G1 element-wise
@pytest.mark.parametrize("subtract", [False, True])
def test_g1_batch_add_exceptional_pairs_in_every_trip(own, geo, subtract):
    n = 2 * T + 1
    pairs = _edge_pairs()
    assert geo.elementwise(n) == 3 and T % len(pairs) == 0, "each pair occurs in the second trip, pair 0 in the third"
    rng = O.SplitMix64(0xADD + subtract)
    a = b"".join(O.jac_to_bytes(pairs[i % 8][0], rand_z(rng)) for i in range(n))
    b = b"".join(O.jac_to_bytes(pairs[i % 8][1], rand_z(rng)) for i in range(n))
    want8 = [O.aff_to_bytes(O.sub(p, q) if subtract else O.add(p, q)) for p, q in pairs]
    got = norm(None, own.g1_batch_add(a, b, subtract))
    bad = [i for i in range(n) if got[64 * i:64 * i + 64] != want8[i % 8]]
    assert not bad, bad[:8]


def test_g1_batch_scalar_mul_rounds_behind_the_barrier(own, pkg, geo):
    """k_g1_batch_scalar_mul_w4: 32 points per workgroup, four lanes each, the LDS table reused in every round"""
    per_trip = pkg.LAUNCH_SCALAR_MUL[0] * pkg.LAUNCH_SCALAR_MUL[1]
    sizes = [per_trip, per_trip + 1, 2 * per_trip + 5]
    assert sizes == [512, 513, 1029] and [geo.scalar_mul(n) for n in sizes] == [1, 2, 3]
    n = sizes[-1]
    rng = O.SplitMix64(0x5CA)
    bases = bytearray(points_from_scalars(rand_frs(rng, n)))
    ss = rand_frs(rng, n)
    # the first workgroup of the second trip (points 512 .. 543): identity bases in some four-lane groups, not in others
    identities = [512, 514, 515, 519, 530, 543, 700, 1023, 1024, 1027]
    for i in identities:
        bases[64 * i:64 * i + 64] = ID_AFF
    for at, s in ((513, 0), (516, 1), (517, O.R - 1), (1025, 0), (1026, O.R - 1), (1028, 1)):
        ss[at] = s
    bases, sb = bytes(bases), fr_bytes(ss)
    want = norm(None, cref.g1_batch_scalar_mul(bases, sb, n))
    assert all(want[64 * i:64 * i + 64] == ID_AFF for i in identities + [513, 1025])
    assert want[64 * 516:64 * 517] == bases[64 * 516:64 * 517] and want[64 * 1028:] == bases[64 * 1028:]
    for m in sizes:
        got = norm(None, own.g1_batch_scalar_mul(bases[:64 * m], sb[:32 * m]))
        bad = [i for i in range(m) if got[64 * i:64 * i + 64] != want[64 * i:64 * i + 64]]
        assert not bad, (m, bad[:8])


# ---------------------------------------------------------------------------------------------- to_affine: the shared inversion
TA_K = 8
TA_SIZES = [T + 1, 8 * T, 8 * T + 1, 9 * T + 3]


@pytest.fixture(scope="module")
def jacobians(pool):
    """9T + 3 Jacobian points over the pool with the z's of the shared-inversion cases, and their affine forms; lane L of the
    launch holds the points L + j T, j < 8, of a trip (every prefix of more than T points has stride T)"""
    rng = O.SplitMix64(0x7AF)
    n = TA_SIZES[-1]
    _gs, pts = pool
    ident = {3, 5 + T}                                             # at i and not at i + T; at i + T and not at i
    ident |= {7 + j * T for j in range(TA_K)}                      # a lane whose eight points are all identities
    ident |= {9 + j * T for j in range(TA_K - 1)}                  # a lane whose only non-identity point is its last
    ident |= {11 + j * T for j in (1, 2, 5)} | {8 * T + 1, 9 * T}  # inside a shared run; in the second outer trip
    aff, jac = [], []
    for i in range(n):
        if i in ident:
            aff.append(ID_AFF)
            jac.append(O.jac_to_bytes(O.INF, 1) if i % 2 else jac_bytes(pts[i % 64], 0))   # (0, 1, 0) and (x, y, 0)
        else:
            aff.append(pts[i % 64])
            jac.append(jac_bytes(pts[i % 64], 1 if i % 5 == 0 else rand_z(rng)))
    return b"".join(aff), b"".join(jac), ident


@pytest.mark.parametrize("n", TA_SIZES)
def test_g1_batch_to_affine_shares_one_inversion(own, pkg, geo, jacobians, n):
    import torch
    aff, jac, ident = jacobians
    per_cu, per_wg = pkg.LAUNCH_ELEMENTWISE
    shared = launch_ref.shared_points(n, per_wg, per_cu, CUS, TA_K)
    assert (shared, geo.elementwise(n, share=TA_K)) == {T + 1: (2, 1), 8 * T: (8, 1), 8 * T + 1: (8, 2), 9 * T + 3: (8, 2)}[n]
    if n >= 8 * T:
        assert all(7 + j * T in ident for j in range(8)) and 9 + 7 * T not in ident and 9 + 6 * T in ident
    want = aff[:64 * n]
    got = own.g1_batch_to_affine(jac[:96 * n])
    bad = [i for i in range(n) if got[64 * i:64 * i + 64] != want[64 * i:64 * i + 64]]
    assert not bad, bad[:8]
    d_jac = torch.frombuffer(bytearray(jac[:96 * n]), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert own.g1_batch_to_affine_device(d_jac.data_ptr(), n) == want
    if n == 8 * T + 1:                                             # the one point of the second outer trip
        bad_x = jac[:96 * 8 * T] + O.P.to_bytes(32, "little") + jac[96 * 8 * T + 32:96 * n]
        refused(pkg, lambda: own.g1_batch_to_affine(bad_x), pkg.ERR_NONCANONICAL)
        assert own.g1_batch_to_affine(jac[:96 * n]) == want


@pytest.mark.parametrize("n", [8 * T + 1, 16 * T + 5])
def test_g1_msm_jac_normalises_with_a_second_outer_trip(own, geo, pool, n):
    """MONT = true: h2agg_g1_msm_jac launches one lane per eight points, so 8T + 1 points are 2049 lanes: a second trip"""
    assert geo.elementwise((n + TA_K - 1) // TA_K) == {8 * T + 1: 2, 16 * T + 5: 3}[n]
    gs_pool, pts = pool
    rng = O.SplitMix64(0x1AC + n)
    gs, jac = [], []
    for i in range(n):
        if i % 11 == 5:
            gs.append(0)
            jac.append(ID_JAC)
        else:
            gs.append(gs_pool[i % 64])
            jac.append(jac_bytes(pts[i % 64], 1 if i % 3 == 0 else rand_z(rng)))
    ss = rand_frs(rng, n)
    assert norm(None, own.g1_msm_jac(b"".join(jac), fr_bytes(ss))) == msm_want(gs, ss)


# ---------------------------------------------------------------------------------------------- wire format
def test_decompress_and_compress_in_the_last_trip(own, pkg, geo):
    n = 2 * T + 1
    assert geo.elementwise(n) == 3
    rng = O.SplitMix64(0x3137)
    base = [O.scalar_mul(rng.fr(), O.G1) for _ in range(14)] + [O.INF, O.neg(O.G1)]
    pts = [base[i % 16] for i in range(n)]
    pts[2 * T] = O.INF                                           # an identity is the third trip's one element
    enc = b"".join(O.compress(p) for p in base) * (n // 16) + O.compress(O.INF)
    aff = b"".join(O.aff_to_bytes(p) for p in pts)
    assert own.g1_batch_decompress(enc) == aff
    assert own.g1_batch_compress(aff) == enc
    x = 2
    while True:                                                  # x with x^3 + 3 a non-residue
        try:
            O.decompress(x.to_bytes(32, "little"))
            x += 1
        except ValueError:
            break
    bad_at = [T, 2 * T - 1, 2 * T]
    data = bytearray(enc)
    for at in bad_at:
        data[32 * at:32 * at + 32] = x.to_bytes(32, "little")
    with pytest.raises(pkg.BadPoint):
        own.g1_batch_decompress(bytes(data))
    out, ok = own.g1_batch_decompress(bytes(data), with_ok=True)
    assert list(ok) == [0 if i in bad_at else 1 for i in range(n)]
    want = bytearray(aff)
    for at in bad_at:
        want[64 * at:64 * at + 64] = ID_AFF
    assert out == bytes(want)
    refused(pkg, lambda: own.g1_batch_compress(aff[:64 * 2 * T] + (O.P + 1).to_bytes(32, "little") + (2).to_bytes(32, "little")),
            pkg.ERR_NONCANONICAL)
    assert own.g1_batch_compress(aff) == enc


# ---------------------------------------------------------------------------------------------- base tables
def test_bases_upload_download_precompute_and_comb(own, pkg, geo, pool):
    n = 2 * T + 1
    assert geo.elementwise(n) == 3
    gs_pool, pts = pool
    gs = [gs_pool[(5 * i + i // 64) % 64] for i in range(n)]
    for at in (T, 2 * T - 1, 2 * T):
        gs[at] = 0                                               # identity bases
    bases = bases_from_coefficients(gs)
    rng = O.SplitMix64(0xBA5)
    ss = rand_frs(rng, n)
    h = own.bases_upload(bases)
    try:
        assert own.table_may_hold_identity(h)
        for first, count in ((0, n), (T - 3, 7), (2 * T - 2, 3), (T, T + 1), (2 * T, 1)):
            assert own.bases_download(h, first, count) == bases[64 * first:64 * (first + count)], (first, count)
        assert norm(None, own.g1_msm_preloaded(h, fr_bytes(ss))) == msm_want(gs, ss)
        own.bases_precompute(h)                                  # k_bases_shift over the table, level by level
        assert norm(None, own.g1_msm_preloaded(h, fr_bytes(ss))) == msm_want(gs, ss)
        assert own.bases_download(h, T - 3, 7) == bases[64 * (T - 3):64 * (T + 4)]
        # a short multi_exp over the precomputed table takes the comb, whose rows k_comb_table_build makes: 32 x 255 entries
        # for each of at least 16 bases, 32 entries per workgroup
        assert geo.scalar_mul(16 * 32 * 255) == 255
        for m in (20, 1):
            assert norm(None, own.g1_msm_preloaded(h, fr_bytes(ss[:m]))) == msm_want(gs[:m], ss[:m]), m
    finally:
        own.bases_free(h)


# ---------------------------------------------------------------------------------------------- MSM
N_MSM = 2 * T + 77


def configured_msm(own, bases, sb, c, glv, lanes=0):
    own.msm_configure(window_bits=c, big_bucket_threshold=64)
    own.msm_configure_glv(glv)
    own.msm_configure_lanes_per_bucket(lanes)
    try:
        return norm(None, own.g1_msm(bases, sb))
    finally:
        own.msm_configure()
        own.msm_configure_glv(0)
        own.msm_configure_lanes_per_bucket(0)


@pytest.fixture(scope="module")
def msm_cases():
    return {kind: _msm_case(O.SplitMix64(0x3500 + len(kind)), N_MSM, kind) for kind in ("edges", "equal_scalars")}


@pytest.mark.parametrize("glv", [1, -1])
@pytest.mark.parametrize("c", [11, 13])
@pytest.mark.parametrize("kind", ["edges", "equal_scalars"])
def test_msm_decomposition_and_size_order(own, geo, msm_cases, kind, c, glv):
    """k_glv_decompose / k_bases_endo_x over 2T + 77 scalars and bases (three trips); the size order of the buckets
    (k_size_count / k_size_scatter: the MSM orders its buckets from 2^16 insertions on) over at least one window of 2^(c-1)
    buckets in each of at least ceil(127 / c) windows, 1024 buckets per trip"""
    assert geo.elementwise(N_MSM) == 3
    windows = -(-127 // c)                                        # a half scalar's, the fewest a plan can have
    insertions = N_MSM * (2 * windows if glv == 1 else -(-254 // c))
    assert insertions >= 1 << 16, "the buckets are ordered"
    assert geo.size_order(windows << (c - 1)) >= 2
    bases, sb, want = msm_cases[kind]
    assert configured_msm(own, bases, sb, c, glv) == want


def test_msm_fix_list_beyond_one_trip(own, pkg, geo, pool):
    """Every base the same point, scalars 1 .. 1023 each at least four times, one lane per bucket, plain 11-bit windows: the
    digit of the lowest window is the scalar itself (below 2^10, no carry), so each of its 1023 buckets meets P + P at its
    second entry and goes to the fix-up list: 1023 entries, 768 per trip of k_msm_accumulate_fix"""
    gs_pool, _pts = pool
    ss = [1 + i % 1023 for i in range(N_MSM)]
    assert len(set(ss)) == 1023 and N_MSM >= 2 * 1023 and geo.fix(1023) == 2
    gs = [gs_pool[0]] * N_MSM
    got = configured_msm(own, bases_from_coefficients(gs), fr_bytes(ss), 11, -1, lanes=1)
    assert got == msm_want(gs, ss)


@pytest.mark.parametrize("glv", [-1, 1])
@pytest.mark.parametrize("c", [11, 13])
def test_msm_over_long_bucket_lists_beyond_one_trip(own, pkg, geo, pool, c, glv):
    """One scalar for all 8T + 77 points whose c-bit digits are all 1 (plain windows: no carry), threshold 64: one over-long
    bucket per window, cut into chunks of 512 entries (csrc/msm_kernels.hpp big_chunk_size), one workgroup per chunk
    (k_msm_accumulate_big) and one per bucket (k_msm_big_combine), eight workgroups per trip"""
    n = 8 * T + 77
    windows = 253 // c
    s = sum(1 << (c * w) for w in range(windows))
    assert s < O.R and n // 256 < 512
    chunks = windows * -(-n // 512)
    assert chunks > 8 * 64 and geo.big(chunks) >= 64 and geo.big(windows) >= 3
    gs_pool, _pts = pool
    gs = [gs_pool[(3 * i + i // 64) % 64] for i in range(n)]
    ss = [s] * n
    assert configured_msm(own, bases_from_coefficients(gs), fr_bytes(ss), c, glv) == msm_want(gs, ss)


def test_g1_msm_segmented_converts_its_bases_in_two_trips(own, geo, pool):
    lens = [1, 2, 65, 300, 700] * 3
    n = sum(lens)
    assert geo.elementwise(n) == 2                                # k_bases_to_mont
    gs_pool, _pts = pool
    rng = O.SplitMix64(0x5E6)
    gs = [gs_pool[(7 * i + i // 64) % 64] for i in range(n)]
    ss = rand_frs(rng, n)
    gs[T], ss[T + 1], ss[n - 1] = 0, 0, O.R - 1
    got = norm(None, b"".join(own.g1_msm_segmented(bases_from_coefficients(gs), fr_bytes(ss), lens)))
    at = 0
    for k, ln in enumerate(lens):
        assert got[64 * k:64 * k + 64] == msm_want(gs[at:at + ln], ss[at:at + ln]), k
        at += ln


# ---------------------------------------------------------------------------------------------- G1 transform
def test_bases_fft_against_the_setups_g_lagrange(own, eng, geo):
    """k = 13 inverse: 4096 twiddle records (k_fft_twiddle_digits, two trips), 8192 points through k_g1_fft_to_jac (four
    trips) and k_jac_to_mont_affine (one trip in which every lane shares four points)"""
    k = 13
    n = 1 << k
    assert geo.elementwise(n // 2) == 2 and geo.elementwise(n) == 4
    s = O.fe_to_bytes(O.SplitMix64(0xFF7).fr() or 5)
    hg, hl = own.params_setup(k, s)
    eg, el = eng.params_setup(k, s)                               # the same tables made without the key
    try:
        want = eng.bases_download(el, 0, n)
        assert own.bases_download(hl, 0, n) == want and own.bases_download(hg, 0, n) == eng.bases_download(eg, 0, n)
        o = own.bases_fft(hg, k, inverse=True)
        try:
            assert own.bases_download(o, 0, n) == want
        finally:
            own.bases_free(o)
    finally:
        for e, hs in ((own, (hg, hl)), (eng, (eg, el))):
            for h in hs:
                e.bases_free(h)


# ---------------------------------------------------------------------------------------------- keys and columns
def test_permutation_sigmas_over_two_trips(own, pkg, geo):
    m, k = 3, 10
    n = 1 << k
    usable = n - 6
    assert geo.elementwise(m * n) == 2                            # k_perm_sigma: one lane per cell
    rng = random.Random(0x51A)
    copies = K.random_copies(rng, m, k, usable, m * usable) + [(1, 1000, 2, 0), (0, 5, 2, 0)]
    mapping = K.assembly_py(m, k, usable, copies)
    assert K.is_valid_mapping(mapping, m, k, usable)
    crossing = [cyc for cyc in K.cycles_of(mapping, m, k) if (2, 0) in cyc][0]
    assert any(c * n + r < T for c, r in crossing) and any(c * n + r >= T for c, r in crossing), "a cycle crosses cell 2048"
    words = K.mapping_words(mapping)
    want = fr_bytes([v for col in K.sigmas_py(mapping, m, k) for v in col])
    delta = O.fe_to_bytes(K.DELTA)
    lag, co = own.permutation_sigmas(words, m, k, usable, delta)
    assert lag == want
    assert co == own.fr_fft_batch(lag, k, inverse=True)
    dup = list(mapping)
    dup[2 * n + 7] = dup[2 * n + 300]                             # a repeated target, both cells in the second trip
    assert not K.is_valid_mapping(dup, m, k, usable)
    refused(pkg, lambda: own.permutation_sigmas(K.mapping_words(dup), m, k, usable, delta), pkg.ERR_INVALID)
    assert own.permutation_sigmas(words, m, k, usable, delta, coeff=False)[0] == want


def test_columns_write_checks_every_trip(own, pkg, geo):
    m, k = 3, 10
    assert geo.elementwise(m << k) == 2                           # k_columns_canonical
    rng = O.SplitMix64(0xC01)
    good = fr_bytes(rand_frs(rng, m << k))
    other = fr_bytes(rand_frs(rng, m << k))
    keep = fr_bytes(rand_frs(rng, 1 << k))
    h = own.columns_create(m + 1, k)                              # a column in front that no write here touches
    try:
        own.columns_write(h, 0, keep)
        own.columns_write(h, 1, good)
        assert own.columns_read(h, 0, m + 1) == keep + good
        at = 32 * ((m << k) - 5)                                  # in the last column: the second trip
        bad = other[:at] + O.R.to_bytes(32, "little") + other[at + 32:]
        refused(pkg, lambda: own.columns_write(h, 1, bad), pkg.ERR_NONCANONICAL)
        # the store still reads back: the written columns are unspecified (include/h2agg.h), the others as before
        assert len(own.columns_read(h, 1, m)) == 32 * (m << k) and own.columns_read(h, 0, 1) == keep
        own.columns_write(h, 1, good)
        assert own.columns_read(h, 0, m + 1) == keep + good
    finally:
        own.columns_destroy(h)


# ---------------------------------------------------------------------------------------------- transcripts
SCRIPT = "CX" + "PPP" + "Q" + "PP" + "QQ" + "PPPP" + "Q" + "PP" + "Q" + "SSSSSSSSSSS" + "Q" + "PPP" + "Q" + "Q"


def items_of(script):
    return len(script) - script.count("Q")                       # a squeeze is no item of the element-stream kernels


def test_transcript_read_batch_over_two_trips(own, pkg, geo):
    """the script of tests/test_gpu_poseidon.py, 80 proofs (16 written by the oracle, repeated): k_transcript_elements takes
    one lane per (proof, item), proof-major"""
    nproofs, distinct = 80, 16
    items = items_of(SCRIPT)
    assert nproofs >= 64 and geo.elementwise(nproofs * items) == 2
    second = T // items + 1                                      # the first proof all of whose items are in the second trip
    assert second * items >= T and second < nproofs - 1
    rng = O.SplitMix64(0x907)
    pts_pool = [O.scalar_mul(rng.fr(), O.G1) for _ in range(24)]
    vk_scalar = rng.fr()
    scalar_at = 32 * SCRIPT[:SCRIPT.index("S")].count("P")

    def write(identity_at=None):
        w = P.PoseidonTranscriptWrite()
        inst = pts_pool[rng.next() % 24]
        pts, ch = [], []
        for op in SCRIPT:
            if op == "C":
                w.common_scalar(vk_scalar)
            elif op == "X":
                w.common_point(inst)
            elif op == "P":
                p = O.INF if len(pts) == identity_at else pts_pool[rng.next() % 24]
                w.write_point(p)
                pts.append(p)
            elif op == "S":
                w.write_scalar(rng.fr())
            else:
                ch.append(w.squeeze_challenge_scalar())
        return w.finalize(), O.aff_to_bytes(inst), b"".join(O.aff_to_bytes(p) for p in pts), fr_bytes(ch)
    base = [write() for _ in range(distinct)]
    rows = [base[i % distinct] for i in range(nproofs)]
    rows[second] = write(identity_at=4)                          # an identity point in a proof of the second trip
    proofs, ext, want_pts, want_ch = [list(col) for col in zip(*rows)]
    assert want_pts[second][64 * 4:64 * 5] == ID_AFF
    consts, extb = O.fe_to_bytes(vk_scalar), b"".join(ext)
    got_pts, got_ch = own.transcript_read_batch(proofs, SCRIPT, consts, extb)
    assert got_pts == want_pts and got_ch == want_ch
    bad = bytearray(proofs[second + 1])
    bad[scalar_at:scalar_at + 32] = O.R.to_bytes(32, "little")
    refused(pkg, lambda: own.transcript_read_batch(proofs[:second + 1] + [bytes(bad)] + proofs[second + 2:], SCRIPT, consts, extb),
            pkg.ERR_NONCANONICAL)
    assert own.transcript_read_batch(proofs, SCRIPT, consts, extb) == (want_pts, want_ch)


@pytest.mark.parametrize("kind", ["sha256", "keccak256"])
def test_hash_transcript_read_batch_over_two_trips(own, pkg, geo, pool, kind):
    """256 proofs (32 distinct, repeated): k_hash_transcript_stream takes one lane per (item, proof), item-major, so the items
    from the eighth on - every scalar and the last four points of this script - are read in the second and third trip"""
    from tests.test_hash_transcript_host import reference
    script = "CXPPQPQQPPPQSSSSSQPPPPQQ"
    nproofs, distinct = 256, 32
    items = items_of(script)
    assert geo.elementwise(nproofs * items) == 3
    item_of = lambda at: items_of(script[:at])                    # the item index of the script position
    first_scalar, last_point = script.index("S"), script.rindex("P")
    assert item_of(first_scalar) * nproofs >= T and item_of(last_point) * nproofs >= 2 * T
    offset = lambda at: 64 * script[:at].count("P") + 32 * script[:at].count("S")
    _gs, pts = pool
    rng = O.SplitMix64(0x7E0 + len(kind))
    consts = [rng.fr()]
    proofs, exts = [], []
    for _ in range(distinct):
        proofs.append(b"".join(pts[rng.next() % 64] if ch == "P" else O.fe_to_bytes(rng.fr()) for ch in script if ch in "PS"))
        exts.append([O.aff_from_bytes(pts[rng.next() % 64])])
    want_pts, want_chal, _ = reference(kind, script, proofs, consts, exts)
    proofs, exts = proofs * (nproofs // distinct), exts * (nproofs // distinct)
    want = (want_pts * (nproofs // distinct), want_chal * (nproofs // distinct))
    cb = fr_bytes(consts)
    xb = b"".join(O.aff_to_bytes(p) for x in exts for p in x)

    def with_bytes(kth, off, b):
        ps = list(proofs)
        ps[kth] = ps[kth][:off] + b + ps[kth][off + len(b):]
        return ps
    own.transcript_configure("device")                            # (the automatic choice runs the chains on host threads)
    try:
        got = own.hash_transcript_read_batch(kind, proofs, script, cb, xb)
        assert (got[0], got[1]) == want
        with pytest.raises(pkg.BadPoint):                         # an identity point read in the third trip
            own.hash_transcript_read_batch(kind, with_bytes(200, offset(last_point), ID_AFF), script, cb, xb)
        refused(pkg, lambda: own.hash_transcript_read_batch(kind, with_bytes(77, offset(first_scalar), O.R.to_bytes(32, "little")),
                                                             script, cb, xb), pkg.ERR_NONCANONICAL)
        got = own.hash_transcript_read_batch(kind, proofs, script, cb, xb)
        assert (got[0], got[1]) == want
    finally:
        own.transcript_configure("auto")


# ---------------------------------------------------------------------------------------------- a whole proof
def test_an_honest_proof_verifies_alike_with_and_without_the_key(own, eng, pkg):
    """k = 7: the device's prover stages write the proof on the session's engine; h2agg_verify_proofs answers the same status,
    verdict and final pair under launch_cus = 1 as the same context does at 0, and as the session's engine does"""
    from tests import honest_prover as HP
    from tests.test_gpu_honest_proofs import TAU, Product, device_prove
    poly = importlib.import_module(entry.PKG_NAME + ".poly")
    verifier = importlib.import_module(entry.PKG_NAME + ".verifier")
    k = 7
    setup = HP.Setup(k, TAU, HP.INSTANCE_ROWS)
    proof = device_prove(pkg, eng, poly, verifier, setup, HP.make_circuit(random.Random(0xD77), k, 4))

    def verdict(e):
        prod = Product(e, verifier, {k: setup}, [[proof]])
        try:
            return [(r[0] + r[1], r[2], r[3]) for r in prod.each()]
        finally:
            prod.close()
    keyed = verdict(own)
    own.debug_configure("launch_cus", 0)
    try:
        plain = verdict(own)
    finally:
        own.debug_configure("launch_cus", CUS)
    assert [(s, ok) for _pair, s, ok in keyed] == [(0, True)]
    assert keyed == plain == verdict(eng)
