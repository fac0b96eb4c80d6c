"""GPU: keys on the device — h2agg_permutation_sigmas (k_perm_sigma and the batched inverse transform), h2agg_commit_columns
(one staging, the batched MSM), and poly.py's permutation_key / fixed_key over them.

halo2_proofs is not vendored in the reference, so the yardstick is the definition in include/h2agg.h, restated with Python
integers in tests/keygen_ref.py (tests/test_keygen_host.py ties it to the scaffolding of tests/quotient_ref.py).  Field
elements and points are exact and compared byte for byte; the one check of meaning (the assembly orders a cycle differently
from the scaffold) is that the permutation argument and the quotient close over the sigma columns made here."""
import copy
import ctypes
import importlib
import random

import pytest

import __graft_entry__ as entry
from oracle import bn254 as O
from tests import keygen_ref as K
from tests import quotient_ref as Q
from tests.fr_bytes import dec, enc, fe
from tests.test_gpu_quotient import cols, make_vk, scalars

pytestmark = pytest.mark.gpu

R = K.R
DELTA = fe(K.DELTA)
ONE = fe(1)
IDENTITY = bytes(64)
SHAPES = [(7, 5, 26), (1, 0, 1), (3, 1, 2), (5, 11, 2042), (3, 13, 8186)]   # (m, k, usable)


@pytest.fixture(scope="module")
def poly(pkg):
    return importlib.import_module(entry.PKG_NAME + ".poly")


@pytest.fixture(scope="module")
def verifier(pkg):
    return importlib.import_module(entry.PKG_NAME + ".verifier")


@pytest.fixture(scope="module")
def cases():
    """(m, k, usable) -> (mapping words, the Lagrange slab sigmas_py gives): computed once, shared, left unchanged"""
    out = {}
    for m, k, usable in SHAPES:
        rng = random.Random(0x51A + 64 * m + k)
        mapping = K.assembly_py(m, k, usable, K.random_copies(rng, m, k, usable, m * usable))
        assert K.is_valid_mapping(mapping, m, k, usable)
        out[(m, k, usable)] = (K.mapping_words(mapping), b"".join(enc(c) for c in K.sigmas_py(mapping, m, k)))
    return out


@pytest.fixture(scope="module")
def params(eng):
    """k -> (s, g handle, g_lagrange handle)"""
    out = {}
    for k in (5, 11):
        s = random.Random(0x5E7 + k).randrange(1, R)
        g, gl = eng.params_setup(k, fe(s))
        out[k] = (s, g, gl)
    yield out
    for _s, g, gl in out.values():
        eng.bases_free(g)
        eng.bases_free(gl)


def check_sigmas(e, words, m, k, usable, want):
    lag, co = e.permutation_sigmas(words, m, k, usable, DELTA)
    assert lag == want, "lagrange"
    assert co == e.fr_fft_batch(lag, k, inverse=True), "coefficient form against fr_fft_batch of the same context"
    assert e.permutation_sigmas(words, m, k, usable, DELTA, coeff=False) == (lag, None), "lagrange alone"
    assert e.permutation_sigmas(words, m, k, usable, DELTA, lagrange=False) == (None, co), "coeff alone (in place)"
    return co


@pytest.mark.parametrize("m,k,usable", SHAPES)
def test_sigmas_on_a_fresh_context_and_after_the_tables_grew(pkg, cases, m, k, usable):
    """(5, 11) and (3, 13) put exponents on both sides of the twiddle tables' split; after an fr_fft at k = 16 every exponent
    is shifted by 16 - k and the split moves to 8 bits"""
    words, want = cases[(m, k, usable)]
    e = pkg.H2Agg(0)
    try:
        co = check_sigmas(e, words, m, k, usable, want)
        if k == 5:
            n = 1 << k
            lag = dec(want)
            assert co == b"".join(enc(Q.ntt(lag[j * n:(j + 1) * n], k, inverse=True)) for j in range(m)), "coeff against ntt"
        zeros = bytes(32 << 16)
        assert e.fr_fft(zeros, 16) == zeros and e.fr_fft(zeros, 16, inverse=True) == zeros
        assert check_sigmas(e, words, m, k, usable, want) == co, "grown tables"
        # array('I') and ctypes forms of the mapping
        arr = (ctypes.c_uint32 * (len(words) // 4)).from_buffer_copy(words)
        assert e.permutation_sigmas(arr, m, k, usable, DELTA, coeff=False)[0] == want
    finally:
        e.close()


def test_the_key_closes_the_permutation_argument_and_the_quotient(eng, pkg, poly, verifier, params):
    k, degree = 5, 5
    cs, lag, polys, sc = Q.satisfied_circuit(random.Random(0xD00 + k), k, degree)
    n, u = cs.n, cs.n - cs.blinding_factors - 1
    _s, _g, gl = params[k]
    columns = [lag[kind][col] for kind, col in cs.permutation_columns]
    m = len(columns)
    classes = {}
    for j, colv in enumerate(columns):
        for i in range(u):
            classes.setdefault(colv[i], []).append((j, i))
    # every cell of a class copied to the class's first: the same classes as the scaffold's, joined in another order
    copies = [cells[0] + cells[t] for cells in classes.values() for t in range(1, len(cells))]
    mapping = poly.permutation_mapping(m, k, u, copies)
    assert mapping == K.mapping_words(K.assembly_py(m, k, u, copies))
    sig_lag, sig_coeff, sig_commit = poly.permutation_key(eng, gl, mapping, m, k, u, DELTA)
    assert len(sig_lag) == len(sig_coeff) == len(sig_commit) == m
    assert b"".join(sig_lag) != b"".join(enc(c) for c in lag["sigma"]), "the assembly's cycle order is its own"
    ch, theta, beta, gamma, y, delta = scalars(sc)
    # the grand product over the witness and THESE sigma columns ends at 1
    zs = poly.permutation_products(eng, cols(columns), sig_lag, k, u, beta, gamma, delta, cs.chunk_len)
    assert len(zs) == cs.num_permutation_sets and zs[-1][32 * u:32 * u + 32] == ONE and zs[0][:32] == ONE
    # and the quotient over their coefficient form is the definition's
    mine = dict(polys)
    mine["sigma"] = [dec(c) for c in sig_coeff]
    mine["perm_z"] = [dec(c) for c in poly.columns_lagrange_to_coeff(eng, zs, k)]
    want, H = Q.quotient_py(cs, *Q.quotient_args(mine, sc))
    assert not any(H[(degree - 1) << k:]), "the circuit holds with the key made here"
    vk = make_vk(eng, verifier, cs)
    try:
        got = poly.quotient_pieces(eng, vk, *[cols(mine[kind]) for kind in Q.POLY_KINDS], ch, theta, beta, gamma, y, delta)
        assert got == cols(want)
    finally:
        vk.close()
    # the commitments make a verifying key the library accepts
    fixed_coeff, fixed_commit = poly.fixed_key(eng, gl, cols(lag["fixed"]), k)
    assert fixed_coeff == cols(polys["fixed"])
    keyed = copy.copy(cs)
    keyed.fixed_commitments, keyed.permutation_commitments = list(fixed_commit), list(sig_commit)
    blob = verifier.encode_vk(keyed, lambda b: b)
    assert blob != verifier.encode_vk(cs, O.aff_to_bytes)
    vk2 = verifier.VerifyingKey(eng, blob)
    try:
        assert vk2.shape["num_permutation_columns"] == m and vk2.shape["num_fixed"] == len(fixed_commit)
    finally:
        vk2.close()


def aff(pt):
    return IDENTITY if pt is None else O.aff_to_bytes(pt)


def column_mix(rng, k):
    """Lagrange columns: all zero, one non-zero row, a sigma-like dense one, r - 1 everywhere, a random one"""
    n = 1 << k
    one_row = [0] * n
    one_row[rng.randrange(n)] = rng.randrange(1, R)
    return [[0] * n, one_row, [rng.randrange(R) for _ in range(n)], [R - 1] * n, [rng.randrange(R) for _ in range(n)]]


@pytest.mark.parametrize("k", [5, 11])
def test_commitments_against_the_oracle_and_the_single_msm(eng, poly, params, k):
    s, g, gl = params[k]
    rng = random.Random(0xC0 + k)
    columns = column_mix(rng, k)
    coeffs = [Q.ntt(c, k, inverse=True) for c in columns]
    want = [aff(O.scalar_mul(Q.horner(c, s), O.G1)) for c in coeffs]
    assert want[0] == IDENTITY and want[1] != IDENTITY
    got = poly.commit_columns_lagrange(eng, gl, cols(columns), k)
    assert got == want, "commit_lagrange of every column is [p(s)] G"
    single = [eng.g1_batch_to_affine(eng.g1_msm_preloaded(gl, c)) for c in cols(columns)]
    assert got == single, "the affine form of g1_msm_preloaded per column"
    assert poly.commit_columns_coeff(eng, g, cols(coeffs), k) == want, "the coefficient columns against g"
    assert poly.commit_columns_lagrange(eng, gl, cols(columns[2:3]), k) == want[2:3], "m = 1"
    assert poly.commit_columns_lagrange(eng, gl, cols(columns[:1]), k) == [IDENTITY], "m = 1, the zero column"
    try:   # five columns in chunks of 2, 2, 1 and of 1: across the slab call's chunk boundary
        for chunk in (2, 1):
            eng.debug_configure("commit_chunk", chunk)
            assert poly.commit_columns_lagrange(eng, gl, cols(columns), k) == want, chunk
    finally:
        eng.debug_configure("commit_chunk", 0)
    # the fixed columns' share of a key, and sigma columns through permutation_key
    fixed_coeff, fixed_commit = poly.fixed_key(eng, gl, cols(columns), k)
    assert fixed_coeff == cols(coeffs) and fixed_commit == want
    m, usable = 3, (1 << k) - 6
    mapping = K.assembly_py(m, k, usable, K.random_copies(rng, m, k, usable, 64))
    sig_lag, sig_coeff, sig_commit = poly.permutation_key(eng, gl, K.mapping_words(mapping), m, k, usable, DELTA)
    assert sig_lag == cols(K.sigmas_py(mapping, m, k))
    assert sig_commit == [aff(O.scalar_mul(Q.horner(dec(c), s), O.G1)) for c in sig_coeff]


def raw_sigmas(pkg, eng, words, m, k, usable, delta, size, want_lag=True, want_coeff=True):
    """the C call over outputs filled with a pattern -> (status, lagrange bytes, coeff bytes)"""
    lib = pkg.load_library()
    lag = ctypes.create_string_buffer(b"\xa5" * size, size)
    co = ctypes.create_string_buffer(b"\xa5" * size, size)
    arr = None if words is None else (ctypes.c_uint32 * max(len(words) // 4, 1)).from_buffer_copy(words or bytes(4))
    rc = lib.h2agg_permutation_sigmas(eng._ctx, arr, m, k, usable, delta, lag if want_lag else None, co if want_coeff else None)
    return rc, lag.raw, co.raw


def test_invalid_mappings_are_refused_and_the_context_goes_on(eng, pkg, cases):
    m, k, usable = 7, 5, 26
    words, want = cases[(m, k, usable)]
    size = 32 * m << k
    untouched = b"\xa5" * size
    eng.debug_configure("phases", 1)
    try:
        for name, mp, in_range in K.invalid_mappings(random.Random(0xBAD), m, k, usable):
            rc, lag, co = raw_sigmas(pkg, eng, K.mapping_words(mp), m, k, usable, DELTA, size)
            assert rc == pkg.ERR_INVALID, name
            assert lag == untouched and co == untouched, name
            # out-of-range entries never reach the device: the host scan refuses them, and no device phase was timed
            assert ("sigma=" in eng.last_phases()) == in_range, (name, eng.last_phases())
            assert "copy=" not in eng.last_phases(), name
            rc, lag, co = raw_sigmas(pkg, eng, words, m, k, usable, DELTA, size)
            assert rc == pkg.OK and lag == want and co == eng.fr_fft_batch(want, k, inverse=True), name
            assert "copy=" in eng.last_phases()
    finally:
        eng.debug_configure("phases", 0)


def test_sigma_refusals(eng, pkg, cases):
    m, k, usable = 7, 5, 26
    words, want = cases[(m, k, usable)]
    size = 32 * m << k
    untouched = b"\xa5" * size
    calls = [("delta = r", pkg.ERR_NONCANONICAL, dict(delta=R.to_bytes(32, "little"))),
             ("delta = 2^256 - 1", pkg.ERR_NONCANONICAL, dict(delta=b"\xff" * 32)),
             ("m = 0", pkg.ERR_INVALID, dict(m=0)),
             ("m = 4097", pkg.ERR_INVALID, dict(m=4097, k=0, usable=1)),
             ("k = 25", pkg.ERR_INVALID, dict(k=25)),
             ("usable > n", pkg.ERR_INVALID, dict(usable=33)),
             ("both outputs NULL", pkg.ERR_INVALID, dict(want_lag=False, want_coeff=False)),
             ("null mapping", pkg.ERR_INVALID, dict(words=None))]
    for name, code, change in calls:
        args = dict(words=words, m=m, k=k, usable=usable, delta=DELTA, size=size)
        args.update(change)
        rc, lag, co = raw_sigmas(pkg, eng, **args)
        assert rc == code, name
        assert lag == untouched and co == untouched, name
    with pytest.raises(pkg.H2AggError) as ei:
        eng.permutation_sigmas(words, m, k, usable, DELTA, lagrange=False, coeff=False)
    assert ei.value.code == pkg.ERR_INVALID
    with pytest.raises(ValueError):
        eng.permutation_sigmas(words[:-4], m, k, usable, DELTA)
    assert eng.permutation_sigmas(words, m, k, usable, DELTA, coeff=False)[0] == want


def test_commit_refusals(eng, pkg, params):
    k = 5
    _s, _g, gl = params[k]
    good = bytes(32 << k) + fe(7) * (1 << k)   # two columns: zero, and 7 on every row
    for name, code, call in [
            ("unknown handle", pkg.ERR_INVALID, lambda: eng.commit_columns(0xDEAD, good, k)),
            ("table shorter than 2^k", pkg.ERR_INVALID, lambda: eng.commit_columns(gl, bytes(32 << 6), 6)),
            ("m = 0", pkg.ERR_INVALID, lambda: eng.commit_columns(gl, b"", k)),
            ("k = 25", pkg.ERR_INVALID, lambda: eng.commit_columns(gl, good, 25)),
            ("a scalar = r", pkg.ERR_NONCANONICAL, lambda: eng.commit_columns(gl, good[:-32] + R.to_bytes(32, "little"), k))]:
        with pytest.raises(pkg.H2AggError) as ei:
            call()
        assert ei.value.code == code, name
    lib = pkg.load_library()
    out = ctypes.create_string_buffer(64)
    assert lib.h2agg_commit_columns(eng._ctx, gl, None, 1, k, out) == pkg.ERR_INVALID
    assert lib.h2agg_commit_columns(eng._ctx, gl, good, 1, k, None) == pkg.ERR_INVALID
    got = eng.commit_columns(gl, good, k)
    assert got == [eng.g1_batch_to_affine(eng.g1_msm_preloaded(gl, good[j * (32 << k):(j + 1) * (32 << k)])) for j in range(2)]
