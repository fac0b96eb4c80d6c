"""GPU: Fr column stores — h2agg_columns_create / _destroy / _info / _write / _read / _ptr / _move and the resident forms
h2agg_columns_fft / _commit / _sigmas / _witness_check / _shplonk_begin, with poly.ColumnStore and the resident helpers.

The one yardstick is that the resident path answers byte for byte what the host-buffer path answers (the existing suites hold
the host-buffer path against the Python restatements); the store's own calls are held against Python slices of the bytes
that were written."""
import ctypes as C
import importlib
import random

import pytest

import __graft_entry__ as entry
from oracle import bn254 as O
from tests import honest_prover as HP
from tests import keygen_ref as K
from tests import quotient_ref as Q
from tests.fr_bytes import enc, fe
from tests.grand_product_ref import DELTA
from tests.test_gpu_shplonk import Q_123, rand_points

pytestmark = pytest.mark.gpu

R = Q.R
TAU = random.Random(0xC01).randrange(2, R)


@pytest.fixture(scope="module")
def poly(pkg):
    return importlib.import_module(entry.PKG_NAME + ".poly")


@pytest.fixture(scope="module")
def verifier(pkg):
    return importlib.import_module(entry.PKG_NAME + ".verifier")


@pytest.fixture(scope="module")
def params(eng):
    """(g, g_lagrange) of one trapdoor per k: made once, shared"""
    tables = {k: eng.params_setup(k, fe(TAU)) for k in (5, 7)}
    yield tables
    for g, gl in tables.values():
        eng.bases_free(g)
        eng.bases_free(gl)


@pytest.fixture(scope="module")
def honest(eng, verifier):
    """the honest prover's circuit at k = 5 with its mapping, a theta and its key on the device"""
    class Honest:
        pass
    h = Honest()
    rng = random.Random(0xD00 + 16 * 5 + 4)
    h.circuit = HP.make_circuit(rng, 5, 4)
    h.m = len(h.circuit.cs.permutation_columns)
    h.mapping = K.assembly_py(h.m, 5, h.circuit.usable, h.circuit.copies)
    h.words = K.mapping_words(h.mapping)
    h.flat = [x for cell in h.mapping for x in cell]
    h.theta = rng.randrange(R)
    h.vk = verifier.VerifyingKey(eng, verifier.encode_vk(h.circuit.cs, O.aff_to_bytes))
    yield h
    h.vk.close()


def columns(seed, m, k):
    """m random columns of 2^k canonical elements as one slab"""
    rng = random.Random(seed)
    return b"".join(enc([rng.randrange(R) for _ in range(1 << k)]) for _ in range(m))


def col_of(slab, k, j, count=1):
    return slab[(32 << k) * j:(32 << k) * (j + count)]


def rotated(slab, k, rotation):
    """every column of the slab with row i <- row (i + rotation) mod n"""
    n, out = 1 << k, []
    for at in range(0, len(slab), 32 << k):
        rows = [slab[at + 32 * i:at + 32 * i + 32] for i in range(n)]
        out += [rows[(i + rotation) % n] for i in range(n)]
    return b"".join(out)


class Stores:
    """stores of one test, destroyed behind it"""

    def __init__(self, eng):
        self.eng, self.handles = eng, []

    def __enter__(self):
        return self

    def new(self, m, k, data=None):
        h = self.eng.columns_create(m, k)
        self.handles.append(h)
        if data is not None:
            self.eng.columns_write(h, 0, data)
        return h

    def __exit__(self, *exc):
        for h in self.handles:
            self.eng.columns_destroy(h)


def refused(pkg, fn, code=None):
    with pytest.raises(pkg.H2AggError) as ei:
        fn()
    assert ei.value.code == (pkg.ERR_INVALID if code is None else code)


# ---------------------------------------------------------------------------------------------- the store itself
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("k", [0, 1, 5])
def test_create_info_write_read(eng, k, m):
    with Stores(eng) as st:
        h = st.new(m, k)
        assert eng.columns_info(h) == (m, k)
        assert eng.columns_read(h, 0, m) == bytes((32 << k) * m), "zero-filled"
        data = columns(0xA00 + 8 * k + m, m, k)
        eng.columns_write(h, 0, data)
        assert eng.columns_read(h, 0, m) == data
        # partial ranges at both ends of the slab
        first, last = columns(1, 1, k), columns(2, 1, k)
        eng.columns_write(h, m - 1, last)
        eng.columns_write(h, 0, first)
        want = bytearray(data)
        want[(32 << k) * (m - 1):] = last
        want[:32 << k] = first
        assert eng.columns_read(h, 0, m) == bytes(want)
        assert eng.columns_read(h, m - 1, 1) == col_of(bytes(want), k, m - 1) and eng.columns_read(h, 0, 1) == first
        if m == 3:
            assert eng.columns_read(h, 1, 2) == col_of(bytes(want), k, 1, 2) and eng.columns_read(h, 0, 2) == col_of(bytes(want), k, 0, 2)


def test_two_stores_alive_then_destroyed(pkg, eng):
    a, b = eng.columns_create(2, 5), eng.columns_create(3, 1)
    assert a != b and a and b
    da, db = columns(3, 2, 5), columns(4, 3, 1)
    eng.columns_write(a, 0, da)
    eng.columns_write(b, 0, db)
    assert eng.columns_read(a, 0, 2) == da and eng.columns_read(b, 0, 3) == db
    eng.columns_destroy(a)
    refused(pkg, lambda: eng.columns_info(a))
    refused(pkg, lambda: eng.columns_destroy(a))
    assert eng.columns_read(b, 0, 3) == db
    eng.columns_destroy(b)
    refused(pkg, lambda: eng.columns_read(b, 0, 1))


@pytest.mark.parametrize("column", [0, 2])
@pytest.mark.parametrize("row", [0, 31])
def test_write_checks_every_element_against_r(pkg, eng, column, row):
    k, m = 5, 3
    with Stores(eng) as st:
        good = columns(5, m, k)
        h = st.new(m, k, good)
        at = (32 << k) * column + 32 * row
        for value, ok in ((R - 1, True), (R, False), ((1 << 256) - 1, False)):
            data = bytearray(columns(6, m, k))
            data[at:at + 32] = value.to_bytes(32, "little")
            if ok:
                eng.columns_write(h, 0, bytes(data))
                assert eng.columns_read(h, 0, m) == bytes(data)
            else:
                refused(pkg, lambda: eng.columns_write(h, 0, bytes(data)), pkg.ERR_NONCANONICAL)
                eng.synchronize()                                   # the context is usable, nothing is left pending
                eng.columns_write(h, 0, good)                       # the next call is fine
                assert eng.columns_read(h, 0, m) == good


# ---------------------------------------------------------------------------------------------- columns_move
ROTATIONS = [0, 1, -1, 31, 32, -35, (1 << 31) - 1]      # n = 32: n - 1, n, -n - 3


@pytest.mark.parametrize("rotation", ROTATIONS)
def test_move_between_two_stores_and_within_one(eng, rotation):
    k = 5
    src = columns(7, 4, k)
    with Stores(eng) as st:
        a, b = st.new(4, k, src), st.new(3, k, columns(8, 3, k))
        eng.columns_move(a, 1, b, 0, 2, rotation)
        got = eng.columns_read(b, 0, 3)
        assert got[:(32 << k) * 2] == rotated(col_of(src, k, 1, 2), k, rotation)
        assert col_of(got, k, 2) == col_of(columns(8, 3, k), k, 2), "the column behind the range is untouched"
        eng.columns_move(a, 0, a, 2, 2, rotation)        # disjoint ranges of one store
        assert eng.columns_read(a, 0, 4) == col_of(src, k, 0, 2) + rotated(col_of(src, k, 0, 2), k, rotation)


@pytest.mark.parametrize("rotation", [1, -300])
def test_move_over_more_than_one_workgroup(eng, rotation):
    k = 11                                               # 4096 units of 16 bytes per column: four workgroups, the wrap inside one
    src = columns(9, 2, k)
    with Stores(eng) as st:
        a, b = st.new(2, k, src), st.new(2, k)
        eng.columns_move(a, 0, b, 0, 2, rotation)
        assert eng.columns_read(b, 0, 2) == rotated(src, k, rotation)
        assert eng.columns_read(a, 0, 2) == src


def test_move_overlaps(pkg, eng):
    k = 5
    src = columns(10, 4, k)
    with Stores(eng) as st:
        a, b = st.new(4, k, src), st.new(4, 4)
        eng.columns_move(a, 1, a, 1, 2, 0)               # the legal no-op
        eng.columns_move(a, 1, a, 1, 2, 32)
        eng.columns_move(a, 0, a, 0, 4, -64)
        refused(pkg, lambda: eng.columns_move(a, 1, a, 1, 2, 1))      # the same range, rotated
        refused(pkg, lambda: eng.columns_move(a, 0, a, 1, 2, 0))      # partial overlaps, either way round
        refused(pkg, lambda: eng.columns_move(a, 1, a, 0, 2, 0))
        refused(pkg, lambda: eng.columns_move(a, 0, a, 1, 3, 5))
        refused(pkg, lambda: eng.columns_move(a, 0, b, 0, 1, 0))      # k = 5 into k = 4
        assert eng.columns_read(a, 0, 4) == src


# ---------------------------------------------------------------------------------------------- columns_fft
@pytest.mark.parametrize("m", [1, 3, 5])
@pytest.mark.parametrize("k,local", [(5, 0), (11, 0), (7, 3)])          # one pass; two passes; three passes
def test_fft_equals_the_host_buffer_batch(eng, poly, k, local, m):
    data = columns(0xF00 + 16 * k + m, m, k)
    edge = columns(11, 2, k)
    eng.debug_configure("fr_fft_local", local)
    eng.debug_configure("fr_fft_batch_chunk", 2)         # a chunk boundary inside the in-place transform for m = 3, 5
    try:
        with Stores(eng) as st:
            for inverse, shift in ((False, None), (True, None), (False, poly.ZETA), (True, poly.ZETA)):
                want = eng.fr_fft_batch(data, k, inverse, shift)
                a = st.new(m, k, data)
                eng.columns_fft(a, 0, a, 0, m, inverse, shift)               # in place
                assert eng.columns_read(a, 0, m) == want
                # store to store, into the middle of a larger store
                b = st.new(m + 2, k)
                eng.columns_write(b, 0, col_of(edge, k, 0))
                eng.columns_write(b, m + 1, col_of(edge, k, 1))
                eng.columns_write(a, 0, data)
                eng.columns_fft(a, 0, b, 1, m, inverse, shift)
                assert eng.columns_read(b, 0, m + 2) == col_of(edge, k, 0) + want + col_of(edge, k, 1)
                assert eng.columns_read(a, 0, m) == data
    finally:
        eng.debug_configure("fr_fft_local", 0)
        eng.debug_configure("fr_fft_batch_chunk", 0)


def test_fft_within_one_store_and_its_overlaps(pkg, eng, poly):
    k = 5
    data = columns(12, 5, k)
    with Stores(eng) as st:
        a = st.new(5, k, data)
        eng.columns_fft(a, 0, a, 3, 2)                   # disjoint ranges of one store
        assert eng.columns_read(a, 0, 5) == col_of(data, k, 0, 3) + eng.fr_fft_batch(col_of(data, k, 0, 2), k)
        refused(pkg, lambda: eng.columns_fft(a, 0, a, 1, 2))
        refused(pkg, lambda: eng.columns_fft(a, 2, a, 1, 3))
        refused(pkg, lambda: eng.columns_fft(a, 0, a, 0, 2, False, bytes(32)))       # the family's own refusals
        refused(pkg, lambda: eng.columns_fft(a, 0, a, 0, 2, False, fe(R - 1)[:31] + b"\xff"), pkg.ERR_NONCANONICAL)
        v = poly.ColumnStore(eng, 5, k, handle=a).view(1, 2)
        assert poly.resident_lagrange_to_coeff(eng, v).read() == poly.columns_lagrange_to_coeff(eng, [col_of(data, k, 1), col_of(data, k, 2)], k)
        with pytest.raises(ValueError):
            poly.resident_coeff_to_lagrange(eng, v, v.store.view(2, 2))


# ---------------------------------------------------------------------------------------------- columns_commit
@pytest.mark.parametrize("chunk", [0, 1])
@pytest.mark.parametrize("m", [1, 4])
@pytest.mark.parametrize("k", [5, 7])
def test_commit_equals_the_host_buffer_call(eng, poly, params, k, m, chunk):
    g, gl = params[k]
    data = bytearray(columns(0xC00 + 8 * k + m, m, k))
    data[(32 << k) * (m - 1):] = bytes(32 << k)          # the last column is all zero: the identity
    data = bytes(data)
    eng.debug_configure("commit_chunk", chunk)
    try:
        with Stores(eng) as st:
            a = st.new(m + 1, k)
            eng.columns_write(a, 1, data)
            for table in (g, gl):
                want = eng.commit_columns(table, data, k)
                assert eng.columns_commit(table, a, 1, m) == want
                assert want[m - 1] == bytes(64)
            view = poly.ColumnStore(eng, m + 1, k, handle=a).view(1, m)
            assert poly.resident_commit_columns_lagrange(eng, gl, view) == eng.commit_columns(gl, data, k)
            assert poly.resident_commit_columns_coeff(eng, g, view) == eng.commit_columns(g, data, k)
    finally:
        eng.debug_configure("commit_chunk", 0)


# ---------------------------------------------------------------------------------------------- columns_sigmas
def test_sigmas_equal_the_host_buffer_call(pkg, eng, poly, params, honest):
    k, m, u = 5, honest.m, honest.circuit.usable
    lag, coeff = eng.permutation_sigmas(honest.words, m, k, u, fe(DELTA))
    edge = columns(13, 2, k)
    with Stores(eng) as st:
        a, b = st.new(m + 2, k), st.new(m, k)
        eng.columns_write(a, 0, col_of(edge, k, 0))
        eng.columns_write(a, m + 1, col_of(edge, k, 1))
        eng.columns_sigmas(honest.words, m, k, u, fe(DELTA), a, 1, b, 0)
        assert eng.columns_read(a, 0, m + 2) == col_of(edge, k, 0) + lag + col_of(edge, k, 1)
        assert eng.columns_read(b, 0, m) == coeff
        # either output absent
        c, d = st.new(m, k), st.new(m, k)
        eng.columns_sigmas(honest.words, m, k, u, fe(DELTA), c, 0)
        eng.columns_sigmas(honest.words, m, k, u, fe(DELTA), 0, 0, d, 0)
        assert eng.columns_read(c, 0, m) == lag and eng.columns_read(d, 0, m) == coeff
        refused(pkg, lambda: eng.columns_sigmas(honest.words, m, k, u, fe(DELTA)))
        refused(pkg, lambda: eng.columns_sigmas(honest.words, m, k, u, fe(DELTA), c, 0, c, 0))
        # a mapping that is no bijection: cell (0, 1) takes the target of cell (0, 0)
        bad = list(honest.flat)
        assert bad[0:2] != bad[2:4]
        bad[2:4] = bad[0:2]
        refused(pkg, lambda: eng.permutation_sigmas(bad, m, k, u, fe(DELTA)))
        before = (eng.columns_read(a, 0, m + 2), eng.columns_read(b, 0, m))
        refused(pkg, lambda: eng.columns_sigmas(bad, m, k, u, fe(DELTA), a, 1, b, 0))
        assert (eng.columns_read(a, 0, m + 2), eng.columns_read(b, 0, m)) == before, "a refused mapping leaves both stores unchanged"
    gl = params[k][1]
    s_lag, s_coeff, commits = poly.resident_permutation_key(eng, gl, honest.words, m, k, u, fe(DELTA))
    try:
        w_lag, w_coeff, w_commits = poly.permutation_key(eng, gl, honest.words, m, k, u, fe(DELTA))
        assert (s_lag.read(), s_coeff.read(), commits) == (w_lag, w_coeff, w_commits)
    finally:
        s_lag.close()
        s_coeff.close()


# ---------------------------------------------------------------------------------------------- columns_witness_check
@pytest.mark.parametrize("witness", ["honest", "gate cell", "copied cell", "outside the table"])
def test_witness_check_equals_the_host_buffer_call(eng, poly, honest, witness):
    c = {"honest": lambda c: c, "gate cell": HP.broken_gate_cell, "copied cell": HP.broken_copied_cell,
         "outside the table": HP.outside_the_table}[witness](honest.circuit)
    lag = {kind: [enc(col) for col in c.lag[kind]] for kind in ("advice", "fixed", "instance")}
    want = poly.witness_check(eng, honest.vk, lag["advice"], lag["fixed"], lag["instance"], [], theta=fe(honest.theta), mapping=honest.words)
    assert want.ok == (witness == "honest")
    with poly.ColumnStore(eng, 8, 5) as st:              # one spare column in front: the slabs start at 1, 4 and 7
        st.write(1, lag["advice"] + lag["fixed"] + lag["instance"])
        got = poly.resident_witness_check(eng, honest.vk, st.view(1, 3), st.view(4, 3), st.view(7, 1), [], theta=fe(honest.theta),
                                          mapping=honest.words)
        assert (got.layout, got.counts, got.first_rows, got.rows, got.total) == (want.layout, want.counts, want.first_rows, want.rows, want.total)
        assert got.failures == want.failures and got.ok == want.ok
        raw = eng.columns_witness_check(honest.vk, 7, (st.handle, 1), (st.handle, 4), (st.handle, 7), None, fe(honest.theta), honest.words, 4)
        assert raw == eng.witness_check(honest.vk, 7, b"".join(lag["advice"]), b"".join(lag["fixed"]), b"".join(lag["instance"]), None,
                                        fe(honest.theta), honest.words, 4)


# ---------------------------------------------------------------------------------------------- columns_shplonk_begin
def test_shplonk_over_a_store_that_is_overwritten_before_finish(eng, poly, params):
    k, npoly = 5, 8
    g = params[k][0]
    slab = columns(14, npoly, k)
    queries, points = Q_123, enc(rand_points(11, 6))     # sets of 1, 2 and 3 points
    assert sorted(len(pts) for pts, _polys in poly.shplonk_sets(queries)) == [1, 2, 3]
    rng = random.Random(15)
    y, v, u = fe(rng.randrange(R)), fe(rng.randrange(R)), fe(rng.randrange(R))
    evals, h1, h2 = poly.shplonk_prove(eng, g, slab, k, queries, points, y, v, lambda _h1: u)
    with poly.ColumnStore(eng, npoly + 1, k) as st:
        st.write(1, slab)
        got1, obj = eng.columns_shplonk_begin(g, st.handle, 1, npoly, queries, points, b"".join(evals), y, v)
        try:
            st.write(0, columns(16, npoly + 1, k))       # the store changes between the rounds
            got2 = eng.kzg_shplonk_finish(obj, u)
        finally:
            eng.kzg_shplonk_destroy(obj)
        assert (got1, got2) == (h1, h2)
        st.write(1, slab)
        assert poly.resident_shplonk_prove(eng, g, st.view(1, npoly), queries, points, y, v, lambda _h1: u) == (evals, h1, h2)


# ---------------------------------------------------------------------------------------------- columns_ptr
def test_the_device_entry_points_run_over_store_pointers(eng, poly, verifier):
    k = 5
    cs, _lag, polys, sc = Q.satisfied_circuit(random.Random(0xD00 + k), k, 4)
    vk = verifier.VerifyingKey(eng, verifier.encode_vk(cs, O.aff_to_bytes))
    try:
        slabs = [[enc(c) for c in polys[kind]] for kind in Q.POLY_KINDS]
        scalars = [fe(sc[s]) for s in ("theta", "beta", "gamma", "y", "delta")]
        want = poly.quotient_pieces(eng, vk, *slabs, [], *scalars)
        total = sum(len(s) for s in slabs)
        with poly.ColumnStore(eng, total + len(want), k) as st:
            ptrs, at = [], 0
            for s in slabs:
                st.write(at, s)
                ptrs.append(st.ptr(at))
                at += len(s)
            assert ptrs[1] == ptrs[0] + (32 << k) * len(slabs[0]), "columns follow one another at 32 * 2^k bytes"
            eng.quotient_device(vk, *ptrs, None, *scalars, st.ptr(total))
            assert st.read(total, len(want)) == want
            points = enc(rand_points(17, 2))
            queries = [(0, 0), (total - 1, 1), (3, 1), (total, 0)]
            everything = b"".join(b"".join(s) for s in slabs) + b"".join(want)
            assert eng.fr_poly_eval_device(st.ptr(0), total + len(want), k, queries, points) == \
                eng.fr_poly_eval(everything, k, queries, points)
    finally:
        vk.close()


# ---------------------------------------------------------------------------------------------- one proof, every column resident
@pytest.mark.parametrize("k", [7, 12])
def test_a_proof_with_every_column_resident(pkg, eng, poly, verifier, k):
    from tests.resident_prover import ResidentStages
    from tests.test_gpu_honest_proofs import TAU as PROOF_TAU, device_prove, verdicts
    setup = HP.Setup(k, PROOF_TAU, HP.INSTANCE_ROWS)
    circuit = HP.make_circuit(random.Random(0xD00 + 16 * k + 4), k, 4)
    want = device_prove(pkg, eng, poly, verifier, setup, circuit)
    stages = ResidentStages(pkg, eng, poly, verifier, setup)
    try:
        got = HP.prove(circuit, setup, stages, random.Random(1))
        assert stages.moves > stages.writes > 0, "most columns a stage is handed are in the store already"
    finally:
        stages.close()
    assert HP.first_difference(got, want) is None, "first differing field: %s" % HP.first_difference(got, want)
    assert got.data == want.data and got.cs.vk_scalar == want.cs.vk_scalar
    each, agg = verdicts(eng, verifier, {k: setup}, [[got]])
    assert [(s, ok) for _pair, s, ok in each] == [(0, True)] and agg is True


# ---------------------------------------------------------------------------------------------- the common refusals
def entry_points(eng, honest, g, a, b5, null=False):
    """every entry point that takes a store, as (name, call(handle, first, count)); a: a store of 8 columns at k = 5"""
    m, u, one = honest.m, honest.circuit.usable, fe(1)
    buf = None if null else C.create_string_buffer((32 << 5) * 8)
    lib, ctx, check = eng._lib, eng._ctx, eng._check
    queries = (C.c_uint32 * 2)(0, 0)
    words = (C.c_uint32 * len(honest.flat))(*honest.flat)
    counts, first, total = (C.c_uint32 * 10)(), (C.c_uint32 * 10)(), C.c_uint64()
    obj = C.c_void_p()

    def wc(which):
        def call(h, f, _n):
            places = [a, 0, a, 3, a, 6]
            places[2 * which:2 * which + 2] = [h, f]
            check(lib.h2agg_columns_witness_check(ctx, honest.vk._vk, 7, *places, None, fe(honest.theta), words, 0, counts, first, None,
                                                  None if null else C.byref(total)))
        return call
    return [
        ("info", lambda h, f, n: eng.columns_info(h)),
        ("destroy", lambda h, f, n: eng.columns_destroy(h)),
        ("write", lambda h, f, n: check(lib.h2agg_columns_write(ctx, h, f, n, buf))),
        ("read", lambda h, f, n: check(lib.h2agg_columns_read(ctx, h, f, n, buf))),
        ("ptr", lambda h, f, n: check(lib.h2agg_columns_ptr(ctx, h, f, None if null else C.byref(C.c_void_p())))),
        ("move from", lambda h, f, n: eng.columns_move(h, f, b5, 0, n, 1)),
        ("move to", lambda h, f, n: eng.columns_move(b5, 0, h, f, n, 1)),
        ("fft from", lambda h, f, n: eng.columns_fft(h, f, b5, 0, n)),
        ("fft to", lambda h, f, n: eng.columns_fft(b5, 0, h, f, n)),
        ("commit", lambda h, f, n: check(lib.h2agg_columns_commit(ctx, g, h, f, n, buf))),
        ("sigmas lagrange", lambda h, f, n: check(lib.h2agg_columns_sigmas(ctx, None if null else words, m, 5, u, fe(DELTA), h, f, 0, 0))),
        ("sigmas coeff", lambda h, f, n: check(lib.h2agg_columns_sigmas(ctx, None if null else words, m, 5, u, fe(DELTA), 0, 0, h, f))),
        ("witness_check advice", wc(0)), ("witness_check fixed", wc(1)), ("witness_check instance", wc(2)),
        ("shplonk_begin", lambda h, f, n: check(lib.h2agg_columns_shplonk_begin(ctx, g, h, f, n, queries, 1, one, 1, None if null else bytes(32),
                                                                                one, one, buf, C.byref(obj)))),
    ]


# what each entry point's count is (the others take it from the call): the range tests put `first` beyond the store for those
FIXED_COUNT = {"info", "destroy", "ptr", "sigmas lagrange", "sigmas coeff", "witness_check advice", "witness_check fixed",
               "witness_check instance"}


def test_common_refusals_once_per_entry_point(pkg, eng, params, honest):
    g = params[5][0]
    data = columns(18, 8, 5)
    with Stores(eng) as st:
        a, b5, b4 = st.new(8, 5, data), st.new(8, 5), st.new(8, 4)
        gone = eng.columns_create(8, 5)
        eng.columns_destroy(gone)
        for name, call in entry_points(eng, honest, g, a, b5):
            refused(pkg, lambda: call(0xDEAD, 0, 1))                 # an unknown handle
            refused(pkg, lambda: call(gone, 0, 1))                   # a destroyed one
            refused(pkg, lambda: call(g, 0, 1))                      # a base table's handle names no store
            if name in ("info", "destroy"):
                continue
            refused(pkg, lambda: call(a, 8, 1))                      # first + count beyond m
            if name not in FIXED_COUNT:
                refused(pkg, lambda: call(a, 7, 2))
                refused(pkg, lambda: call(a, 0, 9))
                refused(pkg, lambda: call(a, 0, 0))                  # count == 0
                refused(pkg, lambda: call(a, 1, (1 << 64) - 1))      # first + count wraps
            elif name not in ("ptr", "witness_check instance"):
                refused(pkg, lambda: call(a, 6, 0))                  # the call's own count (7 sigma columns; 3 advice, 3 fixed) from column 6
            if name.startswith(("move", "fft", "sigmas", "witness_check")):
                refused(pkg, lambda: call(b4, 0, 1))                 # a store of another k than the call's, the other store's or the key's
        for name, call in entry_points(eng, honest, g, a, b5, null=True):
            if name in ("write", "read", "ptr", "commit", "sigmas lagrange", "sigmas coeff", "witness_check advice", "shplonk_begin"):
                refused(pkg, lambda: call(a, 0, 1))                  # a null host buffer
        refused(pkg, lambda: eng.columns_create(0, 5))
        refused(pkg, lambda: eng.columns_create(1, 25))
        refused(pkg, lambda: eng._check(eng._lib.h2agg_columns_create(eng._ctx, 1, 5, None)))
        refused(pkg, lambda: eng.columns_create(1 << 59, 24), pkg.ERR_NOMEM)      # 2^88 bytes: refused before the allocator
        # nothing was written, and the context goes on
        assert eng.columns_read(a, 0, 8) == data and eng.columns_read(b5, 0, 8) == bytes((32 << 5) * 8)
        eng.columns_fft(a, 0, b5, 0, 8)
        assert eng.columns_read(b5, 0, 8) == eng.fr_fft_batch(data, 5)
