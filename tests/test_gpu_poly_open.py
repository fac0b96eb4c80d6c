"""GPU: KZG openings — h2agg_fr_poly_eval / _divide / h2agg_kzg_multiopen (eval_polynomial, kate_division, the GWC multiopen
prover) and poly.py over them.

halo2_proofs is not vendored in the reference, so the yardstick is the definition in include/h2agg.h, evaluated here with
Python integers:  a(z) = sum_i a[i] z^i (Horner);  q[j] = sum_{i>j} a[i] z^(i-j-1), rem = a(z);  and q(X)(X - z) + rem == a(X)
coefficient by coefficient (tests/poly_open_ref.py: quotient_py is the backward recurrence q[j-1] = a[j] + z q[j], which
tests/test_poly_open_host.py ties to the sum as written and the tests here trust).  W is checked in the exponent against a
known trapdoor, and then through the verifier the library already has (batch_multi_open, evaluate_multiopen_proof, the
pairing).  Everything is exact and compared byte for byte.  (The H2AGG_ERR_NOMEM row of the refusals is reached with a polynomial count whose slab cannot be allocated.)"""
import ctypes as C
import importlib
import random

import pytest

import __graft_entry__ as entry
from oracle import bn254 as O
from oracle import pairing as E
from oracle import verifier as V
from tests.fr_bytes import dec, enc, fe
from tests.poly_open_ref import BIG_Z, R, assert_division, horner, quotient_py, random_input

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def poly(pkg):
    return importlib.import_module(entry.PKG_NAME + ".poly")


def inputs(seed, k, t):
    n, T = 1 << k, 1 << t
    out = [random_input(seed, k), [0] * n, [R - 1] * n]
    for pos in sorted({n - 1, T - 1, T, n - T}):
        if 0 <= pos < n:
            a = [0] * n
            a[pos] = 0x1D + pos
            out.append(a)
    return out


def points_for(k, t):
    """0, 1, r - 1, a 254-bit value, w^5 of the domain, and a z with z^T = 1"""
    w = V.omega_for_k(k) if k else 1
    zt = V.omega_for_k(t)
    assert pow(zt, 1 << t, R) == 1 and zt != 1
    return [0, 1, R - 1, BIG_Z, pow(w, 5, R), zt]


def check_eval_and_divide(eng, seed, k, t):
    for a in inputs(seed, k, t):
        data = enc(a)
        zs = points_for(k, t)
        got = dec(eng.fr_poly_eval(data, k, [(0, p) for p in range(len(zs))], enc(zs)))
        assert got == [horner(a, z) for z in zs], (k, t)
        for z in zs:
            quot, rem = eng.fr_poly_divide(data, k, fe(z))
            assert quot == enc(quotient_py(a, z)) and dec(rem) == [horner(a, z)], (k, t, z)
            assert_division(a, z, dec(quot), dec(rem)[0])
            buf = bytearray(data)
            same, rem2 = eng.fr_poly_divide(buf, k, fe(z))                      # out is in
            assert same is buf and bytes(buf) == quot and rem2 == rem


@pytest.mark.parametrize("k", range(0, 13))
def test_eval_and_divide_default_chunk(eng, pkg, k):
    check_eval_and_divide(eng, 200 + k, k, pkg.FR_POLY_CHUNK)


@pytest.mark.parametrize("chunk", [3, 4])
@pytest.mark.parametrize("k", [6, 9, 10])
def test_eval_and_divide_small_chunks(eng, chunk, k):
    try:
        eng.debug_configure("fr_poly_chunk", chunk)
        check_eval_and_divide(eng, 300 + 16 * chunk + k, k, chunk)
    finally:
        eng.debug_configure("fr_poly_chunk", 0)


def test_poly_py_over_the_engine(eng, poly):
    a = random_input(350, 7)
    assert poly.eval_polynomial(eng, enc(a), fe(BIG_Z)) == fe(horner(a, BIG_Z))
    assert poly.kate_division(eng, enc(a), fe(BIG_Z)) == enc(quotient_py(a, BIG_Z)[:-1])


@pytest.mark.parametrize("k,chunk", [(5, 0), (12, 0), (9, 3)])
def test_divide_device_resident(eng, k, chunk):
    import torch
    dev = torch.device("cuda:0")
    a = random_input(400 + k, k)
    data = enc(a)
    z1, z2 = BIG_Z, R - 1
    q1, q2 = enc(quotient_py(a, z1)), enc(quotient_py(a, z2))
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    d_io = d_in.clone()
    d_q1, d_q2, d_q3 = torch.zeros_like(d_in), torch.zeros_like(d_in), torch.zeros_like(d_in)
    d_r1 = torch.zeros(32, dtype=torch.uint8, device=dev)
    d_r2, d_rio = torch.zeros_like(d_r1), torch.zeros_like(d_r1)
    torch.cuda.synchronize()
    try:
        eng.debug_configure("fr_poly_chunk", chunk)
        eng.fr_poly_divide_device(d_in.data_ptr(), k, fe(z1), d_q1.data_ptr(), d_r1.data_ptr())      # distinct buffers
        eng.fr_poly_divide_device(d_in.data_ptr(), k, fe(z2), d_q2.data_ptr(), d_r2.data_ptr())      # another z, queued behind it
        eng.fr_poly_divide_device(d_io.data_ptr(), k, fe(z1), d_io.data_ptr(), d_rio.data_ptr())     # in place
        eng.fr_poly_divide_device(d_in.data_ptr(), k, fe(z2), d_q3.data_ptr(), None)                 # d_rem NULL
        eng.synchronize()
        ev = eng.fr_poly_eval_device(d_in.data_ptr(), 1, k, [(0, 0), (0, 1)], fe(z1) + fe(z2))
    finally:
        eng.debug_configure("fr_poly_chunk", 0)
    assert bytes(d_q1.cpu().numpy()) == q1 and bytes(d_r1.cpu().numpy()) == fe(horner(a, z1))
    assert bytes(d_q2.cpu().numpy()) == q2 and bytes(d_r2.cpu().numpy()) == fe(horner(a, z2))
    assert bytes(d_io.cpu().numpy()) == q1 and bytes(d_rio.cpu().numpy()) == fe(horner(a, z1))
    assert bytes(d_q3.cpu().numpy()) == q2
    assert bytes(d_in.cpu().numpy()) == data, "the device variant changed its input"
    assert ev == fe(horner(a, z1)) + fe(horner(a, z2))


def test_batch_eval_host_and_device_slabs(eng):
    import torch
    k = 9
    polys = [random_input(500 + m, k) for m in range(5)]
    zs = [BIG_Z, 0, random.Random(501).randrange(R)]
    queries = [(4, 2), (0, 0), (3, 1), (1, 2), (0, 0), (2, 2), (4, 0), (1, 1), (3, 0), (2, 1), (0, 2)]   # (0, 0) twice
    assert len(queries) == 11 and len(set(queries)) == 10
    want = enc([horner(polys[m], zs[p]) for m, p in queries])
    slab = b"".join(enc(p) for p in polys)
    assert eng.fr_poly_eval(slab, k, queries, enc(zs)) == want
    d = torch.frombuffer(bytearray(slab), dtype=torch.uint8).to(torch.device("cuda:0"))
    torch.cuda.synchronize()
    assert eng.fr_poly_eval_device(d.data_ptr(), 5, k, queries, enc(zs)) == want
    assert bytes(d.cpu().numpy()) == slab


def test_eval_names_few_of_many_points(eng):
    """20 points (three launches' worth of power tables if all were served), queries at three of them, far apart, and out of
    order; then all 20 named: more than one launch per level"""
    k = 9
    polys = [random_input(520 + m, k) for m in range(2)]
    rng = random.Random(521)
    zs = [rng.randrange(R) for _ in range(20)]
    slab = b"".join(enc(p) for p in polys)
    for queries in ([(1, 17), (0, 2), (1, 9), (0, 17)], [(p % 2, 19 - p) for p in range(20)]):
        assert eng.fr_poly_eval(slab, k, queries, enc(zs)) == enc([horner(polys[m], zs[p]) for m, p in queries])


# ---------------------------------------------------------------------------------------------- multiopen
MO_QUERIES = [(0, 1), (1, 0), (2, 1), (3, 2), (0, 0), (4, 1), (1, 2), (2, 0), (0, 1)]   # 9 queries, 3 points, (0, 1) twice


class Params:
    def __init__(self, eng, k):
        rng = random.Random(0x7A0 + k)
        self.k, self.tau = k, rng.randrange(2, R)
        self.g, self.gl = eng.params_setup(k, fe(self.tau))
        self.polys = [random_input(600 + 8 * k + m, k) for m in range(5)]
        self.slab = b"".join(enc(p) for p in self.polys)
        self.zs = [rng.randrange(R), BIG_Z, rng.randrange(R)]
        self.v = rng.randrange(R)
        self.at_tau = [horner(p, self.tau) for p in self.polys]        # computed once, shared by the tests


@pytest.fixture(scope="module", params=[4, 9])
def params(eng, request):
    p = Params(eng, request.param)
    yield p
    eng.bases_free(p.g)
    eng.bases_free(p.gl)


def expected_ws(par, poly, queries, v, polys=None, at_tau=None):
    """W_g = ((sum_m v^m (p_m(tau) - p_m(z_g))) / (tau - z_g)) * G as canonical affine bytes"""
    polys = par.polys if polys is None else polys
    at_tau = par.at_tau if at_tau is None else at_tau
    out = []
    for pt, members in poly.group_queries(queries):
        z, acc, vm = par.zs[pt], 0, 1
        for m in members:
            acc = (acc + vm * (at_tau[m] - horner(polys[m], z))) % R
            vm = vm * v % R
        d = acc * O.inv((par.tau - z) % R, R) % R
        out.append(O.aff_to_bytes(O.scalar_mul(d, O.G1)) if d else bytes(64))
    return out


def test_multiopen_in_the_exponent(eng, poly, params):
    import torch
    par = params
    want = expected_ws(par, poly, MO_QUERIES, par.v)
    gp, ws = eng.kzg_multiopen(par.g, par.slab, par.k, MO_QUERIES, enc(par.zs), fe(par.v))
    assert gp == [1, 0, 2] and ws == want
    d = torch.frombuffer(bytearray(par.slab), dtype=torch.uint8).to(torch.device("cuda:0"))
    torch.cuda.synchronize()
    gp, ws = eng.kzg_multiopen_device(par.g, d.data_ptr(), 5, par.k, MO_QUERIES, enc(par.zs), fe(par.v))
    assert gp == [1, 0, 2] and ws == want
    assert bytes(d.cpu().numpy()) == par.slab
    try:
        eng.debug_configure("fr_poly_chunk", 3)
        assert eng.kzg_multiopen(par.g, par.slab, par.k, MO_QUERIES, enc(par.zs), fe(par.v)) == ([1, 0, 2], want)
    finally:
        eng.debug_configure("fr_poly_chunk", 0)


def test_multiopen_reports_its_phases(eng, params):
    """debug key phases: the last multiopen's split by events, three non-negative times; the result is unchanged"""
    par = params
    want = eng.kzg_multiopen(par.g, par.slab, par.k, MO_QUERIES, enc(par.zs), fe(par.v))
    try:
        eng.debug_configure("phases", 1)
        assert eng.kzg_multiopen(par.g, par.slab, par.k, MO_QUERIES, enc(par.zs), fe(par.v)) == want
        line = eng.last_phases()
    finally:
        eng.debug_configure("phases", 0)
    fields = [f.split("=") for f in line.split()]
    assert [name for name, _ms in fields] == ["combine", "divide", "commit"], line
    assert all(float(ms) >= 0 for _name, ms in fields), line


@pytest.mark.parametrize("v", [0, 1])
def test_multiopen_trivial_challenges(eng, poly, params, v):
    par = params
    gp, ws = eng.kzg_multiopen(par.g, par.slab, par.k, MO_QUERIES, enc(par.zs), fe(v))
    assert gp == [1, 0, 2] and ws == expected_ws(par, poly, MO_QUERIES, v)


def test_multiopen_zero_combination_is_the_identity(eng, poly, params):
    """p_0 + v p_0 with v = r - 1 is the zero polynomial: its W is the identity, 64 zero bytes; an unused point is ignored"""
    par = params
    queries = [(0, 2), (1, 0), (0, 2), (3, 0)]
    gp, ws = eng.kzg_multiopen(par.g, par.slab, par.k, queries, enc(par.zs), fe(R - 1))
    want = expected_ws(par, poly, queries, R - 1)
    assert gp == [2, 0] and ws == want and ws[0] == bytes(64) and ws[1] != bytes(64)


def test_multiopen_prove_closes_the_loop_through_the_verifier(eng, pkg, poly, params):
    """device commit -> device open -> the library's verifier -> pairing"""
    par = params
    rng = random.Random(0x100B + par.k)
    g2 = b"".join(O.fe_to_bytes(c) for c in (E.G2[0][0], E.G2[0][1], E.G2[1][0], E.G2[1][1]))
    s_g2 = pkg.g2_scalar_mul(g2, fe(par.tau))
    commits = [eng.g1_batch_to_affine(poly.commit_coeff(eng, par.g, enc(p))) for p in par.polys]
    evals, groups, ws = poly.multiopen_prove(eng, par.g, par.slab, par.k, MO_QUERIES, enc(par.zs), fe(par.v))
    assert evals == [fe(horner(par.polys[m], par.zs[p])) for m, p in MO_QUERIES]
    assert groups == poly.group_queries(MO_QUERIES) and ws == expected_ws(par, poly, MO_QUERIES, par.v)
    u = fe(rng.randrange(R))

    def verify(evals, ws):
        b = pkg.SchemaBuilder(eng)
        try:
            nodes = b.evaluation_queries(["p%d" % m for m, _p in MO_QUERIES], b"".join(commits[m] for m, _p in MO_QUERIES),
                                         b"".join(evals))
            w_x, w_g = b.batch_multi_open("loop", [p for _m, p in MO_QUERIES], b"".join(fe(par.zs[p]) for _m, p in MO_QUERIES),
                                          nodes, b"".join(ws), fe(par.v), u)
            left, right, _names = b.evaluate_multiopen_proof(w_x, w_g)
            return eng.final_pair_check(left, right, s_g2, g2)
        finally:
            b.close()

    assert verify(evals, ws)
    bad = list(evals)
    bad[3] = fe(int.from_bytes(bad[3], "little") + 1)
    assert not verify(bad, ws)                                                     # one eval changed by 1
    _gp, other = eng.kzg_multiopen(par.g, par.slab, par.k, MO_QUERIES, enc(par.zs), fe(par.v + 1))
    assert not verify(evals, other)                                                # W made with a different v
    assert not verify(evals, [ws[1], ws[0], ws[2]])                                # two groups' W swapped


def test_refusals_leave_the_context_usable(eng, pkg, params):
    import torch
    par = params
    lib, ctx = eng._lib, eng._ctx
    good = random_input(700, 4)
    zb = fe(BIG_Z)
    good_q, good_r = enc(quotient_py(good, BIG_Z)), fe(horner(good, BIG_Z))
    ws_ok = eng.kzg_multiopen(par.g, par.slab, par.k, MO_QUERIES, enc(par.zs), fe(par.v))

    def still_works():
        assert eng.fr_poly_divide(enc(good), 4, zb) == (good_q, good_r)
        assert eng.fr_poly_eval(enc(good), 4, [(0, 0)], zb) == good_r
        assert eng.kzg_multiopen(par.g, par.slab, par.k, MO_QUERIES, enc(par.zs), fe(par.v)) == ws_ok

    def refused(code, fn, *args):
        with pytest.raises(pkg.H2AggError) as ei:
            fn(*args)
        assert ei.value.code == code, ei.value
        still_works()

    big = R.to_bytes(32, "little")
    zs = enc(par.zs)
    mo = lambda **kw: eng.kzg_multiopen(kw.get("g", par.g), kw.get("slab", par.slab), kw.get("k", par.k),
                                        kw.get("q", MO_QUERIES), kw.get("zs", zs), kw.get("v", fe(par.v)))
    # k > 24
    refused(pkg.ERR_INVALID, eng.fr_poly_eval, bytes(32), 25, [(0, 0)], zb)
    refused(pkg.ERR_INVALID, eng.fr_poly_divide, bytes(32), 25, zb)
    refused(pkg.ERR_INVALID, lambda: mo(k=25))
    # null buffers
    out, rem = C.create_string_buffer(32 * 16), C.create_string_buffer(32)
    q1 = (C.c_uint32 * 2)(0, 0)
    refused(pkg.ERR_INVALID, lambda: eng._check(lib.h2agg_fr_poly_divide(ctx, None, 4, zb, out, rem)))
    refused(pkg.ERR_INVALID, lambda: eng._check(lib.h2agg_fr_poly_divide(ctx, C.cast(out, C.c_void_p), 4, None, out, rem)))
    refused(pkg.ERR_INVALID, lambda: eng._check(lib.h2agg_fr_poly_divide_device(ctx, None, 4, zb, None, None)))
    refused(pkg.ERR_INVALID, lambda: eng._check(lib.h2agg_fr_poly_eval(ctx, C.cast(out, C.c_void_p), 1, 4, q1, 1, zb, 1, None)))
    refused(pkg.ERR_INVALID, lambda: eng._check(lib.h2agg_fr_poly_eval(ctx, C.cast(out, C.c_void_p), 1, 4, None, 1, zb, 1, out)))
    refused(pkg.ERR_INVALID, lambda: eng._check(lib.h2agg_kzg_multiopen(ctx, par.g, None, 5, par.k, q1, 1, zs, 3, zb, out, q1, None)))
    # nq == 0
    refused(pkg.ERR_INVALID, eng.fr_poly_eval, enc(good), 4, [], zb)
    refused(pkg.ERR_INVALID, lambda: mo(q=[]))
    # more queries than one call takes (65535): refused; 65535 themselves are served
    one = fe(0x51)
    assert eng.fr_poly_eval(one, 0, [(0, 0)] * 65535, zb) == one * 65535
    refused(pkg.ERR_INVALID, eng.fr_poly_eval, one, 0, [(0, 0)] * 65536, zb)
    # an index out of range
    refused(pkg.ERR_INVALID, eng.fr_poly_eval, enc(good), 4, [(1, 0)], zb)
    refused(pkg.ERR_INVALID, eng.fr_poly_eval, enc(good), 4, [(0, 1)], zb)
    refused(pkg.ERR_INVALID, lambda: mo(q=MO_QUERIES + [(5, 0)]))
    refused(pkg.ERR_INVALID, lambda: mo(q=MO_QUERIES + [(0, 3)]))
    # a table shorter than 2^k, an unknown table
    refused(pkg.ERR_INVALID, lambda: mo(k=par.k + 1, slab=bytes(5 * (32 << (par.k + 1)))))
    refused(pkg.ERR_INVALID, lambda: mo(g=0xDEAD))
    # a point, z or v >= r
    refused(pkg.ERR_NONCANONICAL, eng.fr_poly_eval, enc(good), 4, [(0, 0)], big)
    refused(pkg.ERR_NONCANONICAL, eng.fr_poly_divide, enc(good), 4, big)
    refused(pkg.ERR_NONCANONICAL, lambda: mo(zs=zs[:32] + big + zs[64:]))
    refused(pkg.ERR_NONCANONICAL, lambda: mo(v=big))
    # a coefficient >= r: from the call for the synchronous entry points
    bad = list(good)
    bad[13] = R
    refused(pkg.ERR_NONCANONICAL, eng.fr_poly_eval, enc(bad), 4, [(0, 0)], zb)
    refused(pkg.ERR_NONCANONICAL, eng.fr_poly_divide, enc(bad), 4, zb)
    bad_slab = bytearray(par.slab)
    bad_slab[32 * 3:32 * 4] = big
    refused(pkg.ERR_NONCANONICAL, lambda: mo(slab=bytes(bad_slab)))
    # ... and at h2agg_synchronize for the queued one, once
    d = torch.frombuffer(bytearray(enc(bad)), dtype=torch.uint8).to(torch.device("cuda:0"))
    d_out = torch.zeros_like(d)
    torch.cuda.synchronize()
    for code, kk, z in ((pkg.ERR_INVALID, 25, zb), (pkg.ERR_NONCANONICAL, 4, big)):
        with pytest.raises(pkg.H2AggError) as ei:
            eng.fr_poly_divide_device(d.data_ptr(), kk, z, d_out.data_ptr(), None)
        assert ei.value.code == code, ei.value
    eng.synchronize()                                                               # nothing was queued, nothing to report
    eng.fr_poly_divide_device(d.data_ptr(), 4, zb, d_out.data_ptr(), None)          # queues; the element >= r is seen on the device
    with pytest.raises(pkg.H2AggError) as ei:
        eng.synchronize()
    assert ei.value.code == pkg.ERR_NONCANONICAL
    eng.synchronize()                                                               # reported once
    still_works()
    # out of memory: 2^30 polynomials of 2^24 coefficients cannot be staged; refused before anything is read
    refused(pkg.ERR_NOMEM, lambda: eng._check(lib.h2agg_fr_poly_eval(ctx, C.cast(out, C.c_void_p), 1 << 30, 24, q1, 1, zb, 1, out)))
