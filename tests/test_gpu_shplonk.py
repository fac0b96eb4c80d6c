"""GPU: the Shplonk multiopen prover — h2agg_kzg_shplonk_begin / _finish / _destroy and poly.shplonk_prove /
poly.shplonk_final_pair over them.

halo2_proofs is not vendored in the reference, so the yardstick is the definition in include/h2agg.h, evaluated with Python
integers (tests/shplonk_ref.py, which tests/test_shplonk_host.py ties together).  H1 and H2 are checked in the exponent
against a known trapdoor tau — H1 = h(tau) G, H2 = h2(tau) G with h(tau) = sum_i v^i N_i(tau) / Z_{S_i}(tau) and
h2(tau) = L(tau) / (tau - u) from the values p(tau) — byte for byte, and then through the pairing the library already has.
At k = 6 the reference's h is computed coefficient by coefficient and committed under two different tau: the object exposes
no read-back of h, and two evaluations of a difference of degree < 64 that both vanish by chance have probability 2^-500."""
import ctypes as C
import importlib
import random

import pytest

import __graft_entry__ as entry
from oracle import bn254 as O
from oracle import pairing as E
from oracle import verifier as V
from tests import shplonk_ref as S
from tests.fr_bytes import enc, fe
from tests.poly_open_ref import BIG_Z, R, horner, random_input

pytestmark = pytest.mark.gpu

NPOLY = 8


@pytest.fixture(scope="module")
def poly(pkg):
    return importlib.import_module(entry.PKG_NAME + ".poly")


class Params:
    """parameters with a known trapdoor (h2agg_params_setup), polynomials and their values at tau: made once per k"""

    def __init__(self, eng, k, seed=0, polys=None):
        rng = random.Random(0x5B00 + 64 * seed + k)
        self.eng, self.k, self.tau = eng, k, rng.randrange(2, R)
        self.g, self.gl = eng.params_setup(k, fe(self.tau))
        self.polys = [random_input(900 + 16 * k + m, k) for m in range(NPOLY)] if polys is None else polys
        self.slab = b"".join(enc(p) for p in self.polys)
        self.at_tau = [horner(p, self.tau) for p in self.polys]
        self.y, self.v, self.u = rng.randrange(R), rng.randrange(R), rng.randrange(R)

    def free(self):
        self.eng.bases_free(self.g)
        self.eng.bases_free(self.gl)


@pytest.fixture(scope="module", params=[4, 9])
def params(eng, request):
    p = Params(eng, request.param)
    yield p
    p.free()


def point(d):
    return O.aff_to_bytes(O.scalar_mul(d % R, O.G1)) if d % R else bytes(64)


def in_the_exponent(op, at_tau, tau, u):
    """(h(tau), h2(tau)) from the values p(tau): no polynomial arithmetic"""
    h1, vi = 0, 1
    for i, (pts, members) in enumerate(op.sets):
        n_tau, yj = 0, 1
        for j, m in enumerate(members):
            n_tau = (n_tau + yj * (at_tau[m] - S.horner(op.r[i][j], tau))) % R
            yj = yj * op.y % R
        h1 = (h1 + vi * n_tau * S.inv(op.z_at(pts, tau))) % R
        vi = vi * op.v % R
    if u is None:
        return h1, None
    _d, c, t = op.scalars(u)
    L, vi = 0, 1
    for i, (_pts, members) in enumerate(op.sets):
        w = vi * c[i] % R
        for j, m in enumerate(members):
            L = (L + w * (at_tau[m] - S.horner(op.r[i][j], u))) % R
            w = w * op.y % R
        vi = vi * op.v % R
    L = (L - t * h1) % R
    return h1, L * S.inv(tau - u) % R


def prove(eng, par, queries, zs, y, v, us, evals=None):
    """begin, finish for every u of `us`, destroy -> (H1, [H2, ...])"""
    ev = eng.fr_poly_eval(par.slab, par.k, queries, enc(zs)) if evals is None else evals
    h1, obj = eng.kzg_shplonk_begin(par.g, par.slab, par.k, queries, enc(zs), ev, fe(y), fe(v))
    try:
        return h1, [eng.kzg_shplonk_finish(obj, fe(u)) for u in us]
    finally:
        eng.kzg_shplonk_destroy(obj)
        assert not obj


def check_in_the_exponent(eng, par, queries, zs, y=None, v=None, u=None):
    y = par.y if y is None else y
    v = par.v if v is None else v
    u = par.u if u is None else u
    op = S.Opening(par.polys, zs, queries, y, v)
    want1, want2 = in_the_exponent(op, par.at_tau, par.tau, u)
    h1, (h2,) = prove(eng, par, queries, zs, y, v, [u])
    assert h1 == point(want1), "H1"
    assert h2 == point(want2), "H2"
    return h1, h2


def rand_points(seed, count):
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(count)]


Q_123 = [(0, 0), (1, 1), (2, 3), (1, 2), (3, 0), (2, 4), (4, 2), (2, 5), (4, 1), (5, 5), (5, 3), (0, 0), (5, 4), (6, 1), (6, 2)]


def case_points(name, k, t):
    """queries and point values of the named case; t: log2 of the chunk in force"""
    w = V.omega_for_k(k)
    if name == "one_set_one_point":
        return [(0, 0), (1, 0), (2, 0)], [BIG_Z]
    if name == "sets_of_1_2_3":
        return Q_123, rand_points(11, 6)
    if name == "sets_of_5_and_8":
        q = [(0, p) for p in range(5)] + [(1, p) for p in range(5, 13)] + [(2, p) for p in (4, 3, 2, 1, 0)] + [(3, 12)]
        return q, rand_points(12, 13)
    if name == "set_of_32":                     # eight rounds of four chains; at k = 4 more points than coefficients
        return [(0, p) for p in range(32)] + [(1, 0), (2, 31), (2, 7)], rand_points(17, 32)
    if name == "every_polynomial_its_own_set":
        return [(0, 0), (1, 1), (2, 0), (2, 1), (3, 2), (4, 1), (4, 2), (5, 0), (5, 2)], rand_points(13, 3)
    if name == "repeated_pairs":
        return [(0, 1), (0, 1), (1, 1), (0, 2), (1, 2), (0, 1), (2, 0), (2, 0)], rand_points(14, 3)
    if name == "points_0_1_minus_1":
        return [(0, 0), (0, 1), (0, 2), (1, 1), (2, 0), (2, 2), (3, 2), (3, 0)], [0, 1, R - 1]
    if name == "omega_related":
        x = rand_points(15, 1)[0]
        return [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (2, 1), (3, 2), (3, 0), (3, 1)], [x, x * w % R, x * S.inv(w) % R]
    if name == "root_of_the_chunk":
        zt = V.omega_for_k(t)
        assert pow(zt, 1 << t, R) == 1 and zt != 1
        return [(0, 0), (0, 1), (1, 0), (2, 1), (2, 0), (3, 2), (3, 0), (3, 1)], [zt, zt * zt % R, rand_points(16, 1)[0]]
    raise KeyError(name)


CASES = ["one_set_one_point", "sets_of_1_2_3", "sets_of_5_and_8", "set_of_32", "every_polynomial_its_own_set", "repeated_pairs",
         "points_0_1_minus_1", "omega_related", "root_of_the_chunk"]


@pytest.mark.parametrize("name", CASES)
def test_h1_and_h2_in_the_exponent(eng, pkg, params, name):
    par = params
    queries, zs = case_points(name, par.k, pkg.FR_POLY_CHUNK)
    h1, _h2 = check_in_the_exponent(eng, par, queries, zs)
    if name == "one_set_one_point":     # N_0 / (X - z) is the GWC combination under y: H1 is that group's W
        gp, ws = eng.kzg_multiopen(par.g, par.slab, par.k, queries, enc(zs), fe(par.y))
        assert gp == [0] and ws == [h1]


@pytest.mark.parametrize("k", [9, 10])
def test_small_chunks_give_the_same_points(eng, k):
    """fr_poly_chunk = 3: three (k = 9) and four (k = 10) sweep levels at 8 coefficients per chunk"""
    par = Params(eng, k, seed=1)
    try:
        for name in ("sets_of_1_2_3", "sets_of_5_and_8"):
            queries, zs = case_points(name, k, 3)
            want = prove(eng, par, queries, zs, par.y, par.v, [par.u])
            try:
                eng.debug_configure("fr_poly_chunk", 3)
                assert check_in_the_exponent(eng, par, queries, zs) == (want[0], want[1][0]), name
            finally:
                eng.debug_configure("fr_poly_chunk", 0)
        queries, zs = case_points("root_of_the_chunk", k, 3)
        try:
            eng.debug_configure("fr_poly_chunk", 3)
            check_in_the_exponent(eng, par, queries, zs)
        finally:
            eng.debug_configure("fr_poly_chunk", 0)
    finally:
        par.free()


def test_quotient_coefficients_at_k6(eng):
    """k = 6, chunks of 8 (one level above the coefficients) and the default: the device's h against the reference's,
    coefficient by coefficient, through commitments under two tau; single non-zero coefficients at n - 1, T - 1, T, n - T,
    all r - 1, all zero"""
    k, n, T = 6, 64, 8
    polys = []
    for pos in (n - 1, T - 1, T, n - T):
        a = [0] * n
        a[pos] = 0x1D + pos
        polys.append(a)
    polys += [[R - 1] * n, [0] * n, random_input(960, k), random_input(961, k)]
    queries, zs = Q_123 + [(7, 3), (7, 4), (7, 5)], rand_points(21, 6)
    pars = [Params(eng, k, seed=2 + s, polys=polys) for s in range(2)]
    try:
        op = S.Opening(polys, zs, queries, pars[0].y, pars[0].v)
        h = op.h()
        h2, rem = op.h2(pars[0].u)
        assert rem == 0
        for chunk in (3, 0):
            for par in pars:
                assert par.tau != pars[0].tau or par is pars[0]
                try:
                    eng.debug_configure("fr_poly_chunk", chunk)
                    got1, (got2,) = prove(eng, par, queries, zs, pars[0].y, pars[0].v, [pars[0].u])
                finally:
                    eng.debug_configure("fr_poly_chunk", 0)
                assert got1 == point(horner(h, par.tau)), (chunk, "H1")
                assert got2 == point(horner(h2, par.tau)), (chunk, "H2")
        # the zero polynomial alone: both points are the identity
        for chunk in (3, 0):
            try:
                eng.debug_configure("fr_poly_chunk", chunk)
                got1, (got2,) = prove(eng, pars[0], [(5, 0), (5, 1)], zs, 3, 5, [7])
            finally:
                eng.debug_configure("fr_poly_chunk", 0)
            assert got1 == bytes(64) and got2 == bytes(64)
    finally:
        for par in pars:
            par.free()


@pytest.mark.parametrize("which,value", [(w, x) for w in "yvu" for x in (0, 1)])
def test_trivial_challenges(eng, params, which, value):
    queries, zs = case_points("sets_of_1_2_3", params.k, 0)
    check_in_the_exponent(eng, params, queries, zs, **{which: value})


def test_u_in_the_first_set(eng, params):
    queries, zs = case_points("sets_of_1_2_3", params.k, 0)
    check_in_the_exponent(eng, params, queries, zs, u=zs[0])


def test_finish_twice_gives_two_points(eng, params):
    par = params
    queries, zs = case_points("sets_of_1_2_3", par.k, 0)
    op = S.Opening(par.polys, zs, queries, par.y, par.v)
    us = [par.u, par.u + 1, par.u]
    h1, h2s = prove(eng, par, queries, zs, par.y, par.v, us)
    assert h2s == [point(in_the_exponent(op, par.at_tau, par.tau, u)[1]) for u in us] and h2s[0] != h2s[1]
    assert h1 == point(in_the_exponent(op, par.at_tau, par.tau, None)[0])


def test_phases(eng, params):
    """debug key phases: the split of begin and of finish by events, the names of the header, non-negative times, and the
    results unchanged"""
    par = params
    queries, zs = case_points("sets_of_1_2_3", par.k, 0)
    want = prove(eng, par, queries, zs, par.y, par.v, [par.u])
    ev = eng.fr_poly_eval(par.slab, par.k, queries, enc(zs))
    lines = []
    try:
        eng.debug_configure("phases", 1)
        h1, obj = eng.kzg_shplonk_begin(par.g, par.slab, par.k, queries, enc(zs), ev, fe(par.y), fe(par.v))
        try:
            lines.append(eng.last_phases())
            h2 = eng.kzg_shplonk_finish(obj, fe(par.u))
            lines.append(eng.last_phases())
        finally:
            eng.kzg_shplonk_destroy(obj)
    finally:
        eng.debug_configure("phases", 0)
    assert (h1, [h2]) == want
    for line, names in zip(lines, (["stage", "numerators", "divide", "commit"], ["combine", "divide", "commit"])):
        fields = [f.split("=") for f in line.split()]
        assert [name for name, _ms in fields] == names, line
        assert all(float(ms) >= 0 for _name, ms in fields), line


def test_the_loop_through_the_pairing(eng, pkg, poly, params):
    """device commit -> poly.shplonk_prove -> poly.shplonk_final_pair -> the pairing"""
    par = params
    queries, zs = case_points("sets_of_1_2_3", par.k, 0)
    g2 = b"".join(O.fe_to_bytes(c) for c in (E.G2[0][0], E.G2[0][1], E.G2[1][0], E.G2[1][1]))
    s_g2 = pkg.g2_scalar_mul(g2, fe(par.tau))
    commits = [eng.g1_batch_to_affine(poly.commit_coeff(eng, par.g, enc(p))) for p in par.polys]
    assert commits == [point(x) for x in par.at_tau]
    y, v, u = fe(par.y), fe(par.v), fe(par.u)
    seen = []

    def squeeze_u(h1):
        seen.append(h1)
        return u

    evals, h1, h2 = poly.shplonk_prove(eng, par.g, par.slab, par.k, queries, enc(zs), y, v, squeeze_u)
    assert seen == [h1]
    assert evals == [fe(horner(par.polys[m], zs[p])) for m, p in queries]
    op = S.Opening(par.polys, zs, queries, par.y, par.v)
    assert (h1, h2) == tuple(point(x) for x in in_the_exponent(op, par.at_tau, par.tau, par.u))

    def verify(evals=evals, v=v, u=u, h1=h1, h2=h2):
        left, right = poly.shplonk_final_pair(eng, commits, queries, enc(zs), evals, y, v, u, h1, h2)
        return eng.final_pair_check(left, right, s_g2, g2)

    assert verify()
    bad = list(evals)
    bad[3] = fe(int.from_bytes(bad[3], "little") + 1)
    assert not verify(evals=bad)                                   # one eval changed by 1, after proving
    assert not verify(h1=h2, h2=h1)                                # H1 and H2 swapped
    assert not verify(v=fe(par.v + 1))                             # a different v on the verifier's side
    assert not verify(u=fe(par.u + 1))                             # a different u


def test_refusals_leave_the_context_usable(eng, pkg, params):
    par = params
    lib, ctx = eng._lib, eng._ctx
    queries, zs = case_points("sets_of_1_2_3", par.k, 0)
    ok = prove(eng, par, queries, zs, par.y, par.v, [par.u])
    big = R.to_bytes(32, "little")

    def begin_raw(**kw):
        """-> (status, message, object): straight through the C ABI, the object preset to a non-null value"""
        q = kw.get("q", queries)
        pts = kw.get("zs", enc(zs))
        slab, k = kw.get("slab", par.slab), kw.get("k", par.k)
        ev = kw["ev"] if "ev" in kw else eng.fr_poly_eval(par.slab, par.k, q, pts)
        flat = (C.c_uint32 * (2 * len(q)))(*[x for pair in q for x in pair])
        h1, obj = C.create_string_buffer(64), C.c_void_p(1)
        rc = lib.h2agg_kzg_shplonk_begin(ctx, kw.get("g", par.g), eng._hostptr(slab), len(slab) // (32 << k), k, flat, len(q), pts,
                                         len(pts) // 32, ev, kw.get("y", fe(par.y)), kw.get("v", fe(par.v)), h1, C.byref(obj))
        return rc, (lib.h2agg_last_error(ctx) or b"").decode(), obj

    def refused(code, needle="", **kw):
        rc, msg, obj = begin_raw(**kw)
        assert rc == code, (rc, msg)
        assert needle in msg, msg
        assert not obj.value, "a refused begin left an object"
        assert prove(eng, par, queries, zs, par.y, par.v, [par.u]) == ok        # an honest call on the same context

    good = eng.fr_poly_eval(par.slab, par.k, queries, enc(zs))
    # an eval that does not match its polynomial: the message names the query
    bad = bytearray(good)
    bad[32 * 5:32 * 6] = fe(int.from_bytes(good[32 * 5:32 * 6], "little") + 1)
    refused(pkg.ERR_INVALID, "query 5 (polynomial 2, point 4)", ev=bytes(bad))
    # a repeated pair with two values: (0, 0) is queries[0] and queries[11]
    bad = bytearray(good)
    bad[32 * 11:32 * 12] = fe(int.from_bytes(good[32 * 11:32 * 12], "little") + 1)
    refused(pkg.ERR_INVALID, "query 11", ev=bytes(bad))
    # two point indices with one value
    refused(pkg.ERR_INVALID, "hold one value", zs=enc(zs[:4] + [zs[1]] + zs[5:]), ev=good)
    # a set of 33 points (32 are served)
    many = rand_points(31, 33)
    rc, msg, obj = begin_raw(q=[(0, p) for p in range(32)], zs=enc(many))
    assert rc == pkg.OK and obj.value, msg
    lib.h2agg_kzg_shplonk_destroy(obj)
    refused(pkg.ERR_INVALID, "more than 32 points", q=[(0, p) for p in range(33)], zs=enc(many))
    # a coefficient, a point, a value, y or v >= r
    bad_slab = bytearray(par.slab)
    bad_slab[32 * 3:32 * 4] = big
    refused(pkg.ERR_NONCANONICAL, slab=bytes(bad_slab), ev=good)
    refused(pkg.ERR_NONCANONICAL, zs=enc(zs[:2]) + big + enc(zs[3:]), ev=good)
    refused(pkg.ERR_NONCANONICAL, ev=good[:64] + big + good[96:])
    refused(pkg.ERR_NONCANONICAL, y=big)
    refused(pkg.ERR_NONCANONICAL, v=big)
    # an index out of range, no queries
    refused(pkg.ERR_INVALID, q=queries + [(NPOLY, 0)], ev=good + bytes(32))
    refused(pkg.ERR_INVALID, q=queries + [(0, 6)], ev=good + bytes(32))
    refused(pkg.ERR_INVALID, q=[], ev=bytes(32))
    # a table shorter than 2^k, an unknown table, k > 24
    refused(pkg.ERR_INVALID, k=par.k + 1, slab=bytes(NPOLY * (32 << (par.k + 1))), ev=good)
    refused(pkg.ERR_INVALID, g=0xDEAD, ev=good)
    refused(pkg.ERR_INVALID, k=25, ev=good)
    # finish: u in T \ S_0 and u >= r are refused, and the object goes on to serve a legal u
    h1, obj = eng.kzg_shplonk_begin(par.g, par.slab, par.k, queries, enc(zs), good, fe(par.y), fe(par.v))
    try:
        for code, u in ((pkg.ERR_INVALID, fe(zs[3])), (pkg.ERR_INVALID, fe(zs[1])), (pkg.ERR_NONCANONICAL, big)):
            with pytest.raises(pkg.H2AggError) as ei:
                eng.kzg_shplonk_finish(obj, u)
            assert ei.value.code == code, ei.value
        assert (h1, [eng.kzg_shplonk_finish(obj, fe(par.u))]) == ok
    finally:
        eng.kzg_shplonk_destroy(obj)
    assert prove(eng, par, queries, zs, par.y, par.v, [par.u]) == ok
