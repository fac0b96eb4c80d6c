"""CPU: the Python yardstick of the Shplonk tests (tests/shplonk_ref.py) against itself — the partial-fraction sum that the
device's set division computes equals successive synthetic division, h and h2 satisfy the identities of the definition
(include/h2agg.h) at a known tau, L(u) = 0, the verifier equation holds in the exponent and fails for every way of getting it
wrong that was tried — and poly.shplonk_sets against the reference's sets.  Polynomials of 16 coefficients."""
import importlib
import random

import pytest

import __graft_entry__ as entry
from tests import shplonk_ref as S

R = S.R
N = 16
# 7 polynomials, 6 points: sets {0}, {1, 2}, {3, 4, 5} with 2, 3 and 2 polynomials, interleaved, (0, 0) repeated
QUERIES = [(0, 0), (1, 1), (2, 3), (1, 2), (3, 0), (2, 4), (4, 2), (2, 5), (4, 1), (5, 5), (5, 3), (0, 0), (5, 4), (6, 1), (6, 2)]


@pytest.fixture(scope="module")
def poly(pkg):
    return importlib.import_module(entry.PKG_NAME + ".poly")


@pytest.fixture(scope="module")
def op():
    rng = random.Random(0x5B10)
    polys = [[rng.randrange(R) for _ in range(N)] for _ in range(7)]
    zs = [rng.randrange(R) for _ in range(6)]
    o = S.Opening(polys, zs, QUERIES, rng.randrange(R), rng.randrange(R))
    o.tau, o.u = rng.randrange(R), rng.randrange(R)
    o.commit = [S.horner(p, o.tau) for p in polys]          # discrete logarithms of the commitments
    o.h1 = S.horner(o.h(), o.tau)
    o.h2_tau = S.horner(o.h2(o.u)[0], o.tau)
    return o


def accepted(op, f, h2_tau=None, u=None):
    """e(H2, tau G2) e(F + u H2, -G2) = 1 in the exponent: tau h2 = F + u h2"""
    h2_tau = op.h2_tau if h2_tau is None else h2_tau
    u = op.u if u is None else u
    return (op.tau * h2_tau - f - u * h2_tau) % R == 0


def test_the_sets_of_the_fixture(op):
    assert op.sets == [([0], [0, 3]), ([1, 2], [1, 4, 6]), ([3, 4, 5], [2, 5])]
    assert op.T == [0, 1, 3, 2, 4, 5]


def test_interpolation_goes_through_the_values(op):
    for i, (pts, members) in enumerate(op.sets):
        for j, m in enumerate(members):
            assert len(op.r[i][j]) == len(pts)
            for p in pts:
                assert S.horner(op.r[i][j], op.zs[p]) == S.horner(op.polys[m], op.zs[p])


def test_partial_fractions_equal_successive_division(op):
    for i, (pts, _members) in enumerate(op.sets):
        num, zs = op.numerator(i), [op.zs[p] for p in pts]
        for z in zs:
            assert S.horner(num, z) == 0
        q = S.divide_by_roots(num, zs)
        assert S.partial_fraction_quotient(num, zs) == q
        assert q[N - len(zs):] == [0] * len(zs)
        back = q[:N - len(zs)]                                  # q Z_S = N, coefficient by coefficient
        for z in zs:
            back = S.poly_mul_linear(back, z)
        assert back == num
    assert op.h(S.partial_fraction_quotient) == op.h()


def test_h_identity_at_tau(op):
    """h(tau) = sum_i v^i N_i(tau) / Z_{S_i}(tau), and times Z_T: h(tau) Z_T(tau) = sum_i v^i N_i(tau) Z_{T \\ S_i}(tau)"""
    want, cleared, vi = 0, 0, 1
    for i, (pts, _m) in enumerate(op.sets):
        n_tau = S.horner(op.numerator(i), op.tau)
        want = (want + vi * n_tau * S.inv(op.z_at(pts, op.tau))) % R
        cleared = (cleared + vi * n_tau * op.z_at([p for p in op.T if p not in pts], op.tau)) % R
        vi = vi * op.v % R
    assert op.h1 == want
    assert op.h1 * op.z_at(op.T, op.tau) % R == cleared


def test_l_vanishes_at_u_and_h2_divides_it(op):
    L = op.L(op.u)
    assert S.horner(L, op.u) == 0
    q, rem = op.h2(op.u)
    assert rem == 0 and q[N - 1] == 0
    assert S.poly_mul_linear(q[:N - 1], op.u) == L
    assert op.h2_tau * (op.tau - op.u) % R == S.horner(L, op.tau)


def test_u_in_the_first_set_is_legal(op):
    u = op.zs[0]
    assert op.scalars(u) is not None and op.scalars(u)[2] == 0          # t = Z_T(u) / d_0 = 0
    assert S.horner(op.L(u), u) == 0
    assert op.scalars(op.zs[3]) is None                                  # a point of T \ S_0: d_0 = 0


def test_verifier_equation_in_the_exponent(op):
    assert accepted(op, op.verifier_f(op.u, op.commit, op.h1))
    assert (op.verifier_f(op.u, op.commit, op.h1) - S.horner(op.L(op.u), op.tau)) % R == 0


def test_verifier_equation_fails_when_it_should(op):
    d, c, t = op.scalars(op.u)
    f = lambda **kw: op.verifier_f(op.u, op.commit, op.h1, **kw)
    for q in (0, 3, len(QUERIES) - 1):                                   # one changed eval
        bad = list(op.evals)
        bad[q] = (bad[q] + 1) % R
        assert not accepted(op, f(evals=bad)), q
    assert not accepted(op, f(y=op.v, v=op.y))                           # y and v swapped
    # a v^i attached to the wrong set: sets 1 and 2 trade their powers of v
    swapped, vi = 0, [1, op.v * op.v % R, op.v]
    for i, (_pts, members) in enumerate(op.sets):
        w = vi[i] * c[i] % R
        for j, m in enumerate(members):
            swapped = (swapped + w * (op.commit[m] - S.horner(op.r[i][j], op.u))) % R
            w = w * op.y % R
    assert not accepted(op, (swapped - t * op.h1) % R)
    assert not accepted(op, f(c=d, t=op.z_at(op.T, op.u)))               # 1 / d_0 missing
    z_t = op.z_at(op.T, op.u)
    assert not accepted(op, f(c=[z_t * S.inv(d[0])] * len(d)))           # Z_T in place of Z_{T \ S_i}
    assert not accepted(op, f(), h2_tau=op.h1)                           # H1 where H2 belongs
    assert not accepted(op, op.verifier_f(op.u + 1, op.commit, op.h1), u=op.u + 1)   # another u, the old H2


SET_CASES = [
    # repeated pairs count once, whatever lies between them
    ([(0, 1), (0, 1), (1, 1), (0, 2), (1, 2), (0, 1)], [([1, 2], [0, 1])]),
    # interleaved first-seen orders: the set of polynomial 2 is complete only at the end
    ([(2, 0), (0, 1), (1, 0), (2, 1), (0, 0), (3, 1)], [([0, 1], [2, 0]), ([0], [1]), ([1], [3])]),
    # equal sets named in different orders are one set
    ([(0, 3), (0, 5), (1, 5), (1, 3)], [([3, 5], [0, 1])]),
    # one set only
    ([(4, 7), (2, 7), (9, 7)], [([7], [4, 2, 9])]),
    # every polynomial its own set
    ([(0, 0), (1, 1), (2, 0), (2, 1), (3, 2)], [([0], [0]), ([1], [1]), ([0, 1], [2]), ([2], [3])]),
    ([(7, 5)], [([5], [7])]),
    ([], []),
]


@pytest.mark.parametrize("queries,want", SET_CASES)
def test_shplonk_sets_is_the_definition(poly, queries, want):
    assert S.sets_of(queries) == want
    assert poly.shplonk_sets(queries) == want


def test_shplonk_sets_scrambled(poly):
    rng = random.Random(0x5E75)
    for _ in range(60):
        queries = [(rng.randrange(7), rng.randrange(4)) for _ in range(rng.randrange(1, 18))]
        got = poly.shplonk_sets(queries)
        assert got == S.sets_of(queries)
        assert sorted(m for _pts, members in got for m in members) == sorted({m for m, _p in queries})
        assert len({frozenset(pts) for pts, _m in got}) == len(got)


def test_the_bindings_exist(pkg, poly):
    names = set(pkg.exported_symbols())
    for fn in ("h2agg_kzg_shplonk_begin", "h2agg_kzg_shplonk_finish", "h2agg_kzg_shplonk_destroy"):
        assert fn in names, fn
    for method in ("kzg_shplonk_begin", "kzg_shplonk_finish", "kzg_shplonk_destroy"):
        assert callable(getattr(pkg.H2Agg, method)), method
    for fn in ("shplonk_sets", "shplonk_prove", "shplonk_final_pair"):
        assert callable(getattr(poly, fn)), fn
