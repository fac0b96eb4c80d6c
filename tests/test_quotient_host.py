"""CPU: tests/quotient_ref.py, the restatement the GPU tests of the quotient compare with, against its own definitions and
against the reference's verifier.  The transform is held against the DFT sum; quotient_py, on a circuit that holds, gives an H
without coefficients above the pieces, and its pieces satisfy the identity the verifier checks at a point
(oracle/verifier.py:393-398: mul_add_accumulate(expressions, y) = (x^n - 1) h(x), h = sum x^(n i) h_i — vanish.rs:18-72) with
the expressions built by the oracle's own permutation_expressions / lookup_expressions / evaluate_expression."""
import random

import pytest

from tests import quotient_ref as Q

R = Q.R


@pytest.fixture(scope="module")
def circuit():
    cs, lag, polys, sc = Q.satisfied_circuit(random.Random(0xC0), 5, 4)
    pieces, H = Q.quotient_py(cs, *Q.quotient_args(polys, sc))
    return cs, lag, polys, sc, pieces, H


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4])
def test_ntt_is_the_dft(k):
    rng = random.Random(0xC1 + k)
    n, w = 1 << k, Q.omega(k)
    vals = [rng.randrange(R) for _ in range(n)]
    for shift in (1, Q.ZETA, rng.randrange(1, R)):
        want = [sum(pow(shift, j, R) * vals[j] % R * pow(w, i * j, R) for j in range(n)) % R for i in range(n)]
        assert Q.ntt(vals, k, shift) == want
        assert Q.ntt(want, k, shift, inverse=True) == vals


def test_extended_k():
    assert [Q.extended_k(5, d) for d in (3, 4, 5, 6, 9, 10)] == [1, 2, 2, 3, 3, 4]


def test_gates_vanish_on_the_witness(circuit):
    cs, lag, _polys, sc, _pieces, _H = circuit
    cols = Q.expressions_rows_py(cs, 0, 0, lag["advice"], lag["fixed"], lag["instance"], [])
    assert len(cols) == 2 and all(v == 0 for col in cols for v in col)
    assert Q.expressions_rows_py(cs, 0, 0, lag["advice"], lag["fixed"], lag["instance"], [], sc["y"]) == [0] * cs.n


def test_quotient_of_a_satisfied_circuit_fits_its_pieces(circuit):
    cs, _lag, _polys, _sc, pieces, H = circuit
    n = cs.n
    assert len(pieces) == cs.degree - 1 and len(H) == n << Q.extended_k(cs.k, cs.degree)
    assert not any(H[(cs.degree - 1) * n:])
    assert any(pieces[-1])


def test_pieces_satisfy_the_verifiers_identity(circuit):
    cs, _lag, polys, sc, pieces, _H = circuit
    rng = random.Random(0xC2)
    for _ in range(2):
        x = rng.randrange(R)
        assert Q.verifier_numerator(cs, polys, sc, x) == Q.h_at(pieces, cs.n, x)


def test_a_broken_witness_cell_fails_the_identity(circuit):
    cs, lag, polys, sc, _pieces, _H = circuit
    broken = {kind: list(cols) for kind, cols in polys.items()}
    c = list(lag["advice"][2])
    assert lag["fixed"][0][3] == 1            # row 3 is a multiplication row: q_m (a b - c) no longer vanishes there
    c[3] = (c[3] + 1) % R
    broken["advice"] = [polys["advice"][0], polys["advice"][1], Q.ntt(c, cs.k, inverse=True)]
    pieces, H = Q.quotient_py(cs, *Q.quotient_args(broken, sc))
    assert any(H[(cs.degree - 1) * cs.n:])    # N is no multiple of X^n - 1 any more
    x = random.Random(0xC3).randrange(R)
    assert Q.verifier_numerator(cs, broken, sc, x) != Q.h_at(pieces, cs.n, x)


def test_random_inputs_have_one_answer():
    """on inputs that satisfy nothing quotient_py still interpolates N / (X^n - 1) on the coset: H(s) (s^n - 1) = N(s)"""
    rng = random.Random(0xC4)
    cs = Q.random_shape(rng, 4, 4, 3, 1, True, num_challenges=2)
    polys, sc = Q.random_inputs(rng, cs), Q.random_scalars(rng, 2)
    _pieces, H = Q.quotient_py(cs, *Q.quotient_args(polys, sc))
    s = Q.ZETA * pow(Q.omega(cs.k + 2), 5, R) % R
    assert Q.horner(H, s) * (pow(s, cs.n, R) - 1) % R == Q.verifier_numerator(cs, polys, sc, s)
