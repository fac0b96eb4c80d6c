"""CPU: the witness check's definition (include/h2agg.h) restated in tests/witness_check_ref.py, on the circuit of
tests/quotient_ref.py::circuit_witness — two gates (multiplication; addition with rotation +1), one two-column lookup, a
permutation over seven columns — honest and with each of the broken witnesses tests/honest_prover.py proves.  The expected
(kind, index, row) lists are worked out here from the circuit's shape, not from the restatement.  And the binding declares the
two entry points."""
import random

import pytest

from tests import honest_prover as HP
from tests import keygen_ref as K
from tests import witness_check_ref as W

SHAPES = [(5, 4), (6, 6)]
A, B, C_COL = 0, 1, 2      # the permutation's columns 0 .. 2 are the advice columns a, b, c
MUL, ADD = 0, 1            # gate polynomials: q_m (a b - c), q_a (a + b(wX) - c)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "k%d-d%d" % s)
def case(request):
    k, degree = request.param
    rng = random.Random(0xD00 + 16 * k + degree)
    circuit = HP.make_circuit(rng, k, degree)
    mapping = K.assembly_py(len(circuit.cs.permutation_columns), k, circuit.usable, circuit.copies)
    return circuit, mapping, rng.randrange(W.R)


def report(circuit, mapping, theta, **kw):
    counts, first_rows, rows, total = W.check_circuit(circuit, mapping, theta, **kw)
    assert total == sum(counts)
    return W.failures(circuit.cs, counts, first_rows, rows), total


def test_the_honest_witness_is_clean(case):
    circuit, mapping, theta = case
    counts, first_rows, rows, total = W.check_circuit(circuit, mapping, theta)
    G, P, L = W.layout(circuit.cs)
    assert (G, P, L) == (2, 7, 1)
    assert total == 0 and counts == [0] * 10 and first_rows == [W.NONE] * 10 and rows == [[W.NONE] * 16] * 10


def test_a_broken_gate_cell(case):
    """c[3] + 1: row 3 is a multiplication row, and nothing else reads c at row 3 (the addition gate is off there); the cell may
    be copied into a later row of a"""
    circuit, mapping, theta = case
    got, total = report(HP.broken_gate_cell(circuit), mapping, theta)
    want = [("gate", MUL, 3)] + W.copy_failures(circuit, mapping, (C_COL, 3))
    assert got == want and total == len(want)


def test_a_broken_copied_cell_on_a_selectorless_row(case):
    """no gate reads it, the lookup reads b only: exactly the cell and the cell that maps to it"""
    circuit, mapping, theta = case
    cell = HP.copied_cell_off_the_gates(circuit)
    got, total = report(HP.broken_copied_cell(circuit), mapping, theta)
    want = W.copy_failures(circuit, mapping, cell)
    assert len(want) == 2 and cell[0] == A
    assert got == want and total == 2


def test_a_b_cell_outside_the_table(case):
    """b[2] leaves the table: the lookup fails on row 2; row 1 is an addition row and reads b at rotation +1, so the addition
    gate fails there; row 2 carries no selector; b[2] equals a table cell, so it is copy-constrained"""
    circuit, mapping, theta = case
    assert circuit.lag["fixed"][1][1] == 1 and not circuit.lag["fixed"][0][2] and not circuit.lag["fixed"][1][2]
    got, total = report(HP.outside_the_table(circuit), mapping, theta)
    copies = W.copy_failures(circuit, mapping, (B, 2))
    assert len(copies) == 2
    assert got == [("gate", ADD, 1)] + copies + [("lookup", 0, 2)] and total == 4


def test_masks_caps_and_no_rows(case):
    circuit, mapping, theta = case
    bad = HP.outside_the_table(circuit)
    full = W.check_circuit(bad, mapping, theta)
    for what, span in ((W.WC_GATES, range(0, 2)), (W.WC_PERMUTATION, range(2, 9)), (W.WC_LOOKUPS, range(9, 10))):
        counts, first_rows, rows, total = W.check_circuit(bad, mapping if what == W.WC_PERMUTATION else None,
                                                          theta if what == W.WC_LOOKUPS else None, what=what)
        for c in range(10):
            want = (full[0][c], full[1][c], full[2][c]) if c in span else (0, W.NONE, [W.NONE] * 16)
            assert (counts[c], first_rows[c], rows[c]) == want
        assert total == sum(full[0][c] for c in span)
    counts, first_rows, rows, total = W.check_circuit(bad, mapping, theta, max_rows=0)
    assert rows == [[]] * 10 and (counts, first_rows, total) == (full[0], full[1], full[3])
    assert W.check_circuit(bad, mapping, theta, want_rows=False)[2] is None
    assert W.failures(bad.cs, full[0], full[1], None) == W.failures(bad.cs, *full[:3])   # one failing row per constraint here


def test_the_binding_declares_both_symbols(pkg):
    names = pkg.exported_symbols()
    assert "h2agg_witness_check" in names and "h2agg_witness_check_layout" in names
    assert (pkg.WC_GATES, pkg.WC_PERMUTATION, pkg.WC_LOOKUPS, pkg.WC_NONE) == (W.WC_GATES, W.WC_PERMUTATION, W.WC_LOOKUPS, W.NONE)
