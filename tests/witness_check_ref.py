"""The definition of include/h2agg.h's witness-check block restated with Python integers: witness_check_py has the
signature and the report of h2agg_witness_check (constraints in the order gate polynomials, permutation columns, lookups;
counts, first rows, the lowest max_rows failing rows per constraint behind 0xFFFFFFFF padding, the total).  Expressions are
evaluated by tests/quotient_ref.py::expressions_rows_py (oracle/verifier.py::evaluate_expression row by row), the mapping is
tests/keygen_ref.py's list of (column, row), cell (j, i) at index j * n + i."""
from tests import quotient_ref as Q

R = Q.R
WC_GATES, WC_PERMUTATION, WC_LOOKUPS = 1, 2, 4
WC_ALL = WC_GATES | WC_PERMUTATION | WC_LOOKUPS
NONE = 0xFFFFFFFF
KINDS = ("gate", "permutation", "lookup")


def layout(cs):
    """-> (gate polynomials, permutation columns, lookups)"""
    return sum(len(g) for g in cs.gates), len(cs.permutation_columns), len(cs.lookups)


def failing_rows_py(cs, what, advice, fixed, instance, challenges, theta, mapping):
    """-> one ascending list of failing rows per constraint (empty for a kind that is not in `what`)"""
    n, u = cs.n, cs.n - cs.blinding_factors - 1
    G, P, L = layout(cs)
    out = []
    if what & WC_GATES and G:
        for col in Q.expressions_rows_py(cs, 0, 0, advice, fixed, instance, challenges):
            out.append([i for i in range(u) if col[i] % R])
    else:
        out += [[] for _ in range(G)]
    if what & WC_PERMUTATION and P:
        slabs = {"advice": advice, "fixed": fixed, "instance": instance}
        value = lambda c, r: slabs[cs.permutation_columns[c][0]][cs.permutation_columns[c][1]][r] % R
        assert len(mapping) == P * n and all(c < P and r < n for c, r in mapping)
        for g in range(P):
            out.append([i for i in range(n) if value(g, i) != value(*mapping[g * n + i])])
    else:
        out += [[] for _ in range(P)]
    for j in range(L):
        if what & WC_LOOKUPS:
            a = Q.expressions_rows_py(cs, 1, j, advice, fixed, instance, challenges, theta)
            s = Q.expressions_rows_py(cs, 2, j, advice, fixed, instance, challenges, theta)
            table = set(s[:u])
            out.append([i for i in range(u) if a[i] not in table])
        else:
            out.append([])
    return out


def witness_check_py(cs, what, advice, fixed, instance, challenges, theta, mapping, max_rows, want_rows=True):
    """h2agg_witness_check -> (counts, first_rows, rows, total); rows is None for want_rows False (the C call's rows == NULL)"""
    assert what and not what & ~WC_ALL
    failing = failing_rows_py(cs, what, advice, fixed, instance, challenges, theta, mapping)
    counts = [len(f) for f in failing]
    first_rows = [f[0] if f else NONE for f in failing]
    rows = [(f[:max_rows] + [NONE] * max_rows)[:max_rows] for f in failing] if want_rows else None
    return counts, first_rows, rows, sum(counts)


def check_circuit(circuit, mapping, theta, what=WC_ALL, max_rows=16, want_rows=True):
    """witness_check_py on a tests/honest_prover.py Circuit"""
    lag = circuit.lag
    return witness_check_py(circuit.cs, what, lag["advice"], lag["fixed"], lag["instance"], [], theta, mapping, max_rows, want_rows)


def copy_failures(circuit, mapping, cell):
    """The permutation failures a change of ONE cell (permutation column, row) of a satisfied witness causes, by the cycle
    structure alone: the cell itself (its image keeps the old value) and the cell that maps to it — nothing if the cell is a
    cycle of its own.  -> [("permutation", column, row), ...] in report order"""
    n = circuit.cs.n
    if mapping[cell[0] * n + cell[1]] == cell:
        return []
    before = [(x // n, x % n) for x, image in enumerate(mapping) if image == cell]
    assert len(before) == 1
    return [("permutation", c, r) for c, r in sorted({cell, before[0]})]


def failures(cs, counts, first_rows, rows):
    """the (kind, index within the kind, row) list of the package's WitnessReport"""
    out, c = [], 0
    for kind, count in zip(KINDS, layout(cs)):
        for index in range(count):
            if rows is not None and rows[c]:
                out += [(kind, index, r) for r in rows[c] if r != NONE]
            elif counts[c]:
                out.append((kind, index, first_rows[c]))
            c += 1
    return out
