"""GPU: the witness check — h2agg_witness_check / h2agg_witness_check_layout and poly.witness_check over them.

halo2_proofs is not vendored in the reference, so the yardstick is the definition in include/h2agg.h, restated with Python
integers in tests/witness_check_ref.py (tests/test_witness_check_host.py works its answers out by hand on the honest
prover's circuit).  Everything is exact: counts, first rows, rows and total are compared word for word."""
import ctypes
import importlib
import random

import pytest

import __graft_entry__ as entry
from oracle import bn254 as O
from tests import honest_prover as HP
from tests import keygen_ref as K
from tests import quotient_ref as Q
from tests import witness_check_ref as W
from tests.fr_bytes import enc, fe

pytestmark = pytest.mark.gpu

R = Q.R
BF = 5
NONE = W.NONE
# k = 7: two workgroups of the interpreter (64 rows each).  k = 12: 4096 rows are two tiles of the report (2048 rows each: the
# second level of its scan), sixteen workgroups of the permutation and search kernels, and u = 4090 keys are two tiles of the
# sort (2^11 keys each) — the sizes tests/test_gpu_honest_proofs.py argues for its own k = 12.
SHAPES = [(5, 4), (7, 4), (12, 4)]


@pytest.fixture(scope="module")
def poly(pkg):
    return importlib.import_module(entry.PKG_NAME + ".poly")


@pytest.fixture(scope="module")
def verifier(pkg):
    return importlib.import_module(entry.PKG_NAME + ".verifier")


class Case:
    """a circuit with its mapping, a theta and the key on the device"""

    def __init__(self, eng, verifier, circuit, mapping, theta):
        self.circuit, self.mapping, self.theta = circuit, mapping, theta
        self.words = K.mapping_words(mapping) if mapping is not None else None
        self.vk = verifier.VerifyingKey(eng, verifier.encode_vk(circuit.cs, O.aff_to_bytes))

    def close(self):
        self.vk.close()


@pytest.fixture(scope="module")
def world(eng, verifier):
    """the honest prover's circuit at the three sizes: built once, shared, left unchanged"""
    cases = {}
    for k, degree in SHAPES:
        rng = random.Random(0xD00 + 16 * k + degree)
        circuit = HP.make_circuit(rng, k, degree)
        mapping = K.assembly_py(len(circuit.cs.permutation_columns), k, circuit.usable, circuit.copies)
        cases[k] = Case(eng, verifier, circuit, mapping, rng.randrange(R))
    yield cases
    for c in cases.values():
        c.close()


def slabs(circuit):
    lag = circuit.lag
    return [enc(c) for c in lag["advice"]], [enc(c) for c in lag["fixed"]], [enc(c) for c in lag["instance"]]


def raw(eng, case, circuit, what=W.WC_ALL, max_rows=16, want_rows=True, theta=True, mapping=True, challenges=None):
    """eng.witness_check on a circuit of the case's shape -> (counts, first_rows, rows, total)"""
    a, f, i = (b"".join(cols) if cols else None for cols in slabs(circuit))
    return eng.witness_check(case.vk, what, a, f, i, challenges, fe(case.theta) if theta is True else theta,
                             case.words if mapping is True else mapping, max_rows, want_rows)


def agree(eng, case, circuit, **kw):
    """the device's report == the restatement's, word for word -> the report"""
    ref_kw = {k: v for k, v in kw.items() if k in ("what", "max_rows", "want_rows")}
    want = W.check_circuit(circuit, case.mapping, case.theta, **ref_kw)
    got = raw(eng, case, circuit, **kw)
    assert got == want
    return got


def clean(eng, case):
    counts, first_rows, rows, total = raw(eng, case, case.circuit)
    C = len(counts)
    assert total == 0 and counts == [0] * C and first_rows == [NONE] * C and rows == [[NONE] * 16] * C


def rows_of(report, c):
    """the failing rows constraint c lists"""
    return [r for r in report[2][c] if r != NONE]


MUL, ADD, PERM0, LOOKUP = 0, 1, 2, 9      # constraints of the circuit: 2 gate polynomials, 7 permutation columns, 1 lookup


# ---------------------------------------------------------------------------------------------- the honest prover's circuit
@pytest.mark.parametrize("k", [5, 7, 12])
def test_the_honest_witness_is_clean(eng, poly, world, k):
    case = world[k]
    assert eng.witness_check_layout(case.vk) == W.layout(case.circuit.cs) == (2, 7, 1)
    agree(eng, case, case.circuit)
    clean(eng, case)
    rep = poly.witness_check(eng, case.vk, *slabs(case.circuit), [], theta=fe(case.theta), mapping=case.words)
    assert rep.ok and rep.total == 0 and rep.failures == [] and rep.layout == (2, 7, 1)


@pytest.mark.parametrize("k", [5, 7])
def test_single_failures_at_row_0_and_at_the_last_usable_row(eng, poly, world, k):
    case = world[k]
    c, u = case.circuit, case.circuit.usable
    assert (u - 1) % 3 == 1, "the last usable row is an addition row"
    for row, gate in ((0, MUL), (u - 1, ADD)):
        bad = c.with_cell("advice", 2, row, c.lag["advice"][2][row] + 1)
        got = agree(eng, case, bad)
        assert got[0][:2] == [int(gate == MUL), int(gate == ADD)] and got[1][gate] == row and rows_of(got, gate) == [row]
        rep = poly.witness_check(eng, case.vk, *slabs(bad), [], theta=fe(case.theta), mapping=case.words)
        assert not rep.ok and rep.failures == W.failures(c.cs, *got[:3]) and rep.failures[0] == ("gate", gate, row)
        assert (rep.counts, rep.first_rows, rep.rows, rep.total) == got


@pytest.mark.parametrize("k", [5, 7])
def test_cells_on_the_blinding_rows(eng, world, k):
    """rows from u up are never reported by their own gate row, but row u - 1 of the rotation +1 gate reads row u"""
    case = world[k]
    c, u, n = case.circuit, case.circuit.usable, case.circuit.cs.n
    on = c.with_cell("fixed", 0, u, 1).with_cell("fixed", 0, n - 1, 1).with_cell("fixed", 1, u, 1)
    lag = on.lag
    assert (lag["advice"][0][u] * lag["advice"][1][u] - lag["advice"][2][u]) % R, "the multiplication gate does not hold on row u"
    assert agree(eng, case, on)[3] == 0, "selectors switched on above the usable rows: nothing to report"
    got = agree(eng, case, on.with_cell("advice", 1, n - 1, 7))
    assert got[3] == 0, "b[n - 1] is read by rows n - 2 and n - 1 only"
    got = agree(eng, case, on.with_cell("advice", 1, u, 7))
    assert got[0] == [0, 1] + [0] * 8 and rows_of(got, ADD) == [u - 1] and got[3] == 1, "row u - 1 reads b[u]"


def test_failures_on_both_sides_of_every_boundary(eng, world):
    """k = 12.  b leaves the table on the rows around the interpreter's wave (63 | 64), the flag words (31 | 32), the
    workgroups of the permutation and search kernels (255 | 256), the report's tile = the second level of its scan
    (2047 | 2048), and on the first and last usable rows: the lookup fails on exactly those rows, the multiplication gate on
    those that are multiplication rows, the addition gate one row above those behind an addition row, and b's copies break"""
    case = world[12]
    c, u = case.circuit, case.circuit.usable
    marks = [0, 31, 32, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, u - 1]
    table = set(c.lag["fixed"][2][:u])
    bad, v = c, 1 << 200
    for row in marks:
        while v in table:
            v += 1
        bad = bad.with_cell("advice", 1, row, v)
        v += 1
    got = agree(eng, case, bad, max_rows=32)
    assert rows_of(got, LOOKUP) == marks and got[0][LOOKUP] == len(marks) and got[1][LOOKUP] == 0
    assert rows_of(got, MUL) == [r for r in marks if r % 3 == 0]
    assert rows_of(got, ADD) == [r - 1 for r in marks if r % 3 == 2]
    # every b cell is a copy of a table cell: it fails, and so does the cell that maps to it (a table cell or another b cell)
    assert set(marks) <= set(rows_of(got, PERM0 + 1)) and len(marks) < sum(got[0][PERM0:LOOKUP]) <= 2 * len(marks)
    assert got[3] == sum(got[0])
    for cap in (10, 11):                                  # the cap falls on the tile boundary, and one row behind it
        capped = agree(eng, case, bad, max_rows=cap)
        assert capped[2][LOOKUP] == marks[:cap] and capped[0] == got[0] and capped[1] == got[1]


@pytest.mark.parametrize("kind", ["gate cell", "copied cell", "outside the table"])
def test_the_broken_witnesses_of_the_honest_prover(eng, world, kind):
    case = world[5]
    c = case.circuit
    bad = {"gate cell": HP.broken_gate_cell, "copied cell": HP.broken_copied_cell, "outside the table": HP.outside_the_table}[kind](c)
    got = agree(eng, case, bad)
    cell = {"gate cell": (2, 3), "copied cell": HP.copied_cell_off_the_gates(c), "outside the table": (1, 2)}[kind]
    want = W.copy_failures(c, case.mapping, cell)
    if kind == "gate cell":
        want = [("gate", MUL, 3)] + want
    if kind == "outside the table":
        want = [("gate", ADD, 1)] + want + [("lookup", 0, 2)]
    assert W.failures(c.cs, *got[:3]) == want


def test_masks(eng, world):
    """each kind alone: the full call's lines for that kind, 0 / no row elsewhere; the other kinds' arguments may be absent"""
    case = world[5]
    bad = HP.outside_the_table(case.circuit)
    full = agree(eng, case, bad)
    for what, span in ((W.WC_GATES, range(0, 2)), (W.WC_PERMUTATION, range(2, 9)), (W.WC_LOOKUPS, range(9, 10))):
        got = agree(eng, case, bad, what=what, theta=True if what == W.WC_LOOKUPS else None,
                    mapping=True if what == W.WC_PERMUTATION else None)
        for con in range(10):
            want = (full[0][con], full[1][con], full[2][con]) if con in span else (0, NONE, [NONE] * 16)
            assert (got[0][con], got[1][con], got[2][con]) == want
        assert got[3] == sum(full[0][con] for con in span) and got[3] > 0
    assert agree(eng, case, bad, what=W.WC_GATES | W.WC_LOOKUPS)[3] == 2


# ---------------------------------------------------------------------------------------------- small keys
def small_cs(k, gates=(), lookups=(), perm=(), num_challenges=0):
    """3 advice, 2 fixed, 1 instance column; a(0) a(1) a(2) at the current row and a(0) at the next"""
    return Q.make_cs(k, 4, 3, 2, 1, [(0, 0), (1, 0), (2, 0), (0, 1)], [(0, 0), (1, 0)], [(0, 0)], [list(g) for g in gates],
                     list(lookups), list(perm), BF, num_challenges)


A0, A1, A2, A0_NEXT = (("advice", q) for q in range(4))
F0, F1, I0 = ("fixed", 0), ("fixed", 1), ("instance", 0)


class Small:
    def __init__(self, eng, verifier, cs):
        self.cs, self.n, self.u = cs, cs.n, cs.n - BF - 1
        self.vk = verifier.VerifyingKey(eng, verifier.encode_vk(cs, O.aff_to_bytes))

    def check(self, eng, advice, fixed, instance, what=W.WC_ALL, theta=None, mapping=None, max_rows=16, want_rows=True, challenges=()):
        want = W.witness_check_py(self.cs, what, advice, fixed, instance, list(challenges), theta, mapping, max_rows, want_rows)
        got = eng.witness_check(self.vk, what, b"".join(enc(c) for c in advice), b"".join(enc(c) for c in fixed),
                                b"".join(enc(c) for c in instance), b"".join(fe(x) for x in challenges) or None,
                                None if theta is None else fe(theta), None if mapping is None else K.mapping_words(mapping),
                                max_rows, want_rows)
        assert got == want
        return got

    def close(self):
        self.vk.close()


def columns(rng, n, count):
    return [[rng.randrange(R) for _ in range(n)] for _ in range(count)]


@pytest.mark.parametrize("k", [5, 12])
def test_every_usable_row_failing_one_gate(eng, verifier, k):
    """the gate a(0) on a column of ones, and the gate a(1) on a column of zeros beside it"""
    s = Small(eng, verifier, small_cs(k, gates=[[A0], [A1]]))
    n, u = s.n, s.u
    advice, fixed, instance = [[1] * n, [0] * n, [3] * n], [[0] * n] * 2, [[0] * n]
    for max_rows in (0, 1, 16):
        counts, first_rows, rows, total = s.check(eng, advice, fixed, instance, what=W.WC_GATES, max_rows=max_rows)
        assert counts == [u, 0] and first_rows == [0, NONE] and total == u
        assert rows == [list(range(max_rows)), [NONE] * max_rows]
    assert s.check(eng, advice, fixed, instance, what=W.WC_GATES, want_rows=False)[2] is None
    wide = s.check(eng, advice, fixed, instance, what=W.WC_GATES, max_rows=n + 8)      # more rows than a line can hold
    assert wide[2] == [list(range(u)) + [NONE] * (n + 8 - u), [NONE] * (n + 8)]
    s.close()


def test_redundant_zeros_are_zero_and_r_minus_1_is_not(eng, verifier):
    """the interpreter's stack values are any representative below 2r: 1 + (r - 1) is r, the negation of 0 is 2r - 0, a product
    with a factor 0 is 0 — all satisfied; r - 1, as a sum and as the negation of 1, fails on every usable row"""
    gates = [[("sum", A0, A1)], [("neg", A2)], [("product", A2, A1), ("sum", ("neg", A2), ("sum", A0, A1))],
             [("sum", A2, A1)], [("neg", A0)], [("sum", ("const", R - 1), A2)]]
    s = Small(eng, verifier, small_cs(5, gates=gates))
    n, u = s.n, s.u
    counts, first_rows, rows, total = s.check(eng, [[1] * n, [R - 1] * n, [0] * n], [[0] * n] * 2, [[0] * n], what=W.WC_GATES)
    assert counts == [0, 0, 0, 0, u, u, u] and total == 3 * u and first_rows[4:] == [0, 0, 0]
    s.close()


def test_permutation_cycles(eng, verifier):
    """columns: a(0), a(1), the instance column, fixed 0"""
    k = 5
    perm = [("advice", 0), ("advice", 1), ("instance", 0), ("fixed", 0)]
    s = Small(eng, verifier, small_cs(k, perm=perm))
    n, u = s.n, s.u
    rng = random.Random(0x5C1)
    advice, fixed, instance = columns(rng, n, 3), columns(rng, n, 2), columns(rng, n, 1)
    ident = K.identity_mapping(4, k)
    got = s.check(eng, advice, fixed, instance, what=W.WC_PERMUTATION, mapping=ident)
    assert got[3] == 0, "the identity never fails"
    copies = [(0, 1, 1, 2), (1, 2, 0, 5),        # a 3-cycle over two advice columns
              (0, 3, 2, 0),                      # an advice cell and an instance cell
              (3, 4, 1, 7)]                      # a fixed cell and an advice cell
    mapping = K.assembly_py(4, k, u, copies)
    value = {(0, 1): 11, (1, 2): 11, (0, 5): 11, (0, 3): 12, (2, 0): 12, (3, 4): 13, (1, 7): 13}
    cols = [advice[0], advice[1], instance[0], fixed[0]]
    for (c, r), v in value.items():
        cols[c][r] = v
    assert s.check(eng, advice, fixed, instance, what=W.WC_PERMUTATION, mapping=mapping)[3] == 0
    # the 3-cycle with one cell changed: the cell and the cell that maps to it fail, the third does not
    cycle = [(0, 1), (1, 2), (0, 5)]
    for mid in cycle:
        before = [x for x in cycle if mapping[x[0] * n + x[1]] == mid][0]
        cols[mid[0]][mid[1]] = 99
        got = s.check(eng, advice, fixed, instance, what=W.WC_PERMUTATION, mapping=mapping)
        assert W.failures(s.cs, *got[:3]) == [("permutation", c, r) for c, r in sorted([mid, before])] and got[3] == 2
        cols[mid[0]][mid[1]] = 11
    for cell, other in (((2, 0), (0, 3)), ((3, 4), (1, 7))):
        cols[cell[0]][cell[1]] += 1
        got = s.check(eng, advice, fixed, instance, what=W.WC_PERMUTATION, mapping=mapping)
        assert W.failures(s.cs, *got[:3]) == [("permutation", c, r) for c, r in sorted([cell, other])]
        cols[cell[0]][cell[1]] -= 1
    s.close()


def test_lookups(eng, verifier):
    """lookup 0: a(0) in fixed 0; lookup 1: (a(1), a(2)) in (fixed 0, fixed 1)"""
    k = 5
    s = Small(eng, verifier, small_cs(k, lookups=[([A0], [F0]), ([A1, A2], [F0, F1])]))
    n, u = s.n, s.u
    theta = random.Random(0x5C2).randrange(R)
    t0 = [100 + (i % 5) for i in range(n)]                     # repeated table values: 100 .. 104
    t1 = [200 + (i % 7) for i in range(n)]                     # the pairs (100 + i % 5, 200 + i % 7): 26 of the 35 below u
    t0[u + 1], t1[u + 1] = 150, 250                            # a value and a pair that only a blinding row holds
    pairs = {(t0[i], t1[i]) for i in range(u)}
    free = [(x, y) for x in range(100, 105) for y in range(200, 207) if (x, y) not in pairs]
    assert free and (150, 250) not in pairs
    a0 = [t0[(3 * i) % u] for i in range(n)]
    a1 = [t0[(5 * i) % u] for i in range(n)]
    a2 = [t1[(5 * i) % u] for i in range(n)]
    fixed, instance = [t0, t1], [[0] * n]
    check = lambda: s.check(eng, [a0, a1, a2], fixed, instance, what=W.WC_LOOKUPS, theta=theta)
    assert check()[3] == 0
    a0[4], a0[9] = 99, 150                                     # absent; present on a blinding row only
    a1[0], a2[0] = free[0]                                     # each coordinate occurs, the pair does not
    a1[u - 1], a2[u - 1] = 150, 250
    a0[u], a1[u + 2] = 98, 97                                  # blinding rows of the input are not checked
    got = check()
    assert W.failures(s.cs, *got[:3]) == [("lookup", 0, 4), ("lookup", 0, 9), ("lookup", 1, 0), ("lookup", 1, u - 1)]
    a0[:] = [7] * n                                            # all inputs equal: absent, then present
    assert check()[0][0] == u
    a0[:] = [103] * n
    assert check()[0][0] == 0
    s.close()


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_context_usable(pkg, eng, verifier, world):
    case = world[5]
    c = case.circuit
    a, f, i = (b"".join(cols) for cols in slabs(c))
    theta, words, vk = fe(case.theta), case.words, case.vk
    n = c.cs.n

    def refused(code, *args, **kw):
        with pytest.raises(pkg.H2AggError) as ei:
            eng.witness_check(*args, **kw)
        assert ei.value.code == code, ei.value
        clean(eng, case)

    refused(pkg.ERR_INVALID, vk, 0, a, f, i, None, theta, words)
    refused(pkg.ERR_INVALID, vk, 8, a, f, i, None, theta, words)
    refused(pkg.ERR_INVALID, vk, W.WC_ALL | 16, a, f, i, None, theta, words)
    refused(pkg.ERR_INVALID, vk, W.WC_ALL, None, f, i, None, theta, words)
    refused(pkg.ERR_INVALID, vk, W.WC_GATES, a, None, i, None, None, None)
    refused(pkg.ERR_INVALID, vk, W.WC_GATES, a, f, None, None, None, None)
    refused(pkg.ERR_INVALID, vk, W.WC_ALL, a, f, i, None, None, words)
    refused(pkg.ERR_INVALID, vk, W.WC_ALL, a, f, i, None, theta, None)
    for cell, entry_ in ((3, (7, 0)), (5 * n + 9, (0, n))):          # a column == P, a row == n
        bad = list(case.mapping)
        bad[cell] = entry_
        refused(pkg.ERR_INVALID, vk, W.WC_PERMUTATION, a, f, i, None, None, K.mapping_words(bad))
    refused(pkg.ERR_NONCANONICAL, vk, W.WC_LOOKUPS, a, f, i, None, enc([R]), None)
    # a column element >= r: through the device status
    for slab_at, what in ((0, W.WC_GATES), (1, W.WC_LOOKUPS), (2, W.WC_PERMUTATION)):
        cols = [bytearray(a), bytearray(f), bytearray(i)]
        at = {0: 32 * 3, 1: 32 * (2 * n + 2), 2: 32 * 1}[slab_at]  # a[3] (a multiplication row), the table's row 2, the instance's row 1
        cols[slab_at][at:at + 32] = enc([R + 1])
        refused(pkg.ERR_NONCANONICAL, vk, what, bytes(cols[0]), bytes(cols[1]), bytes(cols[2]), None, theta, words)
    # null context, key, outputs: the C call itself
    lib = pkg.load_library()
    cnt, first, total = (ctypes.c_uint32 * 10)(), (ctypes.c_uint32 * 10)(), ctypes.c_uint64()
    call = lambda ctx, key, counts, firsts, tot: lib.h2agg_witness_check(ctx, key, W.WC_ALL, a, f, i, None, theta, words, 0, counts, firsts,
                                                                       None, tot)
    assert call(None, vk._vk, cnt, first, ctypes.byref(total)) == pkg.ERR_INVALID
    assert call(eng._ctx, None, cnt, first, ctypes.byref(total)) == pkg.ERR_INVALID
    assert call(eng._ctx, vk._vk, None, first, ctypes.byref(total)) == pkg.ERR_INVALID
    assert call(eng._ctx, vk._vk, cnt, None, ctypes.byref(total)) == pkg.ERR_INVALID
    assert call(eng._ctx, vk._vk, cnt, first, None) == pkg.ERR_INVALID
    assert lib.h2agg_witness_check_layout(None, None, None, None) == pkg.ERR_INVALID
    assert call(eng._ctx, vk._vk, cnt, first, ctypes.byref(total)) == pkg.OK and total.value == 0
    clean(eng, case)


def test_refusals_of_keys_with_challenges_and_deep_expressions(pkg, eng, verifier):
    from tests.test_gpu_quotient import nested_sum
    k = 5
    n = 1 << k
    rng = random.Random(0x5C3)
    advice, fixed, instance = columns(rng, n, 3), columns(rng, n, 2), columns(rng, n, 1)
    s = Small(eng, verifier, small_cs(k, gates=[[("sum", ("product", ("challenge", 0), A0), ("neg", A1))]], num_challenges=1))
    ch = 5
    advice[1] = [ch * x % R for x in advice[0]]
    args = [b"".join(enc(c) for c in cols) for cols in (advice, fixed, instance)]
    assert s.check(eng, advice, fixed, instance, what=W.WC_GATES, challenges=[ch])[3] == 0
    assert s.check(eng, advice, fixed, instance, what=W.WC_GATES, challenges=[ch + 1])[0] == [s.u]
    for challenges, code in ((None, pkg.ERR_INVALID), (enc([R]), pkg.ERR_NONCANONICAL)):
        with pytest.raises(pkg.H2AggError) as ei:
            if challenges is None:                          # (the binding sizes the buffer: the C call sees the null pointer)
                eng._check(eng._lib.h2agg_witness_check(eng._ctx, s.vk._vk, W.WC_GATES, *args, None, None, None, 0,
                                                        (ctypes.c_uint32 * 1)(), (ctypes.c_uint32 * 1)(), None,
                                                        ctypes.byref(ctypes.c_uint64())))
            else:
                eng.witness_check(s.vk, W.WC_GATES, *args, challenges, None, None)
        assert ei.value.code == code
        assert s.check(eng, advice, fixed, instance, what=W.WC_GATES, challenges=[ch])[3] == 0
    s.close()
    # the operand stack: 16 values pass, 17 are refused — and a lookup's only when the lookups are asked for
    ok16 = Small(eng, verifier, Q.make_cs(k, 4, 3, 2, 1, [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1)], [(0, 0), (1, 0)], [(0, 0)],
                                         [[nested_sum(pkg.EXPR_MAX_DEPTH)]], [([nested_sum(pkg.EXPR_MAX_DEPTH + 1)], [F0])], [], BF))
    ok16.check(eng, advice, fixed, instance, what=W.WC_GATES)
    with pytest.raises(pkg.H2AggError) as ei:
        eng.witness_check(ok16.vk, W.WC_LOOKUPS, *args, None, fe(3), None)
    assert ei.value.code == pkg.ERR_INVALID and "H2AGG_EXPR_MAX_DEPTH" in str(ei.value)
    ok16.check(eng, advice, fixed, instance, what=W.WC_GATES)
    ok16.close()


# ---------------------------------------------------------------------------------------------- the rest of the library
def test_agreement_with_the_prover_stages_and_the_verifier(pkg, eng, poly, verifier, world):
    """a witness the check calls clean proves through the device stages and is accepted; the witness with b[2] outside the table
    fails its lookup on exactly the row whose removal lets permute_expression_pair answer"""
    from tests.test_gpu_honest_proofs import TAU, device_prove, verdicts
    case = world[5]
    c = case.circuit
    clean(eng, case)
    setup = HP.Setup(5, TAU, HP.INSTANCE_ROWS)
    proof = device_prove(pkg, eng, poly, verifier, setup, c)
    each, agg = verdicts(eng, verifier, {5: setup}, [[proof]])
    assert [(s, ok) for _pair, s, ok in each] == [(0, True)] and agg is True
    bad = HP.outside_the_table(c)
    rep = poly.witness_check(eng, case.vk, *slabs(bad), [], theta=fe(case.theta), what=pkg.WC_LOOKUPS)
    assert rep.failures == [("lookup", 0, 2)] and rep.total == 1
    fold = lambda circuit, which: poly.expressions_eval(eng, case.vk, which, 0, *slabs(circuit), [], fold=fe(case.theta))
    with pytest.raises(pkg.H2AggError) as ei:
        poly.permute_expression_pair(eng, fold(bad, 1), fold(bad, 2), 5, c.usable)
    assert ei.value.code == pkg.ERR_NOT_IN_TABLE
    a_in = bytearray(fold(bad, 1))
    a_in[32 * 2:32 * 3] = fold(c, 1)[32 * 2:32 * 3]          # row 2 put back: every other row was in the table
    poly.permute_expression_pair(eng, bytes(a_in), fold(bad, 2), 5, c.usable)
    clean(eng, case)
