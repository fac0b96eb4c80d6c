"""CPU: h2agg_permutation_assembly — halo2's permutation::keygen::Assembly on the host, no context — against its restatement
in tests/keygen_ref.py, and that restatement's sigma columns against the ones tests/quotient_ref.py::satisfied_circuit builds
with one pow per cell.  halo2_proofs is not vendored in the reference: the yardstick is the definition in include/h2agg.h."""
import ctypes
import random

import pytest

from tests import keygen_ref as K
from tests import quotient_ref as Q

SHAPES = [(1, 0, 1), (1, 3, 6), (3, 4, 10), (7, 5, 26)]   # (m, k, usable)


def handmade_copies(m, k, usable):
    """the cases the merge rule distinguishes, over the usable cells in column-major order"""
    n = 1 << k
    c = [(j, i) for j in range(m) for i in range(usable)]
    if len(c) < 2:
        return [c[0] + c[0]] if c else []               # (1, 0): the one cell copied to itself — a copy inside one cycle
    out = [c[0] + c[1],                                 # equal sizes 1 and 1: the tie rule, the right one is merged
           c[0] + c[1],                                 # a repeated copy
           c[1] + c[0]]                                 # a copy inside one cycle
    if len(c) >= 6:
        out += [c[2] + c[3],
                c[4] + c[2],                            # left cycle of 1, right cycle of 2: the smaller LEFT one is merged
                c[5] + c[4],                            # 1 into 3
                c[0] + c[3]]                            # 2 against 4: the left is the smaller again
        rest = c[6:]
        half = len(rest) // 2
        a, b = rest[:half], rest[half:2 * half]
        out += [a[t] + a[t + 1] for t in range(half - 1)]            # a long chain: one large cycle
        out += [b[t + 1] + b[t] for t in range(half - 1)]            # a second one, grown from the other side
        if half:
            out += [a[half // 2] + b[half // 2],                     # two large cycles of equal size merge: the tie rule at size
                    b[0] + a[-1],                                    # inside the merged cycle
                    c[1] + a[0]]                                     # the six-cycle against the large one
    assert all(x < m and y < m and r < usable and s < usable and max(r, s) < n for x, r, y, s in out)
    return out


def copy_lists(m, k, usable):
    rng = random.Random(0xA55E + 64 * m + k)
    cells = m * usable
    yield "none", []
    yield "handmade", handmade_copies(m, k, usable)
    yield "sparse", K.random_copies(rng, m, k, usable, max(cells // 4, 1))
    yield "dense", K.random_copies(rng, m, k, usable, 3 * cells)
    yield "handmade then dense", handmade_copies(m, k, usable) + K.random_copies(rng, m, k, usable, 2 * cells)


@pytest.mark.parametrize("m,k,usable", SHAPES)
def test_assembly_is_halo2s(pkg, m, k, usable):
    for name, copies in copy_lists(m, k, usable):
        want = K.assembly_py(m, k, usable, copies)
        got = pkg.permutation_assembly(m, k, usable, copies)
        assert got == K.mapping_words(want), name
        flat = [x for q in copies for x in q]
        assert pkg.permutation_assembly(m, k, usable, (ctypes.c_uint32 * max(len(flat), 1))(*flat) if flat else b"") == got, name
        # what the result means, whatever the order of the merges: a valid mapping whose cycles are the copies' classes
        assert K.is_valid_mapping(want, m, k, usable), name
        assert K.cycles_of(want, m, k) == K.classes_of(m, k, copies), name


def test_the_copies_show_in_the_mapping(pkg):
    """two lists with the same classes give different mappings — which cells a copy names decides where the cycles are
    joined (which representative is merged only decides the cost) — so the bytes pin more than the classes do"""
    m, k, usable = 1, 3, 8
    a = [(0, 0, 0, 1), (0, 1, 0, 2)]     # 0 -> 1 -> 2 -> 0
    b = [(0, 0, 0, 1), (0, 0, 0, 2)]     # 0 -> 2 -> 1 -> 0
    ma, mb = pkg.permutation_assembly(m, k, usable, a), pkg.permutation_assembly(m, k, usable, b)
    assert ma == K.mapping_words(K.assembly_py(m, k, usable, a)) and mb == K.mapping_words(K.assembly_py(m, k, usable, b))
    assert ma != mb and K.classes_of(m, k, a) == K.classes_of(m, k, b)


def raw_call(pkg, m, k, usable, copies, ncopies, out_words):
    lib = pkg.load_library()
    out = (ctypes.c_uint32 * out_words)(*([0xA5A5A5A5] * out_words))
    arr = None if copies is None else (ctypes.c_uint32 * max(len(copies), 1))(*copies)
    rc = lib.h2agg_permutation_assembly(m, k, usable, arr, ncopies, out)
    return rc, all(w == 0xA5A5A5A5 for w in out)


@pytest.mark.parametrize("what,m,k,usable,copies,ncopies", [
    ("k = 25", 1, 25, 4, [], 0),
    ("m = 0", 0, 3, 4, [], 0),
    ("m = 4097", 4097, 0, 1, [], 0),
    ("usable > n", 2, 3, 9, [], 0),
    ("null copies with a count", 2, 3, 6, None, 1),
    ("left column = m", 2, 3, 6, [0, 0, 1, 1, 2, 0, 0, 0], 2),
    ("right column = m", 2, 3, 6, [0, 0, 1, 1, 0, 0, 2, 0], 2),
    ("left row = usable", 2, 3, 6, [0, 0, 1, 1, 1, 6, 0, 0], 2),
    ("right row = usable", 2, 3, 6, [0, 0, 1, 1, 1, 0, 0, 6], 2),
    ("row = n", 2, 3, 8, [0, 8, 1, 0], 1),
    ("usable = 0 refuses every copy", 2, 3, 0, [0, 0, 0, 0], 1),
])
def test_assembly_refusals_leave_the_output_alone(pkg, what, m, k, usable, copies, ncopies):
    rc, untouched = raw_call(pkg, m, k, usable, copies, ncopies, 64)
    assert rc == pkg.ERR_INVALID, what
    assert untouched, what


def test_assembly_refuses_a_null_mapping_and_accepts_the_limits(pkg):
    lib = pkg.load_library()
    assert lib.h2agg_permutation_assembly(1, 0, 1, None, 0, None) == pkg.ERR_INVALID
    rc, untouched = raw_call(pkg, 1, 0, 1, None, 0, 2)                 # null copies with no count is fine
    assert rc == pkg.OK and not untouched
    got = pkg.permutation_assembly(pkg.PERM_MAX_COLUMNS, 0, 1, [(0, 0, 4095, 0)])
    assert got == K.mapping_words(K.assembly_py(4096, 0, 1, [(0, 0, 4095, 0)]))
    with pytest.raises(pkg.H2AggError) as ei:
        pkg.permutation_assembly(3, 4, 10, [(0, 0, 3, 0)])
    assert ei.value.code == pkg.ERR_INVALID
    with pytest.raises(ValueError):
        pkg.permutation_assembly(3, 4, 10, [(0, 0, 1)])
    with pytest.raises(ValueError):
        pkg.permutation_assembly(3, 4, 10, bytes(12))


def test_reference_sigmas_are_the_scaffolds():
    """sigmas_py (running products) of the mapping made of satisfied_circuit's classes == the sigma columns satisfied_circuit
    builds with pow per cell; and the assembly over the same classes is valid with the same cycles"""
    k = 5
    cs, lag, _polys, _sc = Q.satisfied_circuit(random.Random(0xD00 + k), k, 5)
    n, u = cs.n, cs.n - cs.blinding_factors - 1
    columns = [lag[kind][col] for kind, col in cs.permutation_columns]
    m = len(columns)
    classes = {}
    for j, colv in enumerate(columns):
        for i in range(u):
            classes.setdefault(colv[i], []).append((j, i))
    mapping = K.identity_mapping(m, k)
    for cells in classes.values():
        for pos, (j, i) in enumerate(cells):
            mapping[j * n + i] = cells[(pos + 1) % len(cells)]
    assert K.is_valid_mapping(mapping, m, k, u)
    assert K.sigmas_py(mapping, m, k) == lag["sigma"]
    copies = K.copies_from_classes(classes.values())
    built = K.assembly_py(m, k, u, copies)
    assert K.is_valid_mapping(built, m, k, u) and K.cycles_of(built, m, k) == K.cycles_of(mapping, m, k)


def test_invalid_mapping_generator():
    for name, mp, _in_range in K.invalid_mappings(random.Random(7), 3, 4, 10):
        assert not K.is_valid_mapping(mp, 3, 4, 10), name
