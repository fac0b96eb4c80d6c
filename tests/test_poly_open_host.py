"""CPU: the grouping rule of the multiopen prover (poly.group_queries) against a literal restatement of the verifier's
(halo2-snark-aggregator-api/src/systems/halo2/multiopen.rs:31-43), the prototypes of the opening entry points, and the
Python yardstick of the GPU tests (tests/poly_open_ref.py) against the definition as written."""
import importlib

import pytest

import __graft_entry__ as entry
from tests.poly_open_ref import BIG_Z, R, assert_division, horner, quotient_definition, quotient_py, random_input


@pytest.fixture(scope="module")
def poly(pkg):
    return importlib.import_module(entry.PKG_NAME + ".poly")


def group_like_multiopen_rs(queries):
    """multiopen.rs:31-43, line for line: `points` is a Vec of (rotation, point, Vec<schema>); for every query, look for the
    entry with the query's rotation (`points.iter_mut().find(|(rot, _, _)| *rot == rotation)`), push the schema there, or
    push a new entry at the end.  The point index plays the rotation's role, the polynomial index the schema's."""
    points = []
    for schema, rotation in queries:
        pos = None
        for i, (rot, _members) in enumerate(points):
            if rot == rotation:
                pos = i
                break
        if pos is not None:
            points[pos][1].append(schema)
        else:
            points.append((rotation, [schema]))
    return points


CASES = [
    # interleaved points
    ([(0, 2), (1, 0), (2, 2), (3, 1), (4, 0), (0, 1)], [(2, [0, 2]), (0, [1, 4]), (1, [3, 0])]),
    # a repeated query stays repeated (its polynomial counts twice, with two powers of v)
    ([(3, 1), (3, 1), (0, 1), (3, 0)], [(1, [3, 3, 0]), (0, [3])]),
    # point 1 of three is named by no query: no group for it
    ([(0, 2), (1, 2), (0, 0)], [(2, [0, 1]), (0, [0])]),
    # one query
    ([(7, 5)], [(5, [7])]),
    ([], []),
]


@pytest.mark.parametrize("queries,want", CASES)
def test_group_queries_is_the_verifiers_rule(poly, queries, want):
    got = poly.group_queries(queries)
    assert got == want
    assert got == group_like_multiopen_rs(queries)
    assert sum(len(m) for _pt, m in got) == len(queries)
    assert len({pt for pt, _m in got}) == len(got)


def test_group_queries_scrambled(poly):
    import random
    rng = random.Random(0x6C0)
    for _ in range(50):
        queries = [(rng.randrange(6), rng.randrange(4)) for _ in range(rng.randrange(1, 14))]
        assert poly.group_queries(queries) == group_like_multiopen_rs(queries)


def test_the_prototypes_exist(pkg):
    names = set(pkg.exported_symbols())
    for fn in ("h2agg_fr_poly_eval", "h2agg_fr_poly_eval_device", "h2agg_fr_poly_divide", "h2agg_fr_poly_divide_device",
               "h2agg_kzg_multiopen", "h2agg_kzg_multiopen_device"):
        assert fn in names, fn
        assert getattr(pkg.load_library(), fn).argtypes is not None
    for method in ("fr_poly_eval", "fr_poly_eval_device", "fr_poly_divide", "fr_poly_divide_device", "kzg_multiopen",
                   "kzg_multiopen_device"):
        assert callable(getattr(pkg.H2Agg, method)), method
    assert pkg.FR_POLY_CHUNK == 11


def test_poly_functions_exist(poly):
    for fn in ("eval_polynomial", "kate_division", "group_queries", "multiopen_prove"):
        assert callable(getattr(poly, fn)), fn


def test_quotient_py_is_the_definition():
    for k in range(0, 7):
        a = random_input(100 + k, k)
        for z in (0, 1, R - 1, BIG_Z):
            assert quotient_py(a, z) == quotient_definition(a, z), (k, z)
            assert_division(a, z, quotient_py(a, z), horner(a, z))
