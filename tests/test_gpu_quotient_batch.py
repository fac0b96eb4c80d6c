"""GPU: h2agg_quotient over the batched transform — a coset's forward transforms are one launch per pass over the table of the
caller's slabs, in chunks of as many columns as the work array holds.  Whatever the chunk, the pieces are the same bytes, and
those are quotient_py's (tests/quotient_ref.py).  The circuits and builders are those of tests/test_gpu_quotient.py."""
import importlib
import random

import pytest

import __graft_entry__ as entry
from tests import quotient_ref as Q
from tests.test_gpu_quotient import BF, cols, make_vk, quotient_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def poly(pkg):
    return importlib.import_module(entry.PKG_NAME + ".poly")


@pytest.fixture(scope="module")
def verifier(pkg):
    return importlib.import_module(entry.PKG_NAME + ".verifier")


def check_every_chunk(eng, poly, vk, polys, sc, want, local):
    try:
        eng.debug_configure("fr_fft_local", local)
        unforced = quotient_host(eng, poly, vk, polys, sc)
        assert unforced == cols(want), "unforced"
        for chunk in (1, 3):
            eng.debug_configure("fr_fft_batch_chunk", chunk)
            assert quotient_host(eng, poly, vk, polys, sc) == unforced, chunk
    finally:
        eng.debug_configure("fr_fft_batch_chunk", 0)
        eng.debug_configure("fr_fft_local", 0)


def test_satisfied_circuit_with_lookup_and_permutation_sets(eng, poly, verifier):
    """the satisfied circuit at k = 5: gates, one lookup, four permutation sets (the last ragged) — eight slabs and the
    Lagrange rows in the segment table, chunks of 3 cutting through slabs"""
    k, degree = 5, 4
    cs, _lag, polys, sc = Q.satisfied_circuit(random.Random(0xD00 + k), k, degree)
    want, H = Q.quotient_py(cs, *Q.quotient_args(polys, sc))
    assert not any(H[(degree - 1) << k:])
    assert all(polys[kind] for kind in Q.POLY_KINDS), "every kind of slab is there"
    vk = make_vk(eng, verifier, cs)
    try:
        check_every_chunk(eng, poly, vk, polys, sc, want, 0)
    finally:
        vk.close()


def test_multi_pass_batch_inside_the_quotient(eng, poly, verifier):
    """fr_fft_local = 2 at k = 4, degree 6: the coset batch is two passes, the extended inverse four"""
    k, degree, n_perm, n_lookups, with_gates, n_challenges = 4, 6, 5, 1, True, 2
    rng = random.Random(0xD3B)
    cs = Q.random_shape(rng, k, degree, n_perm, n_lookups, with_gates, BF, n_challenges)
    polys, sc = Q.random_inputs(rng, cs), Q.random_scalars(rng, n_challenges)
    want, _H = Q.quotient_py(cs, *Q.quotient_args(polys, sc))
    vk = make_vk(eng, verifier, cs)
    try:
        check_every_chunk(eng, poly, vk, polys, sc, want, 2)
    finally:
        vk.close()
