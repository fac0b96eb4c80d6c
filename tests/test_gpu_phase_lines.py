"""GPU: the line h2agg_last_phases gives behind every call that splits itself by events on the context's stream (debug key
phases): " name=%.4f" per phase, the names and their order as include/h2agg.h states them.  Every call but
h2agg_permutation_sigmas prints all its names (0.0000 for a phase that did not run: tools/poly_open_time.py and
tools/shplonk_time.py read the values by position); the sigmas print the phases that finished.  One call of each at the
smallest shapes the reference restatements build; the results with the key on equal those with the key off.

With the key off no call touches the line: it is empty on a fresh context and otherwise stays as the last keyed call left it."""
import importlib
import random
import re

import pytest

import __graft_entry__ as entry
from oracle import bn254 as O
from tests import honest_prover as HP
from tests import keygen_ref as K
from tests import quotient_ref as Q
from tests import witness_check_ref as W
from tests.fr_bytes import enc, fe
from tests.test_gpu_keygen import DELTA, raw_sigmas
from tests.test_gpu_quotient import make_vk, quotient_host
from tests.test_gpu_shplonk import Params, case_points

pytestmark = pytest.mark.gpu

R = Q.R
K_OPEN = 4


def line_re(names):
    return re.compile("^" + "".join(r" %s=\d+\.\d{4}" % name for name in names) + "$")


def assert_line(line, names):
    assert line_re(names).match(line), (names, line)


@pytest.fixture(scope="module")
def poly(pkg):
    return importlib.import_module(entry.PKG_NAME + ".poly")


@pytest.fixture(scope="module")
def verifier(pkg):
    return importlib.import_module(entry.PKG_NAME + ".verifier")


@pytest.fixture(scope="module")
def ctx(pkg):
    """a context of this module's own: its line starts empty"""
    e = pkg.H2Agg(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def par(ctx):
    p = Params(ctx, K_OPEN)
    yield p
    p.free()


class keyed:
    """debug key phases on for the block"""

    def __init__(self, e):
        self.e = e

    def __enter__(self):
        self.e.debug_configure("phases", 1)

    def __exit__(self, *exc):
        self.e.debug_configure("phases", 0)


def test_a_fresh_context_has_an_empty_line_and_calls_without_the_key_leave_it(ctx, par):
    assert ctx.last_phases() == ""
    queries, zs = case_points("sets_of_1_2_3", par.k, 0)
    want = ctx.kzg_multiopen(par.g, par.slab, par.k, queries, enc(zs), fe(par.v))
    assert ctx.last_phases() == ""
    with keyed(ctx):
        assert ctx.kzg_multiopen(par.g, par.slab, par.k, queries, enc(zs), fe(par.v)) == want
        line = ctx.last_phases()
    assert_line(line, ["combine", "divide", "commit"])
    assert ctx.kzg_multiopen(par.g, par.slab, par.k, queries, enc(zs), fe(par.v)) == want
    assert ctx.last_phases() == line, "a call without the key leaves the line as the last keyed call set it"


def test_shplonk_begin_and_finish(ctx, par):
    queries, zs = case_points("sets_of_1_2_3", par.k, 0)
    ev = ctx.fr_poly_eval(par.slab, par.k, queries, enc(zs))

    def run():
        h1, obj = ctx.kzg_shplonk_begin(par.g, par.slab, par.k, queries, enc(zs), ev, fe(par.y), fe(par.v))
        try:
            begin = ctx.last_phases()
            h2 = ctx.kzg_shplonk_finish(obj, fe(par.u))
            return (h1, h2), begin, ctx.last_phases()
        finally:
            ctx.kzg_shplonk_destroy(obj)

    want, before, after = run()
    with keyed(ctx):
        got, begin, finish = run()
    assert got == want
    assert_line(begin, ["stage", "numerators", "divide", "commit"])
    assert_line(finish, ["combine", "divide", "commit"])
    assert run() == (want, finish, finish), "the key is off again: the line stays"
    assert before == after, "and it stayed while the key was off before"


def test_quotient_of_a_circuit_without_lookups_still_names_them(ctx, poly, verifier):
    rng = random.Random(0x9A5E)
    cs = Q.random_shape(rng, 4, 3, 2, 0, True, 5, 0)
    assert not cs.lookups
    polys, sc = Q.random_inputs(rng, cs), Q.random_scalars(rng, 0)
    vk = make_vk(ctx, verifier, cs)
    try:
        want = quotient_host(ctx, poly, vk, polys, sc)
        with keyed(ctx):
            assert quotient_host(ctx, poly, vk, polys, sc) == want
            line = ctx.last_phases()
    finally:
        vk.close()
    # (not 0.0000: the store of the coset's extended values is queued behind the lookups and its time counts as theirs)
    assert_line(line, ["forward", "gates", "permutation", "lookups", "inverse"])


def test_witness_check(ctx, verifier):
    k, degree = 5, 4
    rng = random.Random(0xD00 + 16 * k + degree)
    circuit = HP.make_circuit(rng, k, degree)
    mapping = K.assembly_py(len(circuit.cs.permutation_columns), k, circuit.usable, circuit.copies)
    theta = rng.randrange(R)
    vk = verifier.VerifyingKey(ctx, verifier.encode_vk(circuit.cs, O.aff_to_bytes))
    a, f, i = (b"".join(enc(c) for c in circuit.lag[kind]) or None for kind in ("advice", "fixed", "instance"))
    call = lambda: ctx.witness_check(vk, W.WC_ALL, a, f, i, None, fe(theta), K.mapping_words(mapping))
    try:
        want = call()
        with keyed(ctx):
            assert call() == want
            line = ctx.last_phases()
    finally:
        vk.close()
    assert want[3] == 0
    assert_line(line, ["gates", "permutation", "lookups", "report"])


def test_sigmas_name_the_phases_that_finished(ctx, pkg):
    m, k, usable = 7, 5, 26
    rng = random.Random(0x51A + 64 * m + k)
    words = K.mapping_words(K.assembly_py(m, k, usable, K.random_copies(rng, m, k, usable, m * usable)))
    size = 32 * m << k
    bad = {in_range: K.mapping_words(mp) for _name, mp, in_range in K.invalid_mappings(random.Random(0xBAD), m, k, usable)}
    want = raw_sigmas(pkg, ctx, words, m, k, usable, DELTA, size)
    assert want[0] == pkg.OK
    with keyed(ctx):
        assert raw_sigmas(pkg, ctx, words, m, k, usable, DELTA, size) == want
        assert_line(ctx.last_phases(), ["stage", "sigma", "inverse", "copy"])
        # refused by the device's verdict: nothing was copied back
        assert raw_sigmas(pkg, ctx, bad[True], m, k, usable, DELTA, size)[0] == pkg.ERR_INVALID
        assert_line(ctx.last_phases(), ["stage", "sigma", "inverse"])
        full = raw_sigmas(pkg, ctx, words, m, k, usable, DELTA, size)
        assert full == want and ctx.last_phases() != ""
        # refused by the host's scan of the mapping: no device phase ran, the line is empty
        assert raw_sigmas(pkg, ctx, bad[False], m, k, usable, DELTA, size)[0] == pkg.ERR_INVALID
        assert ctx.last_phases() == ""
        assert raw_sigmas(pkg, ctx, words, m, k, usable, DELTA, size) == want
        line = ctx.last_phases()
    assert_line(line, ["stage", "sigma", "inverse", "copy"])
    assert raw_sigmas(pkg, ctx, bad[False], m, k, usable, DELTA, size)[0] == pkg.ERR_INVALID
    assert ctx.last_phases() == line, "a call without the key leaves the line"
