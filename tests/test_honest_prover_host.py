"""CPU: honest proofs through the oracle's verifier.  tests/honest_prover.py's driver over PyStages — the restatements of
tests/grand_product_ref.py, lookup_permute_ref.py, quotient_ref.py, poly_open_ref.py and keygen_ref.py composed into a prover —
writes a proof from a witness; oracle/verifier.py::verify_aggregation_proofs_in_chip and the pairing check must accept it,
and must reject (with a False pairing, not an exception) a proof of a broken witness, a wrong instance value, and every proof
written under one of the misreadings of the sensitivity table: the conventions the restatements recall from halo2 are
thereby held against the part of the project that is read against the reference line by line."""
import random

import pytest

from tests import honest_prover as HP
from tests.grand_product_ref import DELTA, R

TAU = random.Random(0x7A0).randrange(1, R)
SHAPES = [(5, 4), (5, 5), (6, 6)]           # extended domains of 2, 2 and 3 bits; 4, 3 and 2 permutation sets


@pytest.fixture(scope="module")
def world():
    """setups (one tau: proofs of both k share [tau]_2), circuits, the stages' memo, and one honest proof per shape — built
    once, shared, left unchanged"""
    class World:
        setups = {k: HP.Setup(k, TAU, HP.INSTANCE_ROWS) for k in (5, 6)}
        circuits = {(k, d): HP.make_circuit(random.Random(0xD00 + 16 * k + d), k, d) for k, d in SHAPES}
        memo = {}
        proofs = {}

        def prove(self, shape, circuit=None, seed=1, stages_cls=HP.PyStages, **kw):
            setup = self.setups[shape[0]]
            return HP.prove(circuit or self.circuits[shape], setup, stages_cls(setup, self.memo), random.Random(seed), **kw)

        def accepts(self, *groups, instances=None):
            """groups: lists of proofs, one list per circuit"""
            cps = [HP.circuit_proofs("circuit%d" % i, self.setups[g[0].cs.k], g, instances) for i, g in enumerate(groups)]
            return HP.oracle_accepts(self.setups[5], cps)
    w = World()
    for shape in SHAPES:
        w.proofs[shape] = w.prove(shape)
    return w


def test_the_shapes_are_the_ones_meant(world):
    got = [(HP.Q.extended_k(k, d), world.circuits[(k, d)].cs.num_permutation_sets) for k, d in SHAPES]
    assert got == [(2, 4), (2, 3), (3, 2)]
    for c in world.circuits.values():
        assert len(c.cs.permutation_columns) % c.cs.chunk_len, "the last set is ragged"
        assert any(r == 1 for _c, r in c.cs.advice_queries)


@pytest.mark.parametrize("shape", SHAPES)
def test_honest_proofs_are_accepted(world, shape):
    p = world.proofs[shape]
    assert len([f for f in p.fields if f[0].startswith("W ")]) == 4
    assert world.accepts([p])
    assert p.data == world.prove(shape).data, "the prover is deterministic"


def test_aggregations_of_honest_proofs_are_accepted(world):
    first = world.proofs[(5, 4)]
    second = world.prove((5, 4), seed=2)
    assert second.data != first.data and second.cs.vk_scalar == first.cs.vk_scalar
    assert world.accepts([first, second]), "two proofs of one circuit"
    assert world.accepts([first], [world.proofs[(6, 6)]]), "two circuits, k = 5 and k = 6"
    assert world.accepts([first, second], [world.proofs[(5, 5)]])


def test_zero_blinding_is_accepted(world):
    p = world.prove((5, 4), blinding=None)
    assert p.data != world.proofs[(5, 4)].data
    assert world.accepts([p])


@pytest.mark.parametrize("shape", SHAPES)
def test_a_changed_gate_cell_is_rejected(world, shape):
    """row 3 of c: a multiplication row"""
    assert not world.accepts([world.prove(shape, HP.broken_gate_cell(world.circuits[shape]))])


@pytest.mark.parametrize("shape", SHAPES)
def test_a_changed_copied_cell_is_rejected(world, shape):
    """a cell of a on a row where no selector is on: the gates hold, only the permutation argument can notice"""
    c = world.circuits[shape]
    col, row = HP.copied_cell_off_the_gates(c)
    assert col == 0 and not c.lag["fixed"][0][row] and not c.lag["fixed"][1][row], "a cell of a that no gate reads"
    assert not world.accepts([world.prove(shape, HP.broken_copied_cell(c))])


@pytest.mark.parametrize("shape", SHAPES)
def test_an_instance_value_that_was_not_proven_is_rejected(world, shape):
    p = world.proofs[shape]
    wrong = [[list(col) for col in inner] for inner in p.instances]
    wrong[0][0][1] = (wrong[0][0][1] + 1) % R
    assert not world.accepts([p], instances=[wrong])


# ---------------------------------------------------------------------------------------------- the sensitivity table
class EverySetAtDeltaZero(HP.PyStages):
    def set_start(self, s, chunk_len, previous_last):
        return 1, previous_last


class EverySetStartsAtOne(HP.PyStages):
    def set_start(self, s, chunk_len, previous_last):
        return pow(DELTA, s * chunk_len, R), 1


class UsableOffByOne(HP.PyStages):
    def product_rows(self, usable):
        return usable + 1


class TableLeftUnpermuted(HP.PyStages):
    def permute(self, a, s, k, usable, blinding):
        _ap, sp = super().permute(a, s, k, usable, blinding)
        ap = sorted(a[:usable])
        return ap + _ap[usable:], list(s[:usable]) + sp[usable:]


class PiecesAgainstTheLagrangeTable(HP.PyStages):
    def commit_coeff(self, cols, k):
        if len(cols) == self.cs.quotient_poly_degree:
            return super().commit_lagrange(cols, k)
        return super().commit_coeff(cols, k)


class AdviceAgainstTheMonomialTable(HP.PyStages):
    def commit_lagrange(self, cols, k):
        if self.cs is not None and len(cols) == self.cs.num_advice_columns:     # (the key is made before it is loaded)
            return super().commit_coeff(cols, k)
        return super().commit_lagrange(cols, k)


class PermutedInputOpenedForward(HP.Driver):
    def point(self, x, omega, rotation):
        return super().point(x, omega, 1 if rotation == -1 else rotation)


class LastOpenedOneRowShort(HP.Driver):
    def point(self, x, omega, rotation):
        return super().point(x, omega, rotation + 1 if rotation < -1 else rotation)


class PiecesReversed(HP.Driver):
    def h_commitment_order(self, commitments):
        return list(reversed(commitments))


class WByAscendingRotation(HP.Driver):
    def w_order(self, rotations, ws):
        assert sorted(rotations) != list(rotations)
        return [w for _r, w in sorted(zip(rotations, ws), key=lambda rw: rw[0])]


MISREADINGS = {
    "every permutation set started at delta^0": dict(stages_cls=EverySetAtDeltaZero),
    "set s > 0 started at 1": dict(stages_cls=EverySetStartsAtOne),
    "usable off by one, l_last one row late": dict(stages_cls=UsableOffByOne),
    "a' opened at omega x": dict(driver=PermutedInputOpenedForward()),
    "h pieces committed in reverse order": dict(driver=PiecesReversed()),
    "W points by ascending rotation": dict(driver=WByAscendingRotation()),
    "s' left equal to s": dict(stages_cls=TableLeftUnpermuted),
    "x_last one row short": dict(driver=LastOpenedOneRowShort()),
    "h pieces committed against g_lagrange": dict(stages_cls=PiecesAgainstTheLagrangeTable),
    "advice committed against g": dict(stages_cls=AdviceAgainstTheMonomialTable),
}


@pytest.mark.parametrize("name", list(MISREADINGS))
def test_a_misread_convention_is_rejected(world, name):
    """each proof differs from the accepted one of test_honest_proofs_are_accepted in ONE convention (same witness, same seed)"""
    shape = (5, 4)
    p = world.prove(shape, **MISREADINGS[name])
    assert p.data != world.proofs[shape].data, "the misreading changes nothing here: the check would be vacuous"
    assert not world.accepts([p])
