"""CPU: the Shplonk verifier restated over oracle/ (tests/shplonk_verifier_ref.py), held against two provers that do not share
its code: the trapdoor prover with a Shplonk tail (tests/toy_prover_shplonk.py: H2 solved for in the exponent) over the three
shapes of tests/test_verifier_pipeline.py, and the honest prover (tests/honest_prover_shplonk.py over PyStagesShplonk, whose
openings are tests/shplonk_ref.py's Opening: the PROVER's definition).  Honest proofs are accepted, broken ones rejected by a
False verdict, and every row of the sensitivity table — the verifier misreading ONE convention — rejects the honest proof: the
conventions prover and verifier share are thereby pinned to one another, not to a shared helper."""
import random

import pytest

from oracle import bn254 as O
from oracle import pairing as E
from oracle import schema as S
from oracle import verifier as V
from tests import honest_prover as HP
from tests import honest_prover_shplonk as HS
from tests import shplonk_ref as SR
from tests import shplonk_verifier_ref as SV
from tests import toy_prover_hash as TH
from tests import toy_prover_shplonk as TS
from tests.grand_product_ref import R
from tests.test_verifier_pipeline import SHAPES as TOY_SHAPES

TAU = random.Random(0x7A0).randrange(1, R)
SHAPES = [(5, 4), (5, 5), (6, 6)]


def accepted(setup, left, right):
    """e(left, [tau]_2) = e(right, [1]_2) iff tau * left = right (tests/test_exceptional_points_host.py::accepted)"""
    return TH.CrefEccChip().scalar_mul(None, setup.tau, left) == right


# ---------------------------------------------------------------------------------------------- trapdoor proofs
@pytest.fixture(scope="module")
def toy():
    """one Shplonk proof of each of the three shapes, with the discrete logarithms of every point in them"""
    dlogs = {}
    setup, circuits = TS.make_batch(0x5B1, TOY_SHAPES, 1, dlogs=dlogs)
    return setup, circuits, dlogs


def test_the_toy_shapes_cover_what_they_should():
    assert TOY_SHAPES[1].get("phases") == (0, 1) and TOY_SHAPES[1]["n_challenges"] == 2
    assert TOY_SHAPES[2]["n_lookups"] == 2 and TOY_SHAPES[2]["n_perm_columns"] == 0
    assert [s["degree"] for s in TOY_SHAPES] == [4, 3, 5]


def test_trapdoor_proofs_are_accepted_and_a_changed_evaluation_is_not(toy):
    setup, circuits, _dlogs = toy
    pairs = SV.verify_each(TH.CrefEccChip, circuits)
    assert len(pairs) == 3 and all(accepted(setup, l, r) for l, r in pairs)
    left, right, _lam = SV.verify_aggregation(TH.CrefEccChip(), circuits)
    assert accepted(setup, left, right), "three circuits in one aggregation"
    c = circuits[0]
    inst, data = c.proofs[0]
    at = len(data) - 64 - 32                                # the last evaluation: two compressed points follow it
    bad = data[:at] + O.fe_to_bytes((O.fe_from_bytes(data[at:at + 32]) + 1) % R) + data[at + 32:]
    twin = V.CircuitProofs(c.name, c.cs, c.g_lagrange, [(inst, bad)])
    (l, r), = SV.verify_each(TH.CrefEccChip, [twin])
    assert not accepted(setup, l, r)


def test_the_sets_of_the_toy_shapes(toy):
    """several sets, sets of one, two and three points that share points, and the vanishing query in the set of x alone"""
    _setup, circuits, _dlogs = toy
    conv = SV.Conventions()
    for c in circuits:
        inst, data = c.proofs[0]
        _plain, com = V.assign_instance_commitment(TH.CrefEccChip(), S.OracleCtx(), inst, c.cs, c.g_lagrange)
        _t, vp, _tail = SV.build_params_shplonk(data, S.OracleEccChip(), S.OracleCtx(), com, c.cs, "k")
        qs = V.queries(vp)
        ids = [conv.poly_id(i, q[0], q[2]) for i, q in enumerate(qs)]
        sets = conv.sets(ids, [q[0] for q in qs])
        assert sorted(sets[0][0]) == [0] and len(sets) >= 4
        assert {len(pts) for pts, _m in sets} >= {1, 2, 3}
        assert sum(1 for m in ids if isinstance(m, tuple)) == 1 and any(isinstance(m, tuple) for m in sets[0][1])


def test_the_pair_is_the_provers_f_plus_u_h2_in_the_exponent(toy):
    """the restatement's (left, right), evaluated in the exponent, against shplonk_ref.Opening.verifier_f: the scalars of the
    PROVER's restatement over the same queries, commitments and values"""
    setup, circuits, dlogs = toy
    chip = TS.DlogChip(dlogs)
    for c in circuits:
        inst, data = c.proofs[0]
        ctx = S.OracleCtx()
        _plain, com = V.assign_instance_commitment(TH.CrefEccChip(), ctx, inst, c.cs, c.g_lagrange)
        _t, vp, tail = SV.build_params_shplonk(data, S.OracleEccChip(), ctx, com, c.cs, "k")
        qs = V.queries(vp)
        proof = SV.shplonk_multi_open_proofs("k", qs, None, tail.h1, tail.h2, tail.y, tail.v, tail.u)
        left, right, _names = S.evaluate_multiopen_proof(ctx, S.OracleFieldChip(), chip, proof)
        # every query as (polynomial, point index), its commitment's logarithm and its value, read off its schema
        conv = SV.Conventions()
        polys, rots, zs, queries, commit, evals = [], [], [], [], {}, []
        for i, (rot, pt, s) in enumerate(qs):
            m = conv.poly_id(i, rot, s)
            if m not in polys:
                polys.append(m)
            if rot not in rots:
                rots.append(rot)
                zs.append(pt)
            cd = ev = 0
            for name, p, sc in s.eval_prepare(ctx, S.OracleFieldChip(), 1, None):
                if name == "":
                    ev = (ev + sc) % R
                else:
                    cd = (cd + chip._d(p) * (1 if sc is None else sc)) % R
            queries.append((polys.index(m), rots.index(rot)))
            commit.setdefault(polys.index(m), cd)
            evals.append(ev)                                # a query is C + e and evaluate_multiopen_proof subtracts e G: the value is e
        op = SR.Opening([[0]] * len(polys), zs, queries, tail.y, tail.v, evals=evals)
        f = op.verifier_f(tail.u, commit, chip._d(tail.h1))
        assert left == chip._d(tail.h2)
        assert right == (f + tail.u * chip._d(tail.h2)) % R
        assert setup.tau * left % R == right


# ---------------------------------------------------------------------------------------------- honest proofs
@pytest.fixture(scope="module")
def world():
    class World:
        setups = {k: HP.Setup(k, TAU, HP.INSTANCE_ROWS) for k in (5, 6)}
        circuits = {(k, d): HP.make_circuit(random.Random(0xD00 + 16 * k + d), k, d) for k, d in SHAPES}
        memo = {}
        proofs = {}

        def prove(self, shape, circuit=None, seed=1):
            setup = self.setups[shape[0]]
            return HS.prove_shplonk(circuit or self.circuits[shape], setup, HS.PyStagesShplonk(setup, self.memo), random.Random(seed))

        def pair(self, *groups, instances=None, conv=None):
            cps = [HP.circuit_proofs("circuit%d" % i, self.setups[g[0].cs.k], g, instances) for i, g in enumerate(groups)]
            left, right, _lam = SV.verify_aggregation(TH.CrefEccChip(), cps, conv=conv)
            return left, right

        def accepts(self, *groups, **kw):
            return accepted(self.setups[5], *self.pair(*groups, **kw))
    w = World()
    for shape in SHAPES:
        w.proofs[shape] = w.prove(shape)
    return w


@pytest.mark.parametrize("shape", SHAPES)
def test_honest_proofs_are_accepted_by_the_pairing(world, shape):
    p = world.proofs[shape]
    assert [f[0] for f in p.fields[-2:]] == ["H1", "H2"] and not any(f[0].startswith("W ") for f in p.fields)
    gwc = HP.prove(world.circuits[shape], world.setups[shape[0]], HP.PyStages(world.setups[shape[0]], world.memo), random.Random(1))
    assert p.data[:-64] == gwc.data[:-4 * 32], "identical up to the evaluations"
    left, right = world.pair([p])
    setup = world.setups[shape[0]]
    assert E.pairing_check([(left, setup.s_g2), (right, E.g2_neg(setup.g2))])
    assert accepted(setup, left, right), "the trapdoor verdict is the pairing's"


def test_aggregations_are_accepted(world):
    first, second = world.proofs[(5, 4)], world.prove((5, 4), seed=2)
    assert second.data != first.data
    assert world.accepts([first, second]), "two proofs of one circuit"
    assert world.accepts([first], [world.proofs[(6, 6)]]), "two circuits, k = 5 and k = 6"


@pytest.mark.parametrize("what", ["gate cell", "copied cell"])
def test_a_broken_witness_is_rejected_by_verdict(world, what):
    c = world.circuits[(5, 4)]
    bad = HP.broken_gate_cell(c) if what == "gate cell" else HP.broken_copied_cell(c)
    assert not world.accepts([world.prove((5, 4), bad)])


def test_a_wrong_instance_value_is_rejected_by_verdict(world):
    p = world.proofs[(5, 4)]
    wrong = [[list(col) for col in inner] for inner in p.instances]
    wrong[0][0][1] = (wrong[0][0][1] + 1) % R
    assert not world.accepts([p], instances=[wrong])


def test_one_bit_of_the_last_evaluation_is_rejected_by_verdict(world):
    p = world.proofs[(5, 4)]
    name, lo, _hi = [f for f in p.fields if f[0] == "permuted table evaluation"][0]
    assert p.fields[-3][0] == name, "the last evaluation: H1 and H2 follow it"
    data = bytearray(p.data)
    data[lo] ^= 1                                           # still canonical
    assert not world.accepts([HP.Proof(p.cs, p.instances, bytes(data), p.fields)])


# ---------------------------------------------------------------------------------------------- the sensitivity table
class YAndVExchanged(SV.Conventions):
    def challenges(self, y, v):
        return v, y


class VPowersInReverseSetOrder(SV.Conventions):
    def set_power(self, i, nsets):
        return nsets - 1 - i


class CLeftOut(SV.Conventions):
    def c(self, d, i):
        return 1


class TUndivided(SV.Conventions):
    def t(self, um_s0, um_all, d0):
        return SV._prod(um_all)


class ValueAtTheFirstPoint(SV.Conventions):
    def weights(self, zs, u):
        return [1] + [0] * (len(zs) - 1)


class UH2LeftOut(SV.Conventions):
    def with_h2(self, right, u, h2):
        return right


class YPowersRunOnAcrossSets(SV.Conventions):
    def poly_power(self, j, polys_before):
        return polys_before + j


class USqueezedBeforeH1(SV.Conventions):
    def read_tail(self, t, tail):
        u = t.squeeze_challenge_scalar()
        t.data = t.data + tail
        return t.read_point(), u, t.read_point()


class PolynomialsByCommitmentAndRotation(SV.Conventions):
    def poly_id(self, index, rotation, schema):
        return (super().poly_id(index, rotation, schema), rotation)


MISREADINGS = {
    "y and v exchanged": YAndVExchanged,
    "v powers in reverse set order": VPowersInReverseSetOrder,
    "c_i left out": CLeftOut,
    "t taken as Z_T(u) undivided": TUndivided,
    "r_ij(u) replaced by the value at the set's first point": ValueAtTheFirstPoint,
    "u H2 left out": UH2LeftOut,
    "y powers running on across sets": YPowersRunOnAcrossSets,
    "u squeezed before H1 is absorbed": USqueezedBeforeH1,
    "polynomials identified by (commitment, rotation)": PolynomialsByCommitmentAndRotation,
}


@pytest.mark.parametrize("name", list(MISREADINGS))
def test_a_misread_convention_is_rejected(world, name):
    """the honest (5, 4) proof, read by a verifier that differs from the accepted one in ONE convention"""
    p = world.proofs[(5, 4)]
    good = world.pair([p])
    bad = world.pair([p], conv=MISREADINGS[name]())
    assert bad != good, "the misreading changes nothing here: the check would be vacuous"
    assert not accepted(world.setups[5], *bad)
