"""GPU: Shplonk verification through every layer the GWC verification has — h2agg_schema_shplonk_multi_open, the key switch
h2agg_vk_set_multiopen, h2agg_verify_proofs and h2agg_verify_aggregation(_ex) from proof bytes.

The yardstick is tests/shplonk_verifier_ref.py (the definition of include/h2agg.h over oracle/, which
tests/test_shplonk_verifier_host.py holds against two provers): every pair is compared with it bit for bit.  Proofs come from
the trapdoor prover with a Shplonk tail (tests/toy_prover_shplonk.py) and from the honest prover over the device's stages
(tests/honest_prover_shplonk.py: poly.shplonk_prove), which must write the Python stages' proof byte for byte."""
import importlib
import random

import pytest

import __graft_entry__ as entry
from oracle import bn254 as O
from oracle import schema as S
from oracle import verifier as V
from tests import hash_transcript_ref as H
from tests import honest_prover as HP
from tests import honest_prover_shplonk as HS
from tests import shplonk_verifier_ref as SV
from tests import toy_prover as T
from tests import toy_prover_hash as TH
from tests import toy_prover_shplonk as TS
from tests.grand_product_ref import R
from tests.test_gpu_verify_each import oracle_pairs
from tests.test_pairing_capi import g2b
from tests.test_verifier_pipeline import SHAPES

pytestmark = pytest.mark.gpu

TAU = random.Random(0x7A0).randrange(1, R)
HONEST_SHAPES = [(5, 4), (5, 5), (6, 6)]
BIG = (12, 4)           # every row-scaled prover stage beyond one workgroup (tests/test_gpu_honest_proofs.py)
fe = O.fe_to_bytes


@pytest.fixture(scope="module")
def poly(pkg):
    return importlib.import_module(entry.PKG_NAME + ".poly")


@pytest.fixture(scope="module")
def ver(pkg):
    return importlib.import_module(entry.PKG_NAME + ".verifier")


@pytest.fixture(params=["device", "host"])
def backend(request, eng):
    """both sponge backends (h2agg_transcript_configure)"""
    eng.transcript_configure(request.param)
    yield request.param
    eng.transcript_configure("auto")


def pair_bytes(pairs):
    return [S.final_pair_bytes(left, right) for left, right in pairs]


# ---------------------------------------------------------------------------------------------- schema level
class Case:
    """queries (polynomial, rotation) over random commitments c * G and free values; the same case for the restatement and
    the library"""

    def __init__(self, seed, named, points=None, y=None, v=None, u=None, composite=False):
        rng = O.SplitMix64(seed)
        self.named = list(named)
        rots = []
        for _m, r in self.named:
            if r not in rots:
                rots.append(r)
        self.z = dict(points) if points else {}
        for r in rots:
            self.z.setdefault(r, rng.fr())
        polys = []
        for m, _r in self.named:
            if m not in polys:
                polys.append(m)
        self.polys, self.rots = polys, rots
        self.commit = {m: TH.g1_mul(rng.fr()) for m in polys}
        self.evals = [rng.fr() for _ in self.named]
        self.h1, self.h2 = TH.g1_mul(rng.fr()), TH.g1_mul(rng.fr())
        pick = lambda given: rng.fr() if given is None else given % R
        self.y, self.v, self.u = pick(y), pick(v), pick(u)
        self.extra = (rng.fr(), TH.g1_mul(rng.fr()), rng.fr()) if composite else None
        self.ids = [polys.index(m) for m, _r in self.named]

    def want(self):
        qs = [S.evaluation_query(r, "c_%s" % m, self.z[r], self.commit[m], e) for (m, r), e in zip(self.named, self.evals)]
        if self.extra:      # the first query becomes scalar * commit + commit + scalar
            s, c2, s2 = self.extra
            m, r = self.named[0]
            node = S.scalar(s) * S.commit(S.CommitQuery("c_%s" % m, self.commit[m], None)) + \
                S.commit(S.CommitQuery("c_extra", c2, None)) + S.scalar(s2)
            qs[0] = (r, self.z[r], node)
        proof = SV.shplonk_multi_open_proofs("c", qs, self.ids, self.h1, self.h2, self.y, self.v, self.u)
        ctx = S.OracleCtx()
        left, right, _names = S.evaluate_multiopen_proof(ctx, S.OracleFieldChip(), TH.CrefEccChip(), proof)
        return S.final_pair_bytes(left, right)

    def build(self, b, pkg):
        nodes = b.evaluation_queries(["c_%s" % m for m, _r in self.named], b"".join(O.aff_to_bytes(self.commit[m]) for m, _r in self.named),
                                     b"".join(fe(e) for e in self.evals))
        if self.extra:
            s, c2, s2 = self.extra
            m, _r = self.named[0]
            nodes[0] = b.scalar(fe(s)) * b.commit(pkg.CommitQuery("c_%s" % m, O.aff_to_bytes(self.commit[m]))) + \
                b.commit(pkg.CommitQuery("c_extra", O.aff_to_bytes(c2))) + b.scalar(fe(s2))
        return b.shplonk_multi_open("c", self.ids, [r for _m, r in self.named], b"".join(fe(self.z[r]) for _m, r in self.named), nodes,
                                    O.aff_to_bytes(self.h1), O.aff_to_bytes(self.h2), fe(self.y), fe(self.v), fe(self.u))

    def got(self, eng, pkg):
        b = pkg.SchemaBuilder(eng)
        try:
            left, right = self.build(b, pkg)
            l, r, _names = b.evaluate_multiopen_proof(left, right)
            return l + r
        finally:
            b.close()


SETS_123 = [("a", 0), ("b", 0), ("b", 1), ("c", 0), ("c", 1), ("c", -1), ("d", 0), ("e", 1), ("e", 0), ("f", -1), ("f", 1), ("f", 0)]
FIVE = [("a", 0)] + [("b", r) for r in (0, 1, -1, 2, -6)] + [("c", r) for r in (-6, 2, -1, 1, 0)] + [("d", 1)]
Z_123 = {0: 11, 1: 22, -1: 33}

SCHEMA_CASES = {
    "one polynomial at one point": dict(named=[("a", 0)]),
    "sets of 1, 2 and 3 points sharing points": dict(named=SETS_123),
    "a set of 5 points": dict(named=FIVE),
    "y = 0": dict(named=SETS_123, y=0),
    "v = 0": dict(named=SETS_123, v=0),
    "u = 0": dict(named=SETS_123, u=0),
    "y = v = u = 0 and the point of S_0 is 0": dict(named=SETS_123, points={0: 0}, y=0, v=0, u=0),
    "u a point of S_0": dict(named=SETS_123, points=Z_123, u=11),
    "a composite query node": dict(named=SETS_123, composite=True),
}


@pytest.mark.parametrize("name", list(SCHEMA_CASES))
def test_schema_pairs_match_the_restatement(eng, pkg, name):
    case = Case(0x5C0 + list(SCHEMA_CASES).index(name), **SCHEMA_CASES[name])
    assert case.got(eng, pkg) == case.want()


def test_u_in_s0_gives_t_zero_and_h1_drops_out(eng, pkg):
    a = Case(0x5D0, SETS_123, points=Z_123, u=11)
    b = Case(0x5D0, SETS_123, points=Z_123, u=11)
    b.h1 = TH.g1_mul(77)
    assert a.got(eng, pkg) == b.got(eng, pkg) == a.want()


@pytest.mark.parametrize("name,kw", [
    ("u a point of T \\ S_0", dict(named=SETS_123, points=Z_123, u=22)),
    ("two rotations of one set with equal points", dict(named=SETS_123, points={0: 5, 1: 5})),
    ("two rotations of different sets with equal points", dict(named=[("a", 0), ("b", 1)], points={0: 9, 1: 9})),
])
def test_inversions_of_zero(eng, pkg, name, kw):
    case = Case(0x5E0, **kw)
    with pytest.raises(ZeroDivisionError):
        case.want()
    with pytest.raises(pkg.DivisionByZero):
        case.got(eng, pkg)
    assert Case(0x5E1, SETS_123).got(eng, pkg) == Case(0x5E1, SETS_123).want(), "the context goes on"


def test_refusals(eng, pkg):
    big = Case(0x5F0, [("a", r) for r in range(33)])
    twice = Case(0x5F1, [("a", 0), ("b", 0), ("a", 0)])
    for case in (big, twice):
        with pytest.raises(ValueError):
            case.want()
        with pytest.raises(pkg.H2AggError) as ei:
            case.got(eng, pkg)
        assert ei.value.code == pkg.ERR_INVALID
    assert Case(0x5F2, [("a", r) for r in range(32)]).got(eng, pkg) == Case(0x5F2, [("a", r) for r in range(32)]).want(), "32 points are taken"
    b = pkg.SchemaBuilder(eng)
    try:
        ok = Case(0x5F3, [("a", 0)])
        with pytest.raises(pkg.H2AggError) as ei:       # an unknown node
            b.shplonk_multi_open("c", [0], [0], fe(1), [12345], O.aff_to_bytes(ok.h1), O.aff_to_bytes(ok.h2), fe(1), fe(2), fe(3))
        assert ei.value.code == pkg.ERR_INVALID
        with pytest.raises(pkg.H2AggError) as ei:       # no queries
            b.shplonk_multi_open("c", [], [], b"", [], O.aff_to_bytes(ok.h1), O.aff_to_bytes(ok.h2), fe(1), fe(2), fe(3))
        assert ei.value.code == pkg.ERR_INVALID
        l, r, _names = b.evaluate_multiopen_proof(*ok.build(b, pkg))
        assert l + r == ok.want(), "the schema stays usable"
    finally:
        b.close()


def test_the_third_witness(eng, pkg, poly):
    """poly.shplonk_final_pair: the scalars in Python integers and one g1_msm"""
    case = Case(0x600, SETS_123)
    commits = [O.aff_to_bytes(case.commit[m]) for m in case.polys]
    queries = [(case.polys.index(m), case.rots.index(r)) for m, r in case.named]
    left, right = poly.shplonk_final_pair(eng, commits, queries, b"".join(fe(case.z[r]) for r in case.rots), [fe(e) for e in case.evals],
                                          fe(case.y), fe(case.v), fe(case.u), O.aff_to_bytes(case.h1), O.aff_to_bytes(case.h2))
    assert left + right == case.got(eng, pkg) == case.want()


# ---------------------------------------------------------------------------------------------- from bytes
class Product:
    """the library's view of some circuits: one key per circuit with its transcript and multiopen kind, one g_lagrange table"""

    def __init__(self, eng, ver, setup, circuits, kinds=None, transcript="poseidon"):
        self.eng, self.ver = eng, ver
        self.table = eng.bases_upload(b"".join(O.aff_to_bytes(p) for p in setup.g_lagrange))
        kinds = kinds or ["shplonk"] * len(circuits)
        self.vks = [ver.VerifyingKey(eng, ver.encode_vk(c.cs, O.aff_to_bytes), transcript=transcript, multiopen=k) for c, k in zip(circuits, kinds)]
        self.g2 = (g2b(setup.s_g2), g2b(setup.g2))
        self.arg = [self.circuit_arg(vk, c) for vk, c in zip(self.vks, circuits)]

    def circuit_arg(self, vk, c):
        proofs = [([b"".join(fe(v) for v in col) for col in inst[0]], data) for inst, data in c.proofs]
        return (vk, c.name, self.table, proofs)

    def each(self, arg=None):
        return self.ver.verify_proofs(self.eng, arg or self.arg, *self.g2)

    def aggregate(self, arg=None):
        return self.ver.verify_aggregation(self.eng, arg or self.arg, *self.g2)

    def close(self):
        for vk in self.vks:
            vk.close()
        self.eng.bases_free(self.table)


@pytest.fixture(scope="module")
def toy():
    """a Shplonk proof of each of the three shapes and the restatement's pair for each: built once, left unchanged"""
    setup, circuits = TS.make_batch(0x5B1, SHAPES, 1)
    return setup, circuits, pair_bytes(SV.verify_each(TH.CrefEccChip, circuits))


def test_trapdoor_proofs_from_bytes(eng, ver, backend, toy):
    setup, circuits, want = toy
    prod = Product(eng, ver, setup, circuits)
    try:
        got = prod.each()
    finally:
        prod.close()
    assert [r[2] for r in got] == [0, 0, 0] and [r[3] for r in got] == [True] * 3
    assert [r[0] + r[1] for r in got] == want


@pytest.mark.parametrize("kind", ["sha256", "keccak256"])
def test_trapdoor_proofs_of_a_hash_transcript(eng, ver, kind):
    setup, circuits = TS.make_batch(0x5B2, [SHAPES[0]], 2, kind=kind)
    want = pair_bytes(SV.verify_each(TH.CrefEccChip, circuits, make_transcript=H.READERS[kind]))
    prod = Product(eng, ver, setup, circuits, transcript=kind)
    try:
        got = prod.each()
    finally:
        prod.close()
    assert [(r[2], r[3]) for r in got] == [(0, True)] * 2
    assert [r[0] + r[1] for r in got] == want


# ---------------------------------------------------------------------------------------------- honest proofs
@pytest.fixture(scope="module")
def world():
    class World:
        setups = {k: HP.Setup(k, TAU, HP.INSTANCE_ROWS) for k in (5, 6, BIG[0])}
        circuits = {(k, d): HP.make_circuit(random.Random(0xD00 + 16 * k + d), k, d) for k, d in HONEST_SHAPES + [BIG]}
        memo, python, pairs = {}, {}, {}
    w = World()
    for shape in HONEST_SHAPES:
        setup = w.setups[shape[0]]
        w.python[shape] = HS.prove_shplonk(w.circuits[shape], setup, HS.PyStagesShplonk(setup, w.memo), random.Random(1))
        w.pairs[shape] = restatement_pair(setup, w.python[shape])
    return w


def restatement_pair(setup, proof, name="honest"):
    return pair_bytes(SV.verify_each(TH.CrefEccChip, [HP.circuit_proofs(name, setup, [proof])]))[0]


def device_prove(pkg, eng, poly, ver, setup, circuit, seed=1):
    stages = HS.DeviceStagesShplonk(pkg, eng, poly, ver, setup)
    try:
        return HS.prove_shplonk(circuit, setup, stages, random.Random(seed))
    finally:
        stages.close()


class HonestProduct:
    """tests/test_gpu_honest_proofs.py::Product with Shplonk keys: one key per group of proofs, one table per k"""

    def __init__(self, eng, ver, setups, groups):
        self.eng, self.ver, self.tables, self.vks, self.arg = eng, ver, {}, [], []
        for gi, proofs in enumerate(groups):
            k = proofs[0].cs.k
            setup = setups[k]
            if k not in self.tables:
                self.tables[k] = eng.bases_upload(b"".join(O.aff_to_bytes(p) for p in setup.g_lagrange))
            vk = ver.VerifyingKey(eng, ver.encode_vk(proofs[0].cs, O.aff_to_bytes), multiopen="shplonk")
            self.vks.append(vk)
            rows = [([b"".join(fe(v) for v in col) for col in p.instances[0]], p.data) for p in proofs]
            self.arg.append((vk, "honest" if len(groups) == 1 else "honest%d" % gi, self.tables[k], rows))
        self.g2 = (g2b(setup.s_g2), g2b(setup.g2))

    def verdicts(self):
        """-> ([(left + right, status, verdict) per proof], the aggregation's verdict)"""
        try:
            each = [(r[0] + r[1], r[2], r[3]) for r in self.ver.verify_proofs(self.eng, self.arg, *self.g2)]
            return each, self.ver.verify_aggregation(self.eng, self.arg, *self.g2)[3]
        finally:
            for vk in self.vks:
                vk.close()
            for table in self.tables.values():
                self.eng.bases_free(table)


@pytest.mark.parametrize("shape", HONEST_SHAPES)
def test_the_device_proof_is_the_python_proof_and_is_accepted(pkg, eng, poly, ver, world, backend, shape):
    setup, want = world.setups[shape[0]], world.python[shape]
    got = device_prove(pkg, eng, poly, ver, setup, world.circuits[shape])
    assert HP.first_difference(got, want) is None, "first differing field: %s" % HP.first_difference(got, want)
    assert got.data == want.data
    each, agg = HonestProduct(eng, ver, world.setups, [[got]]).verdicts()
    assert each == [(world.pairs[shape], 0, True)], "status 0, verdict True, the restatement's (left, right) bit for bit"
    assert agg is True


def test_a_proof_at_sizes_beyond_one_workgroup(pkg, eng, poly, ver, world):
    proof = device_prove(pkg, eng, poly, ver, world.setups[BIG[0]], world.circuits[BIG])
    each, agg = HonestProduct(eng, ver, world.setups, [[proof]]).verdicts()
    assert [(s, ok) for _pair, s, ok in each] == [(0, True)] and agg is True


def test_an_honest_a_broken_and_an_honest_proof(pkg, eng, poly, ver, world):
    shape = (5, 4)
    setup, c = world.setups[5], world.circuits[shape]
    honest = device_prove(pkg, eng, poly, ver, setup, c)
    broken = device_prove(pkg, eng, poly, ver, setup, HP.broken_gate_cell(c))
    other = device_prove(pkg, eng, poly, ver, setup, c, seed=2)
    assert honest.data == world.python[shape].data and other.data != honest.data
    each, agg = HonestProduct(eng, ver, world.setups, [[honest, broken, other]]).verdicts()
    assert [s for _p, s, _ok in each] == [0, 0, 0]
    assert [ok for _p, _s, ok in each] == [True, False, True]
    assert each[0][0] == world.pairs[shape] and each[1][0] == restatement_pair(setup, broken)
    assert agg is False


# ---------------------------------------------------------------------------------------------- kinds
def gwc_circuit(rng, setup, dlogs, name, shape, nproofs, cs=None):
    cs = cs or T.make_constraint_system(rng, dlogs=dlogs, **shape)
    c = V.CircuitProofs(name, cs, setup.g_lagrange)
    for i in range(nproofs):
        instances = [[[rng.fr() for _ in range(3 + col)] for col in range(cs.num_instance_columns)]]
        c.proofs.append((instances, T.prove(cs, setup, rng, instances, dlogs, "%s_p%d" % (name, i))))
    return c


def shplonk_circuit(rng, setup, dlogs, name, shape, nproofs, cs=None):
    cs = cs or T.make_constraint_system(rng, dlogs=dlogs, **shape)
    c = V.CircuitProofs(name, cs, setup.g_lagrange)
    for i in range(nproofs):
        instances = [[[rng.fr() for _ in range(3 + col)] for col in range(cs.num_instance_columns)]]
        c.proofs.append((instances, TS.prove(cs, setup, rng, instances, dlogs, "%s_p%d" % (name, i))))
    return c


@pytest.fixture(scope="module")
def mixed():
    """one setup; a GWC circuit and a Shplonk circuit of different shapes, and a GWC and a Shplonk proof of ONE circuit"""
    class Mixed:
        rng = O.SplitMix64(0x5B3)
        dlogs = {}
    m = Mixed()
    m.setup = T.Setup(5, m.rng.fr(), 16)
    m.gwc = gwc_circuit(m.rng, m.setup, m.dlogs, "circuit0", SHAPES[0], 2)
    m.shp = shplonk_circuit(m.rng, m.setup, m.dlogs, "circuit1", SHAPES[1], 2)
    m.same_gwc = gwc_circuit(m.rng, m.setup, m.dlogs, "circuit2", SHAPES[0], 1)
    m.same_shp = shplonk_circuit(m.rng, m.setup, m.dlogs, "circuit2", SHAPES[0], 1, cs=m.same_gwc.cs)
    return m


def test_one_call_holds_a_gwc_and_a_shplonk_circuit(eng, ver, backend, mixed):
    circuits, kinds = [mixed.gwc, mixed.shp], ["gwc", "shplonk"]
    want = oracle_pairs([mixed.gwc], chip=TH.CrefEccChip) + pair_bytes(SV.verify_each(TH.CrefEccChip, [mixed.shp]))
    assert want == pair_bytes(SV.verify_each(TH.CrefEccChip, circuits, kinds))
    want_l, want_r, want_lam = SV.verify_aggregation(TH.CrefEccChip(), circuits, kinds)
    prod = Product(eng, ver, mixed.setup, circuits, kinds)
    try:
        got = prod.each()
        left, right, lam, ok = prod.aggregate()
    finally:
        prod.close()
    assert [r[0] + r[1] for r in got] == want, "each pair equals its own oracle"
    assert [(r[2], r[3]) for r in got] == [(0, True)] * 4
    assert left + right == S.final_pair_bytes(want_l, want_r) and lam == fe(want_lam) and ok is True


def test_a_proof_of_the_other_kind_does_not_fit_the_key(eng, ver, pkg, mixed):
    g_inst, g_data = mixed.same_gwc.proofs[0]
    s_inst, s_data = mixed.same_shp.proofs[0]
    assert len(g_data) != len(s_data)
    both = V.CircuitProofs("circuit2", mixed.same_gwc.cs, mixed.setup.g_lagrange, [(s_inst, s_data), (g_inst, g_data)])
    # (a pair does not depend on its proof's place in the call: the place only names the keys)
    want = {"shplonk": pair_bytes(SV.verify_each(TH.CrefEccChip, [mixed.same_shp]))[0],
            "gwc": oracle_pairs([mixed.same_gwc], chip=TH.CrefEccChip)[0]}
    for kind in ("shplonk", "gwc"):
        prod = Product(eng, ver, mixed.setup, [both], [kind])
        try:
            got = prod.each()
        finally:
            prod.close()
        fits, other = (0, 1) if kind == "shplonk" else (1, 0)
        assert got[other][2] == pkg.ERR_INVALID and got[other][3] is False, kind
        assert (got[fits][2], got[fits][3]) == (0, True), "the other proof of the call is still verified"
        assert got[fits][0] + got[fits][1] == want[kind]


# ---------------------------------------------------------------------------------------------- aggregation
@pytest.mark.parametrize("what", ["two proofs", "two circuits"])
def test_aggregations_match_the_restatement(eng, ver, backend, what):
    setup, circuits = TS.make_batch(0x5B4, [SHAPES[0]] if what == "two proofs" else [SHAPES[2], SHAPES[1]], 2 if what == "two proofs" else 1)
    want_l, want_r, want_lam = SV.verify_aggregation(TH.CrefEccChip(), circuits)
    prod = Product(eng, ver, setup, circuits)
    try:
        left, right, lam, ok = prod.aggregate()
    finally:
        prod.close()
    assert left + right == S.final_pair_bytes(want_l, want_r) and lam == fe(want_lam) and ok is True


def test_a_second_call_of_the_same_shape_hits_the_plan_cache(eng, ver):
    dlogs = {}
    setup, first = TS.make_batch(0x5B5, [SHAPES[0]], 2, dlogs=dlogs)
    rng = O.SplitMix64(0x5B6)
    second = [shplonk_circuit(rng, setup, dlogs, "circuit0", None, 2, cs=first[0].cs)]
    want = [SV.verify_aggregation(TH.CrefEccChip(), cs) for cs in (first, second)]
    prod = Product(eng, ver, setup, first)
    try:
        arg2 = [prod.circuit_arg(prod.vks[0], second[0])]
        h0, m0, _k = eng.verify_plan_stats()
        got1 = prod.aggregate()
        h1, m1, _k = eng.verify_plan_stats()
        got2 = prod.aggregate(arg2)
        h2, m2, _k = eng.verify_plan_stats()
        eng.debug_configure("plan_cache", 0)
        fresh2 = prod.aggregate(arg2)
    finally:
        eng.debug_configure("plan_cache", 1)
        prod.close()
    assert (h1 - h0, m1 - m0) == (0, 1) and (h2 - h1, m2 - m1) == (1, 0), "recorded once, then refilled"
    for got, (wl, wr, wlam) in ((got1, want[0]), (got2, want[1])):
        assert got[0] + got[1] == S.final_pair_bytes(wl, wr) and got[2] == fe(wlam) and got[3] is True
    assert fresh2 == got2 and got2[:3] != got1[:3]


def two_rotation_circuits(seed):
    """a circuit whose queries name two rotations only: its GWC proofs end in two W points and are as long as its Shplonk
    proofs.  -> (setup, the circuit with two Shplonk proofs, the same circuit with two GWC proofs)"""
    rng = O.SplitMix64(seed)
    dlogs = {}
    setup = T.Setup(5, rng.fr(), 16)
    cs = T.make_constraint_system(rng, dlogs=dlogs, k=5, n_advice=3, n_fixed=2, n_instance=1, n_gates=2, n_lookups=0, degree=4, n_perm_columns=2)
    assert cs.advice_queries[-1] == (0, -1) and (1, 1) not in cs.advice_queries
    cs.advice_queries[-1] = (1, 1)
    assert cs.num_permutation_sets == 1
    shp = shplonk_circuit(rng, setup, dlogs, "circuit0", None, 2, cs=cs)
    gwc = gwc_circuit(rng, setup, dlogs, "circuit0", None, 2, cs=cs)
    assert [len(d) for _i, d in shp.proofs] == [len(d) for _i, d in gwc.proofs]
    return setup, shp, gwc


def test_a_proof_of_the_other_kind_and_equal_length_is_rejected_by_verdict(eng, ver):
    """include/h2agg.h: where the lengths coincide the proof is read as the key's kind — status 0, verdict False"""
    setup, shp, gwc = two_rotation_circuits(0x5B8)
    for kind, wrong in (("shplonk", gwc), ("gwc", shp)):
        prod = Product(eng, ver, setup, [wrong], [kind])
        try:
            got = prod.each()
            agg = prod.aggregate()
        finally:
            prod.close()
        assert [(r[2], r[3]) for r in got] == [(0, False)] * 2, kind
        assert agg[3] is False, kind


def test_a_switched_key_records_afresh(eng, ver):
    """the two calls have one byte shape (two_rotation_circuits) and differ in the key's kind alone"""
    setup, shp, gwc = two_rotation_circuits(0x5B7)
    want_s = SV.verify_aggregation(TH.CrefEccChip(), [shp])
    want_g = SV.verify_aggregation(TH.CrefEccChip(), [gwc], ["gwc"])
    prod = Product(eng, ver, setup, [shp])
    try:
        _h0, m0, _k = eng.verify_plan_stats()
        got_s = prod.aggregate()
        prod.vks[0].set_multiopen("gwc")
        got_g = prod.aggregate([prod.circuit_arg(prod.vks[0], gwc)])
        _h1, m1, _k = eng.verify_plan_stats()
        prod.vks[0].set_multiopen("shplonk")
        again = prod.aggregate()
    finally:
        prod.close()
    assert m1 - m0 == 2, "the second call did not get the first one's recording back"
    for got, (wl, wr, wlam) in ((got_s, want_s), (got_g, want_g), (again, want_s)):
        assert got[0] + got[1] == S.final_pair_bytes(wl, wr) and got[2] == fe(wlam) and got[3] is True


def test_the_sharded_call_refuses_a_shplonk_key_before_any_exchange(eng, ver, pkg, toy):
    setup, circuits, _want = toy
    entered = []

    def allgather(payload):
        entered.append(len(payload))
        return [payload]
    prod = Product(eng, ver, setup, circuits[:1])
    try:
        with pytest.raises(pkg.H2AggError) as ei:
            ver.verify_aggregation_sharded(eng, prod.arg, [0], 1, 0, 1, allgather, *prod.g2)
        assert ei.value.code == pkg.ERR_INVALID and entered == []
    finally:
        prod.close()
