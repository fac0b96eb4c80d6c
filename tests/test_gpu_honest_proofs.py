"""GPU: honest proofs — the device's prover stages through the verifier.

tests/honest_prover.py's driver over DeviceStages (poly.py and the engine: params_setup, permutation_key / fixed_key,
commit_columns, expressions_eval, permute_expression_pair, the grand products, the Fr transform, quotient_pieces, fr_poly_eval,
multiopen_prove) writes a proof from a witness.  It must equal the proof the same driver writes over PyStages (the Python
restatements, which tests/test_honest_prover_host.py holds against the oracle's verifier) byte for byte, and the library's
from-bytes verifier must accept it with the oracle's pair; proofs of broken witnesses, made by the same device stages, must be
rejected with status 0 and a False verdict."""
import importlib
import random

import pytest

import __graft_entry__ as entry
from oracle import bn254 as O
from oracle import pairing as E
from tests import hash_transcript_ref as H
from tests import honest_prover as HP
from tests import toy_prover_hash as TH
from tests.grand_product_ref import R
from tests.test_gpu_verify_each import oracle_pairs
from tests.test_pairing_capi import g2b

pytestmark = pytest.mark.gpu

TAU = random.Random(0x7A0).randrange(1, R)
SHAPES = [(5, 4), (5, 5), (6, 6)]
# k = 12 is the smallest k at which EVERY row-scaled stage leaves its one-workgroup path: a column's transform takes two
# passes from k = 11 (csrc/fr_fft.inc: ceil(k / 10) launches; at k = 9 only the quotient's extended domain, k + 2 = 11, does),
# and usable + 1 = 4091 > 2^11 positions put the product scans (csrc/fr_chunk.hpp), the sort of permute_expression_pair
# (csrc/lookup_kernels.hpp) and the division's sweeps across two workgroups — which k = 11 (2043 positions) would not.
BIG = (12, 4)


@pytest.fixture(scope="module")
def poly(pkg):
    return importlib.import_module(entry.PKG_NAME + ".poly")


@pytest.fixture(scope="module")
def verifier(pkg):
    return importlib.import_module(entry.PKG_NAME + ".verifier")


@pytest.fixture(params=["device", "host"])
def backend(request, eng):
    """both sponge backends (h2agg_transcript_configure), as tests/test_gpu_verify_each.py runs them"""
    eng.transcript_configure(request.param)
    yield request.param
    eng.transcript_configure("auto")


@pytest.fixture(scope="module")
def world():
    """one tau, the circuits, and the PyStages proof of each small shape with the oracle's pair for it: built once, shared,
    left unchanged"""
    class World:
        setups = {k: HP.Setup(k, TAU, HP.INSTANCE_ROWS) for k in (5, 6, BIG[0])}
        circuits = {(k, d): HP.make_circuit(random.Random(0xD00 + 16 * k + d), k, d) for k, d in SHAPES + [BIG]}
        memo, python, pairs = {}, {}, {}
    w = World()
    for shape in SHAPES:
        setup = w.setups[shape[0]]
        w.python[shape] = HP.prove(w.circuits[shape], setup, HP.PyStages(setup, w.memo), random.Random(1))
        w.pairs[shape] = oracle_pair(setup, w.python[shape])
    return w


def oracle_pair(setup, proof, name="honest"):
    """verify_single_proof_in_chip of the oracle -> (left, right) as 128 bytes"""
    return oracle_pairs([HP.circuit_proofs(name, setup, [proof])], chip=TH.CrefEccChip)[0]


def device_prove(pkg, eng, poly, verifier, setup, circuit, seed=1, **kw):
    stages = HP.DeviceStages(pkg, eng, poly, verifier, setup)
    try:
        assert stages.s_g2() == g2b(setup.s_g2), "[tau]_2"
        return HP.prove(circuit, setup, stages, random.Random(seed), **kw)
    finally:
        stages.close()


class Product:
    """the library's view of some proofs: one key per group of proofs, one g_lagrange table per k (the points of the oracle's
    setup, uploaded), [tau]_2"""

    def __init__(self, eng, verifier, setups, groups, transcript="poseidon", instances=None):
        self.eng, self.verifier = eng, verifier
        self.tables, self.vks, self.arg = {}, [], []
        setup = None
        try:
            for gi, proofs in enumerate(groups):
                k = proofs[0].cs.k
                setup = setups[k]
                if k not in self.tables:
                    self.tables[k] = eng.bases_upload(b"".join(O.aff_to_bytes(p) for p in setup.g_lagrange))
                vk = verifier.VerifyingKey(eng, verifier.encode_vk(proofs[0].cs, O.aff_to_bytes), transcript=transcript)
                self.vks.append(vk)
                rows = []
                for i, p in enumerate(proofs):
                    inst = p.instances if instances is None else instances[gi][i]
                    rows.append(([b"".join(O.fe_to_bytes(v) for v in col) for col in inst[0]], p.data))
                self.arg.append((vk, "honest" if len(groups) == 1 else "honest%d" % gi, self.tables[k], rows))
        except Exception:
            self.close()
            raise
        self.g2 = (g2b(setup.s_g2), g2b(setup.g2))

    def each(self):
        return self.verifier.verify_proofs(self.eng, self.arg, *self.g2)

    def aggregate(self):
        return self.verifier.verify_aggregation(self.eng, self.arg, *self.g2)

    def close(self):
        for vk in self.vks:
            vk.close()
        for table in self.tables.values():
            self.eng.bases_free(table)
        self.vks, self.tables = [], {}


def verdicts(eng, verifier, setups, groups, **kw):
    """-> ([(left + right, status, verdict) per proof], the aggregation's verdict)"""
    prod = Product(eng, verifier, setups, groups, **kw)
    try:
        each = [(r[0] + r[1], r[2], r[3]) for r in prod.each()]
        agg = prod.aggregate()[3] if kw.get("transcript", "poseidon") == "poseidon" else None
    finally:
        prod.close()
    return each, agg


# ---------------------------------------------------------------------------------------------- acceptance
@pytest.mark.parametrize("shape", SHAPES)
def test_the_device_proof_is_the_python_proof_and_is_accepted(pkg, eng, poly, verifier, world, backend, shape):
    setup, want = world.setups[shape[0]], world.python[shape]
    got = device_prove(pkg, eng, poly, verifier, setup, world.circuits[shape])
    assert got.cs.vk_scalar == want.cs.vk_scalar and got.cs.fixed_commitments == want.cs.fixed_commitments and \
        got.cs.permutation_commitments == want.cs.permutation_commitments, "the key"
    assert HP.first_difference(got, want) is None, "first differing field: %s" % HP.first_difference(got, want)
    assert got.data == want.data
    each, agg = verdicts(eng, verifier, world.setups, [[got]])
    assert each == [(world.pairs[shape], 0, True)], "status 0, verdict True, the oracle's (left, right) bit for bit"
    assert agg is True


def test_a_proof_at_sizes_beyond_one_workgroup(pkg, eng, poly, verifier, world):
    """k = 12, degree 4 (see BIG above).  The Python quotient is no yardstick at this size: the assertion is acceptance, by the
    device verifier and by the oracle's pairing on the device's pair; the device verifier's parity with the oracle on this
    proof is the oracle's replay of the transcript (no prover in it, about a second)."""
    setup = world.setups[BIG[0]]
    proof = device_prove(pkg, eng, poly, verifier, setup, world.circuits[BIG])
    each, agg = verdicts(eng, verifier, world.setups, [[proof]])
    assert [(s, ok) for _pair, s, ok in each] == [(0, True)] and agg is True
    pair = each[0][0]
    left, right = O.aff_from_bytes(pair[:64]), O.aff_from_bytes(pair[64:])
    assert E.pairing_check([(left, setup.s_g2), (right, E.g2_neg(setup.g2))])
    assert pair == oracle_pair(setup, proof)


# ---------------------------------------------------------------------------------------------- batches
def test_an_honest_and_a_broken_proof_in_one_batch(pkg, eng, poly, verifier, world):
    shape = (5, 4)
    setup, c = world.setups[5], world.circuits[shape]
    honest = device_prove(pkg, eng, poly, verifier, setup, c)
    broken = device_prove(pkg, eng, poly, verifier, setup, HP.broken_gate_cell(c))
    other = device_prove(pkg, eng, poly, verifier, setup, c, seed=2)
    assert honest.data == world.python[shape].data and other.data != honest.data
    each, agg = verdicts(eng, verifier, world.setups, [[honest, broken, other]])
    assert [s for _p, s, _ok in each] == [0, 0, 0]
    assert [ok for _p, _s, ok in each] == [True, False, True]
    assert each[0][0] == world.pairs[shape]
    assert agg is False


def test_two_circuits_in_one_aggregation(pkg, eng, poly, verifier, world):
    proofs = [device_prove(pkg, eng, poly, verifier, world.setups[s[0]], world.circuits[s]) for s in ((5, 4), (6, 6))]
    each, agg = verdicts(eng, verifier, world.setups, [[proofs[0]], [proofs[1]]])
    assert [(s, ok) for _p, s, ok in each] == [(0, True), (0, True)]
    assert agg is True


# ---------------------------------------------------------------------------------------------- rejections
@pytest.mark.parametrize("what", ["gate cell", "copied cell"])
def test_a_broken_witness_proven_on_the_device_is_rejected(pkg, eng, poly, verifier, world, what):
    shape = (5, 4)
    c = world.circuits[shape]
    bad = HP.broken_gate_cell(c) if what == "gate cell" else HP.broken_copied_cell(c)
    proof = device_prove(pkg, eng, poly, verifier, world.setups[5], bad)
    assert proof.data != world.python[shape].data
    each, agg = verdicts(eng, verifier, world.setups, [[proof]])
    assert [(s, ok) for _p, s, ok in each] == [(0, False)]
    assert each[0][0] == oracle_pair(world.setups[5], proof), "rejected with the oracle's pair"
    assert agg is False


def test_a_wrong_instance_value_is_rejected(pkg, eng, poly, verifier, world):
    proof = device_prove(pkg, eng, poly, verifier, world.setups[5], world.circuits[(5, 4)])
    wrong = [[list(col) for col in inner] for inner in proof.instances]
    wrong[0][0][1] = (wrong[0][0][1] + 1) % R
    each, agg = verdicts(eng, verifier, world.setups, [[proof]], instances=[[wrong]])
    assert [(s, ok) for _p, s, ok in each] == [(0, False)] and agg is False


def test_an_input_outside_the_table_is_refused_and_the_context_goes_on(pkg, eng, poly, verifier, world):
    shape = (5, 4)
    setup, c = world.setups[5], world.circuits[shape]
    with pytest.raises(pkg.H2AggError) as ei:
        device_prove(pkg, eng, poly, verifier, setup, HP.outside_the_table(c))
    assert ei.value.code == pkg.ERR_NOT_IN_TABLE
    proof = device_prove(pkg, eng, poly, verifier, setup, c)
    assert proof.data == world.python[shape].data
    each, agg = verdicts(eng, verifier, world.setups, [[proof]])
    assert each == [(world.pairs[shape], 0, True)] and agg is True


# ---------------------------------------------------------------------------------------------- another transcript
def test_a_keccak_proof_is_accepted_and_its_tampered_twin_rejected(pkg, eng, poly, verifier, world):
    shape, kind = (5, 4), "keccak256"
    setup = world.setups[5]
    want = HP.prove(world.circuits[shape], setup, HP.PyStages(setup, world.memo), random.Random(1), writer_cls=H.WRITERS[kind])
    proof = device_prove(pkg, eng, poly, verifier, setup, world.circuits[shape], writer_cls=H.WRITERS[kind])
    assert HP.first_difference(proof, want) is None and proof.data == want.data
    assert proof.data != world.python[shape].data and len(proof.data) > len(world.python[shape].data), "points are 64 bytes here"
    mk = lambda data: H.READERS[kind](data)
    assert HP.oracle_accepts(setup, [HP.circuit_proofs("honest", setup, [proof])], make_transcript=mk)
    each, _agg = verdicts(eng, verifier, world.setups, [[proof]], transcript=kind)
    assert [(s, ok) for _p, s, ok in each] == [(0, True)]
    name, lo, _hi = [f for f in proof.fields if f[0] == "permuted table evaluation"][0]
    data = bytearray(proof.data)
    data[lo] ^= 1                                       # one bit of the last evaluation: still canonical
    twin = HP.Proof(proof.cs, proof.instances, bytes(data), proof.fields)
    each, _agg = verdicts(eng, verifier, world.setups, [[twin]], transcript=kind)
    assert [(s, ok) for _p, s, ok in each] == [(0, False)], name

