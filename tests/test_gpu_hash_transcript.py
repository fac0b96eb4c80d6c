"""GPU: the ShaRead transcript family (transcript/sha.rs) on the device and through the verifier.

  * h2agg_hash_transcript_read_batch: device backend == host backend == the reference reader (tests/hash_transcript_ref.py),
    both digests, at 1 / 3 / 64 / 65 / 1000 proofs (one, a partial wave, a full interleaving group, one past it, many groups).
    At 1000 proofs every proof is compared device against host (which tests/test_hash_transcript_host.py pins to the
    reference) and a sample — the group boundaries and the ends — against the pure-Python reference itself.
  * h2agg_verify_proofs with keys set to each digest over trapdoor proofs of two constraint-system shapes: pairs bit for bit
    equal to the oracle's, all verdicts true, a one-bit change named per proof, a Poseidon proof under a SHA key, one call
    mixing a Poseidon and a SHA-256 circuit, fs.verify_check over files, and the aggregation entry points' refusal.
The oracle's group operations go through oracle/cref (the same algorithms in C) to keep this file within its time budget."""
import importlib

import pytest

import __graft_entry__ as entry
from oracle import bn254 as O
from oracle import schema as S
from tests import hash_transcript_ref as H
from tests import toy_prover_hash as TH
from tests.test_hash_transcript_host import SCRIPTS, off_curve_point, reference
from tests.test_pairing_capi import g2b
from tests.test_verifier_pipeline import SHAPES

pytestmark = pytest.mark.gpu
KINDS = ["sha256", "keccak256"]


@pytest.fixture
def ver():
    return importlib.import_module(entry.PKG_NAME + ".verifier")


@pytest.fixture(scope="module")
def pool(eng):
    """256 curve points made on the device (k * G), as oracle tuples"""
    rng = O.SplitMix64(0x9001)
    n = 256
    ks = b"".join(O.fe_to_bytes(rng.fr()) for _ in range(n))
    aff = eng.g1_batch_to_affine(eng.g1_batch_scalar_mul(O.aff_to_bytes(O.G1) * n, ks))
    return [O.aff_from_bytes(aff[64 * i:64 * i + 64]) for i in range(n)]


def make_proofs(rng, pool, script, nproofs):
    consts = [rng.fr() for _ in range(script.count("C"))]
    proofs, exts = [], []
    for _ in range(nproofs):
        out = bytearray()
        for ch in script:
            if ch == "P":
                out += O.aff_to_bytes(pool[rng.next() % len(pool)])
            elif ch == "S":
                out += O.fe_to_bytes(rng.fr())
        proofs.append(bytes(out))
        exts.append([pool[rng.next() % len(pool)] for _ in range(script.count("X"))])
    return proofs, consts, exts


def both_backends(eng, kind, proofs, script, consts, exts):
    cb = b"".join(O.fe_to_bytes(c) for c in consts)
    xb = b"".join(O.aff_to_bytes(p) for x in exts for p in x)
    out = {}
    try:
        for backend in ("device", "host"):
            eng.transcript_configure(backend)
            out[backend] = eng.hash_transcript_read_batch(kind, proofs, script, cb, xb)
    finally:
        eng.transcript_configure("auto")
    return out["device"], out["host"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nproofs", [1, 3, 64, 65, 1000])
def test_read_batch_device_equals_host_equals_reference(eng, pool, kind, nproofs):
    rng = O.SplitMix64(0x7E0 + nproofs)
    scripts = SCRIPTS if nproofs <= 3 else ["CXQPQQSSQ", "PPPQSQPQ", "S" * 5 + "Q" + "P" * 12 + "Q"] if nproofs <= 65 else \
        ["CXPPQPQQPPPQSSSSSQPPPPQQ"]
    for script in scripts:
        proofs, consts, exts = make_proofs(rng, pool, script, nproofs)
        dev, host = both_backends(eng, kind, proofs, script, consts, exts)
        assert dev == host, script
        sample = range(nproofs) if nproofs <= 65 else [0, 1, 63, 64, 127, 128, 500, 959, 960, 999]
        want_pts, want_chal, _ = reference(kind, script, [proofs[i] for i in sample], consts, [exts[i] for i in sample])
        assert [dev[0][i] for i in sample] == want_pts, script
        assert [dev[1][i] for i in sample] == want_chal, script


@pytest.mark.parametrize("kind", KINDS)
def test_read_batch_errors(eng, pkg, pool, kind):
    rng = O.SplitMix64(0xBAD)
    script = "CPSQPQ"
    proofs, consts, exts = make_proofs(rng, pool, script, 65)
    cb = O.fe_to_bytes(consts[0])

    def with_bytes(k, off, b):
        ps = list(proofs)
        bad = bytearray(ps[k])
        bad[off:off + len(b)] = b
        ps[k] = bytes(bad)
        return ps
    try:
        for backend in ("device", "host"):
            eng.transcript_configure(backend)
            for ps in (with_bytes(40, 96, off_curve_point()), with_bytes(64, 0, O.P.to_bytes(32, "little")),
                       with_bytes(3, 0, bytes(64))):
                with pytest.raises(pkg.BadPoint):
                    eng.hash_transcript_read_batch(kind, ps, script, cb)
            with pytest.raises(pkg.H2AggError) as ei:
                eng.hash_transcript_read_batch(kind, with_bytes(40, 64, O.R.to_bytes(32, "little")), script, cb)
            assert ei.value.code == pkg.ERR_NONCANONICAL
            with pytest.raises(pkg.BadPoint):          # an identity external point
                eng.hash_transcript_read_batch(kind, [proofs[0][:64]], "XPQ", b"", bytes(64))
            assert eng.hash_transcript_read_batch(kind, proofs, script, cb)[0] == [p[:64] + p[96:] for p in proofs]
    finally:
        eng.transcript_configure("auto")
    with pytest.raises(pkg.H2AggError) as ei:
        eng.hash_transcript_read_batch(0, proofs, script, cb)
    assert ei.value.code == pkg.ERR_INVALID
    import ctypes as C
    out = C.create_string_buffer(4096)
    assert eng._lib.h2agg_hash_transcript_read_batch(eng._ctx, pkg.TRANSCRIPT_KINDS[kind], proofs[0], 32, 1, b"PQ", 2, None, 0,
                                                     None, 0, out, out) == pkg.ERR_INVALID


# ---- the verifier --------------------------------------------------------------------------------------------------------
class Product:
    """the product's view of a batch: keys (one transcript kind per circuit), one g_lagrange table, the circuits argument"""

    def __init__(self, eng, ver, setup, circuits, kinds):
        self.eng, self.ver = eng, ver
        self.table = eng.bases_upload(b"".join(O.aff_to_bytes(p) for p in setup.g_lagrange))
        self.vks = [ver.VerifyingKey(eng, ver.encode_vk(c.cs, O.aff_to_bytes), transcript=k) for c, k in zip(circuits, kinds)]
        self.g2 = (g2b(setup.s_g2), g2b(setup.g2))
        self.arg = []
        for vk, c in zip(self.vks, circuits):
            proofs = [([b"".join(O.fe_to_bytes(v) for v in col) for col in inst[0]], data) for inst, data in c.proofs]
            self.arg.append((vk, c.name, self.table, proofs))

    def each(self, arg=None):
        return self.ver.verify_proofs(self.eng, arg or self.arg, *self.g2)

    def close(self):
        for vk in self.vks:
            vk.close()
        self.eng.bases_free(self.table)


@pytest.fixture(scope="module")
def batches():
    """per digest: two shapes x two proofs, one setup for all (and the dlogs the trapdoor prover keeps)"""
    out, setup, dlogs = {}, None, {}
    for k, kind in enumerate(KINDS):
        setup, circuits = TH.make_batch(0x5A0 + k, [SHAPES[0], SHAPES[1]], 2, kind, setup=setup, dlogs=dlogs)
        want = [S.final_pair_bytes(*TH.oracle_pair(c, i, kind, fast=True)) for c in circuits for i in range(len(c.proofs))]
        out[kind] = (setup, circuits, want)
    return out


@pytest.fixture(params=["device", "host"])
def backend(request, eng):
    eng.transcript_configure(request.param)
    yield request.param
    eng.transcript_configure("auto")


@pytest.mark.parametrize("kind", KINDS)
def test_verify_proofs_matches_the_oracle(eng, ver, batches, backend, kind):
    setup, circuits, want = batches[kind]
    prod = Product(eng, ver, setup, circuits, [kind] * len(circuits))
    try:
        got = prod.each()
        commits = ver.verify_proofs(eng, prod.arg, with_commits=True)
    finally:
        prod.close()
    assert [r[0] + r[1] for r in got] == want
    assert [r[2] for r in got] == [0] * len(got)
    assert [r[3] for r in got] == [True] * len(got)
    # advice_out: the proof's first num_advice points, column order restored
    for rec, (c, i) in zip(commits, [(c, i) for c in circuits for i in range(len(c.proofs))]):
        _proof, adv, _vp = _no_eval(c, i, kind)
        assert rec[4] == [O.aff_to_bytes(p) for p in adv]


def _no_eval(c, i, kind):
    from oracle import verifier as V
    inst, data = c.proofs[i]
    pchip, ctx = TH.CrefEccChip(), S.OracleCtx()
    _plain, commitments = V.assign_instance_commitment(pchip, ctx, inst, c.cs, c.g_lagrange)
    return V.verify_single_proof_no_eval(H.READERS[kind](data), pchip, ctx, commitments, c.cs, "%s_p%d" % (c.name, i))


@pytest.mark.parametrize("kind", KINDS)
def test_one_bit_changes_are_named_per_proof(eng, pkg, ver, batches, kind):
    setup, circuits, want = batches[kind]
    prod = Product(eng, ver, setup, circuits, [kind] * len(circuits))
    vk, name, table, proofs = prod.arg[0]

    def with_proof(k, data):
        ps = list(proofs)
        ps[k] = (ps[k][0], data)
        return [(vk, name, table, ps)] + prod.arg[1:]

    def others_pass(got, k):
        for i, rec in enumerate(got):
            if i != k:
                assert rec[0] + rec[1] == want[i] and rec[2] == 0 and rec[3] is True, i

    def flipped(data, off, bit=1):
        b = bytearray(data)
        b[off] ^= bit
        return bytes(b)
    try:
        data = proofs[1][1]
        last_eval = len(data) - 64 * 4 - 32        # four W points close the transcript; the last evaluation before them
        # a bit of a scalar (still canonical): that proof's pairing fails
        got = prod.each(with_proof(1, flipped(data, last_eval)))
        assert got[1][2] == 0 and got[1][3] is False
        others_pass(got, 1)
        # a bit of a point's coordinate: the point leaves the curve — the documented status
        got = prod.each(with_proof(1, flipped(data, 5)))
        assert got[1][2] == pkg.ERR_BAD_POINT and got[1][3] is False
        others_pass(got, 1)
        # a scalar >= r
        b = bytearray(data)
        b[last_eval:last_eval + 32] = O.R.to_bytes(32, "little")
        got = prod.each(with_proof(0, bytes(b)))
        assert got[0][2] == pkg.ERR_NONCANONICAL and got[0][3] is False
        others_pass(got, 0)
        # one W point too many for the key's rotation groups
        got = prod.each(with_proof(1, data + data[-64:]))
        assert got[1][2] == pkg.ERR_INVALID and got[1][3] is False
        others_pass(got, 1)
        # a changed instance value
        cols = [bytearray(col) for col in proofs[0][0]]
        cols[0][0] ^= 1
        ps = list(proofs)
        ps[0] = ([bytes(col) for col in cols], ps[0][1])
        got = prod.each([(vk, name, table, ps)] + prod.arg[1:])
        assert got[0][2] == 0 and got[0][3] is False
        others_pass(got, 0)
    finally:
        prod.close()


def test_poseidon_and_sha_circuits_in_one_call(eng, pkg, ver, batches):
    setup, circuits, want = batches["sha256"]
    rng = O.SplitMix64(0x9051)
    from oracle import verifier as V
    from tests import toy_prover as T
    dlogs = {}
    cs = T.make_constraint_system(rng, dlogs=dlogs, **SHAPES[0])
    pc = V.CircuitProofs("poseidon0", cs, setup.g_lagrange)
    for i in range(2):
        instances = [[[rng.fr() for _ in range(3 + col)] for col in range(cs.num_instance_columns)]]
        pc.proofs.append((instances, T.prove(cs, setup, rng, instances, dlogs, "%s_p%d" % (pc.name, i))))
    sha = circuits[0]
    prod = Product(eng, ver, setup, [pc, sha], ["poseidon", "sha256"])
    sha_only_key = ver.VerifyingKey(eng, ver.encode_vk(pc.cs, O.aff_to_bytes), transcript="sha256")
    try:
        mixed = prod.each()
        apart = prod.each(prod.arg[:1]) + prod.each(prod.arg[1:])
        assert mixed == apart
        assert [r[2] for r in mixed] == [0] * 4 and [r[3] for r in mixed] == [True] * 4
        assert [r[0] + r[1] for r in mixed[2:]] == want[:2]
        # a Poseidon-written proof under a SHA key: it does not fit the key
        got = prod.each([(sha_only_key, "poseidon0", prod.table, prod.arg[0][3])])
        assert [r[2] for r in got] == [pkg.ERR_INVALID] * 2 and [r[3] for r in got] == [False] * 2
        # the aggregation entry points refuse a key whose kind is not Poseidon, before any work
        for arg in (prod.arg, prod.arg[1:]):
            with pytest.raises(pkg.H2AggError) as ei:
                ver.verify_aggregation(eng, arg, *prod.g2)
            assert ei.value.code == pkg.ERR_INVALID and "SHA-256" in str(ei.value)
        with pytest.raises(pkg.H2AggError) as ei:
            ver.verify_aggregation_sharded(eng, prod.arg[1:], [0, 1], 2, 0, 1, allgather=lambda b: [b])
        assert ei.value.code == pkg.ERR_INVALID
        assert ver.verify_aggregation(eng, prod.arg[:1], *prod.g2)[3] is True
    finally:
        sha_only_key.close()
        prod.close()
    with pytest.raises(ValueError):
        ver.VerifyingKey(eng, ver.encode_vk(pc.cs, O.aff_to_bytes), transcript="blake2b")


@pytest.mark.parametrize("kind", KINDS)
def test_fs_verify_check(eng, ver, batches, tmp_path, kind):
    fs = importlib.import_module(entry.PKG_NAME + ".fs")
    setup, circuits, _want = batches[kind]
    c = circuits[0]                                  # one instance column, as verify_circuit_instance.data holds
    inst, data = c.proofs[0]
    assert len(inst[0]) == 1
    fs.write_verify_circuit_instance(str(tmp_path), [O.fe_to_bytes(v) for v in inst[0][0]])
    (tmp_path / "verify_circuit_proof.data").write_bytes(data)
    assert fs.load_verify_circuit_proof(str(tmp_path)) == data
    table = eng.bases_upload(b"".join(O.aff_to_bytes(p) for p in setup.g_lagrange))
    vk = ver.VerifyingKey(eng, ver.encode_vk(c.cs, O.aff_to_bytes), transcript=kind)
    try:
        assert fs.verify_check(eng, str(tmp_path), vk, table, g2b(setup.s_g2), g2b(setup.g2), transcript=kind) is True
        bad = bytearray(data)
        bad[len(bad) - 64 * 4 - 1] ^= 1              # the last evaluation
        (tmp_path / "verify_circuit_proof.data").write_bytes(bytes(bad))
        assert fs.verify_check(eng, str(tmp_path), vk, table, g2b(setup.s_g2), g2b(setup.g2), transcript=kind) is False
        with pytest.raises(ValueError):
            fs.verify_check(eng, str(tmp_path), vk, table, g2b(setup.s_g2), g2b(setup.g2),
                            transcript="keccak256" if kind == "sha256" else "sha256")
    finally:
        vk.close()
        eng.bases_free(table)
