"""The trapdoor prover of tests/toy_prover.py for proofs written with ANOTHER transcript: `prove` takes the writer and reader
classes (tests/hash_transcript_ref.py: ShaTranscriptWrite / ShaTranscriptRead and their Keccak twins; oracle/poseidon.py's
pair works as well).  Setup, DlogChip and make_constraint_system are toy_prover's own, imported; the proving steps are the
same (commitments and evaluations are free scalars, the W points are solved for in the exponent with the known tau) — only the
bytes on the wire and the challenges differ.  Checker-side infrastructure, like toy_prover."""
from __future__ import annotations

from oracle import bn254 as O
from oracle import schema as S
from oracle import verifier as V
from tests.toy_prover import DlogChip, Setup, make_constraint_system  # noqa: F401  (re-exported for the tests)

R = O.R
_G = O.aff_to_bytes(O.G1)


def g1_mul(d: int):
    """d * G through the oracle's C restatement (oracle/cref.py: the same group law, ~500 x faster than oracle/bn254.py)"""
    from oracle import cref
    return O.aff_from_bytes(cref.g1_batch_to_affine(cref.g1_batch_scalar_mul(_G, O.fe_to_bytes(d % R), 1), 1))


class CrefEccChip(S.OracleEccChip):
    """MockEccChip with multi_exp and scalar_mul through oracle/cref.py (the reference algorithm in C)"""

    def scalar_mul(self, ctx, lhs, rhs):
        from oracle import cref
        if rhs is O.INF:
            return O.INF
        return O.aff_from_bytes(cref.g1_batch_to_affine(cref.g1_batch_scalar_mul(O.aff_to_bytes(rhs), O.fe_to_bytes(lhs % R), 1), 1))

    scalar_mul_constant = scalar_mul

    def multi_exp(self, ctx, points, scalars):
        from oracle import cref
        ctx.point_list = [O.debug_fmt(p) for p in points]
        n = len(points)
        return O.aff_from_bytes(cref.multi_exp_naive(b"".join(O.aff_to_bytes(p) for p in points),
                                                     b"".join(O.fe_to_bytes(s % R) for s in scalars), n))


def prove(cs, setup, rng, instances, dlogs: dict, key: str, writer_cls, reader_cls) -> bytes:
    """-> transcript bytes of ONE proof (instances: [inner proof][column][values]) accepted by the verifier"""
    w = writer_cls()

    def new_point():
        d = rng.fr()
        p = g1_mul(d)
        dlogs[p] = d
        return p
    w.common_scalar(cs.vk_scalar % R)
    inst_commitments = []
    for inst in instances:
        row = []
        for column in inst:
            d = sum(v * setup.lagrange_dlogs[i] for i, v in enumerate(column)) % R
            p = g1_mul(d) if column else O.INF
            if p is not O.INF:
                dlogs[p] = d
            row.append(p)
            w.common_point(p)
        inst_commitments.append(row)
    assert len(instances) == 1
    for phase in cs.phases():
        for ph in cs.advice_column_phase:
            if ph == phase:
                w.write_point(new_point())
        for ph in cs.challenge_phase:
            if ph == phase:
                w.squeeze_challenge_scalar()
    w.squeeze_challenge_scalar()                                   # theta
    for _ in cs.lookups:
        w.write_point(new_point())
        w.write_point(new_point())
    w.squeeze_challenge_scalar()                                   # beta
    w.squeeze_challenge_scalar()                                   # gamma
    for _ in range(cs.num_permutation_sets):
        w.write_point(new_point())
    for _ in cs.lookups:
        w.write_point(new_point())
    w.write_point(new_point())                                     # random commitment
    w.squeeze_challenge_scalar()                                   # y
    for _ in range(cs.quotient_poly_degree):
        w.write_point(new_point())
    w.squeeze_challenge_scalar()                                   # x
    n_evals = len(cs.instance_queries) + len(cs.advice_queries) + len(cs.fixed_queries) + 1 + \
        len(cs.permutation_commitments) + (3 * cs.num_permutation_sets - 1 if cs.num_permutation_sets else 0) + \
        5 * len(cs.lookups)
    for _ in range(n_evals):
        w.write_scalar(rng.fr())
    v = w.squeeze_challenge_scalar()
    rd = reader_cls(w.finalize())                                  # the verifier's own view so far (no W yet)
    vp = V.build_params(rd, S.OracleEccChip(), S.OracleCtx(), inst_commitments, cs, key)
    assert vp.v == v and vp.w == []
    chip = DlogChip(dlogs)
    groups = []                                                    # multiopen.rs:33-43: by rotation, first-seen order
    for rot, pt, s in V.queries(vp):
        for g in groups:
            if g[0] == rot:
                g[2].append(s)
                break
        else:
            groups.append([rot, pt, [s]])
    for _rot, z, schemas in groups:
        a, vk = 0, 1
        for s in schemas:                                          # sum_k v^k q_k (multiopen.rs:56-60)
            c = e = 0
            for name, pt_, sc in s.eval_prepare(S.OracleCtx(), S.OracleFieldChip(), 1, None):
                if name == "":
                    e = (e + sc) % R
                else:
                    c = (c + chip._d(pt_) * (1 if sc is None else sc)) % R
            a = (a + vk * (c - e)) % R
            vk = vk * v % R
        wd = a * O.inv((setup.tau - z) % R, R) % R
        p = g1_mul(wd)
        dlogs[p] = wd
        w.write_point(p)
    return w.finalize()


def make_batch(seed, shapes, proofs_per_circuit, kind, setup=None, dlogs=None):
    """tests/test_verifier_pipeline.py::make_batch with the proofs written by transcript `kind` ("sha256" | "keccak256")"""
    from tests import hash_transcript_ref as H
    rng = O.SplitMix64(seed)
    dlogs = {} if dlogs is None else dlogs
    circuits = []
    setup = setup or Setup(5, rng.fr(), 16)
    for ci, shape in enumerate(shapes):
        cs = make_constraint_system(rng, dlogs=dlogs, **shape)
        c = V.CircuitProofs("circuit%d" % ci, cs, setup.g_lagrange)
        for i in range(proofs_per_circuit):
            instances = [[[rng.fr() for _ in range(3 + col)] for col in range(cs.num_instance_columns)]]
            c.proofs.append((instances, prove(cs, setup, rng, instances, dlogs, "%s_p%d" % (c.name, i),
                                              H.WRITERS[kind], H.READERS[kind])))
        circuits.append(c)
    return setup, circuits


def oracle_pair(c, i, kind, fast=False):
    """verify_single_proof_in_chip for proof i of circuit c -> (left, right); fast: the group operations through oracle/cref"""
    from tests import hash_transcript_ref as H
    inst, data = c.proofs[i]
    pchip, ctx = (CrefEccChip() if fast else S.OracleEccChip()), S.OracleCtx()
    _plain, commitments = V.assign_instance_commitment(pchip, ctx, inst, c.cs, c.g_lagrange)
    proof, _adv, _vp = V.verify_single_proof_no_eval(H.READERS[kind](data), pchip, ctx, commitments, c.cs, "%s_p%d" % (c.name, i))
    left, right, _names = S.evaluate_multiopen_proof(ctx, S.OracleFieldChip(), pchip, proof)
    return left, right
