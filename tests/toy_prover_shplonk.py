"""The trapdoor prover of tests/toy_prover.py with a Shplonk tail.  Up to the challenge squeezed behind the evaluations the proof
is toy_prover's own (tests/toy_prover_hash.py::prove, which takes the transcript classes: the bytes before the W points do not
depend on them, so they are cut off); then y, v are the two squeezes, H1 is a FREE point, u is squeezed behind it, and
    H2 = f / (tau - u) * G,      f the discrete logarithm of F = right - u H2
solves the verifier equation tau * left = right in the exponent (DlogChip), as toy_prover solves for its W.  F comes from the
restatement (tests/shplonk_verifier_ref.py) with H2 = 0: a library that computes another F rejects these proofs.
Checker-side infrastructure."""
from __future__ import annotations

from oracle import bn254 as O
from oracle import poseidon as P
from oracle import schema as S
from oracle import verifier as V
from tests import shplonk_verifier_ref as SV
from tests import toy_prover_hash as TH
from tests.toy_prover import DlogChip, Setup, make_constraint_system

R = O.R


def encode_point(writer_cls, pt) -> bytes:
    w = writer_cls()
    w.write_point(pt)
    return bytes(w.finalize())


def prove(cs, setup, rng, instances, dlogs: dict, key: str, writer_cls=P.PoseidonTranscriptWrite,
          reader_cls=P.PoseidonTranscriptRead) -> bytes:
    """-> transcript bytes of ONE Shplonk proof that the verifier accepts"""
    gwc = TH.prove(cs, setup, rng, instances, dlogs, key, writer_cls, reader_cls)
    chip, ctx = S.OracleEccChip(), S.OracleCtx()
    _plain, commitments = V.assign_instance_commitment(TH.CrefEccChip(), ctx, instances, cs, setup.g_lagrange)
    n_w = len(V.build_params(reader_cls(gwc), chip, ctx, commitments, cs, key).w)
    body = gwc[:len(gwc) - n_w * SV.point_bytes(reader_cls)]
    rd = reader_cls(body)
    vp = V.build_params(rd, chip, ctx, commitments, cs, key)
    assert vp.w == [] and rd.pos == len(body)
    y, v = vp.v, vp.u                                              # two squeezes, nothing absorbed between them
    d1 = rng.fr()
    h1 = TH.g1_mul(d1)
    dlogs[h1] = d1
    rd.data = rd.data + encode_point(writer_cls, h1)
    assert rd.read_point() == h1
    u = rd.squeeze_challenge_scalar()
    proof = SV.shplonk_multi_open_proofs(key, V.queries(vp), None, h1, 0, y, v, u)      # H2 = 0 in the exponent: right = F
    f_s, f_e, _names = proof.w_g.eval(ctx, S.OracleFieldChip(), DlogChip(dlogs), 1)
    d2 = (f_s - (f_e or 0)) * O.inv((setup.tau - u) % R, R) % R
    h2 = TH.g1_mul(d2) if d2 else O.INF
    if h2 is not O.INF:
        dlogs[h2] = d2
    return body + encode_point(writer_cls, h1) + encode_point(writer_cls, h2)


def make_batch(seed, shapes, proofs_per_circuit, kind="poseidon", setup=None, dlogs=None, first_circuit=0):
    """tests/test_verifier_pipeline.py::make_batch with Shplonk proofs; kind: "poseidon" | "sha256" | "keccak256" """
    from tests import hash_transcript_ref as H
    wr, rdr = (P.PoseidonTranscriptWrite, P.PoseidonTranscriptRead) if kind == "poseidon" else (H.WRITERS[kind], H.READERS[kind])
    rng = O.SplitMix64(seed)
    dlogs = {} if dlogs is None else dlogs
    setup = setup or Setup(5, rng.fr(), 16)
    circuits = []
    for ci, shape in enumerate(shapes):
        cs = make_constraint_system(rng, dlogs=dlogs, **shape)
        c = V.CircuitProofs("circuit%d" % (first_circuit + ci), cs, setup.g_lagrange)
        for i in range(proofs_per_circuit):
            instances = [[[rng.fr() for _ in range(3 + col)] for col in range(cs.num_instance_columns)]]
            c.proofs.append((instances, prove(cs, setup, rng, instances, dlogs, "%s_p%d" % (c.name, i), wr, rdr)))
        circuits.append(c)
    return setup, circuits
