"""The honest prover of tests/honest_prover.py with a Shplonk tail: `prove_shplonk` over the same stages.

Up to the evaluations the proof is honest_prover.prove's own, byte for byte — that driver is run as it stands, over a proxy of
the stages that notes what it asks to be opened (the slab, the queries, the points) and answers with placeholder W points,
which are cut off again: the bytes before them do not depend on them.  Then the tail: y and v are the two squeezes behind the
evaluations, H1 is written, u squeezed, H2 written.  The openings come from one more stage, `open_shplonk`, with the two
backends of honest_prover:

  PyStagesShplonk      tests/shplonk_ref.py's Opening (the prover's definition in Python integers), commitments p(tau) * G
  DeviceStagesShplonk  poly.shplonk_prove (h2agg_kzg_shplonk_begin / _finish)

The two must agree byte for byte (tests/test_gpu_shplonk_verifier.py).  A polynomial is a column of the slab, i.e. one
commitment key of the verifier's queries, and the queries keep the order of oracle/verifier.py::queries, so prover and verifier
form the same sets.  Checker-side infrastructure."""
from __future__ import annotations

from oracle import bn254 as O
from oracle import poseidon as P
from oracle import schema as S
from oracle import verifier as V
from tests import honest_prover as HP
from tests import shplonk_ref as SR
from tests.fr_bytes import enc, fe

R = O.R


class PyStagesShplonk(HP.PyStages):
    def open_shplonk(self, polys, k, queries, points, y, v, squeeze_u):
        """-> (H1, H2); squeeze_u(H1) writes H1 and returns u"""
        op = SR.Opening(polys, points, queries, y, v)
        h1 = self._commit([op.h()])[0]
        u = squeeze_u(h1)
        q, rem = op.h2(u)
        assert rem == 0, "L(u) != 0"
        return h1, self._commit([q])[0]


class DeviceStagesShplonk(HP.DeviceStages):
    def open_shplonk(self, polys, k, queries, points, y, v, squeeze_u):
        _evals, h1, h2 = self.poly.shplonk_prove(self.eng, self.g, b"".join(self._cols(polys)), k, queries, enc(points), fe(y), fe(v),
                                                 lambda h1_aff: fe(squeeze_u(O.aff_from_bytes(h1_aff))))
        return O.aff_from_bytes(h1), O.aff_from_bytes(h2)


class _NoteTheOpening:
    """the stages as they are, but `open` notes its arguments and answers with placeholders (one point per rotation group)"""

    def __init__(self, stages):
        self._stages, self.opened = stages, None

    def __getattr__(self, name):
        return getattr(self._stages, name)

    def open(self, polys, k, queries, points, v):
        self.opened = (polys, k, queries, points)
        return [O.G1] * len(HP.group_queries(queries))


def encode_point(writer_cls, pt) -> bytes:
    w = writer_cls()
    w.write_point(pt)
    return bytes(w.finalize())


def prove_shplonk(circuit: HP.Circuit, setup, stages, rng, writer_cls=P.PoseidonTranscriptWrite, reader_cls=P.PoseidonTranscriptRead,
                  blinding=True, driver=None) -> HP.Proof:
    """one Shplonk proof of `circuit` by the stages of `stages` (a PyStagesShplonk or a DeviceStagesShplonk)"""
    note = _NoteTheOpening(stages)
    gwc = HP.prove(circuit, setup, note, rng, writer_cls=writer_cls, blinding=blinding, driver=driver)
    w_at = min(lo for name, lo, _hi in gwc.fields if name.startswith("W "))
    body = gwc.data[:w_at]
    fields = [f for f in gwc.fields if not f[0].startswith("W ")]
    polys, k, queries, points = note.opened
    # the transcript behind the evaluations, as a reader of the body leaves it: it squeezes twice and finds no W
    rd = reader_cls(body)
    inst = stages.commit_lagrange(circuit.lag["instance"], k)
    vp = V.build_params(rd, S.OracleEccChip(), S.OracleCtx(), [inst], gwc.cs, "")
    assert vp.w == [] and rd.pos == len(body)
    y, v = vp.v, vp.u
    tail = []

    def squeeze_u(h1):
        tail.append(encode_point(writer_cls, h1))
        rd.data = rd.data + tail[0]
        assert rd.read_point() == h1
        return rd.squeeze_challenge_scalar()
    _h1, h2 = stages.open_shplonk(polys, k, queries, points, y, v, squeeze_u)
    tail.append(encode_point(writer_cls, h2))
    at = len(body)
    fields += [("H1", at, at + len(tail[0])), ("H2", at + len(tail[0]), at + len(tail[0]) + len(tail[1]))]
    return HP.Proof(gwc.cs, circuit.instances, body + tail[0] + tail[1], fields)
