"""The Shplonk VERIFIER restated over oracle/: the definition of include/h2agg.h (h2agg_schema_shplonk_multi_open and the
Shplonk section) built from S.scalar, S.commit and the query schemas, the tail of a Shplonk proof (y, v, H1, u, H2) read
behind V.build_params, and the two drivers over S.evaluate_multiopen_proof.  tests/shplonk_ref.py restates the PROVER and the
verifier's scalars in the exponent; tests/test_shplonk_verifier_host.py ties the two, tests/test_gpu_shplonk_verifier.py holds
the library against this file bit for bit.

Every convention the definition fixes is one method of `Conventions`, so a test can misread one (the sensitivity table).
halo2_proofs' own set ordering and byte layout are recalled, not pinned: what is pinned is that prover and verifier follow the
one definition and that the pairing accepts.  Checker-side infrastructure."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, List

from oracle import bn254 as O
from oracle import poseidon as P
from oracle import schema as S
from oracle import verifier as V

R = O.R
MAX_SET = 32


def _inv(x: int) -> int:
    if x % R == 0:
        raise ZeroDivisionError("inversion of zero (the reference's invert().unwrap())")
    return pow(x % R, R - 2, R)


def _prod(xs) -> int:
    out = 1
    for x in xs:
        out = out * x % R
    return out


class Conventions:
    """what the definition fixes, one method each"""

    def poly_id(self, index: int, rotation: int, schema: S.Schema):
        """which polynomial a query opens: its commitment's key; the vanishing query (the h pieces folded with x^n, plus
        expected_h_eval) is a polynomial of its own"""
        if schema.kind == "add" and schema.l.kind == "commitment":
            return schema.l.cq.key
        return ("vanishing", index)

    def sets(self, poly_ids, rotations):
        """-> [(rotations of the set, in the order its first polynomial names them; its polynomials)]: polynomials with equal
        point sets, sets in first-seen order of their first polynomial, polynomials in first-seen order of their first query"""
        first_seen, named = [], {}
        for m, r in zip(poly_ids, rotations):
            if m not in named:
                first_seen.append(m)
                named[m] = []
            if r in named[m]:
                raise ValueError("a (polynomial, rotation) pair is named twice")
            named[m].append(r)
        out = []
        for m in first_seen:
            for pts, members in out:
                if set(pts) == set(named[m]):
                    members.append(m)
                    break
            else:
                out.append((named[m], [m]))
        return out

    def challenges(self, y: int, v: int):
        """(the challenge whose powers separate the polynomials of a set, the one whose powers separate the sets)"""
        return y, v

    def set_power(self, i: int, nsets: int) -> int:
        return i

    def poly_power(self, j: int, polys_before: int) -> int:
        """j: the polynomial's place in its set; polys_before: polynomials of the earlier sets"""
        return j

    def c(self, d: List[int], i: int) -> int:
        return d[i] * _inv(d[0]) % R

    def t(self, um_s0: List[int], um_all: List[int], d0: int) -> int:
        """prod_{b in S_0} (u - z_b) = Z_T(u) / d_0"""
        return _prod(um_s0)

    def weights(self, zs: List[int], u: int) -> List[int]:
        """l_{i,a}(u) over the set's points zs: the values at the points weighted so, the sum is r_{i,j}(u)"""
        out = []
        for a, za in enumerate(zs):
            num = _prod((u - zb) % R for b, zb in enumerate(zs) if b != a)
            den = _prod((za - zb) % R for b, zb in enumerate(zs) if b != a)
            out.append(num * _inv(den) % R if len(zs) > 1 else 1)
        return out

    def with_h2(self, right: S.Schema, u: int, h2: S.Schema) -> S.Schema:
        return right + S.scalar(u % R) * h2

    def read_tail(self, t, tail: bytes):
        """behind the evaluations and the squeezes y, v: H1 is read (and absorbed), then u squeezed, then H2 read"""
        t.data = t.data + tail
        h1 = t.read_point()
        u = t.squeeze_challenge_scalar()
        h2 = t.read_point()
        return h1, u, h2


def shplonk_multi_open_proofs(key: str, queries, poly_ids, h1, h2, y: int, v: int, u: int, conv: Conventions = None) -> S.MultiOpenProof:
    """queries: [(rotation, point, schema)] in VerifierParams::queries order; poly_ids: one per query, or None for
    conv.poly_id.  -> MultiOpenProof(left = commit(H2), right = F + u H2) for S.evaluate_multiopen_proof.
    ValueError: what the library refuses; ZeroDivisionError: what inverts zero on its tape."""
    conv = conv or Conventions()
    if not queries:
        raise ValueError("no queries")
    if poly_ids is None:
        poly_ids = [conv.poly_id(i, rot, s) for i, (rot, _pt, s) in enumerate(queries)]
    z, node = {}, {}
    for (rot, pt, s), m in zip(queries, poly_ids):
        z.setdefault(rot, pt % R)                       # a rotation names the point its first query carries
        node.setdefault((m, rot), s)
    sets = conv.sets(poly_ids, [q[0] for q in queries])
    if any(len(pts) > MAX_SET for pts, _m in sets):
        raise ValueError("a set of more than 32 points")
    T = list(z)
    for a in range(len(T)):
        for b in range(a + 1, len(T)):
            _inv(z[T[a]] - z[T[b]])                     # two rotations with equal points
    y, v = conv.challenges(y % R, v % R)
    um = {r: (u - z[r]) % R for r in T}
    d = [_prod(um[b] for b in T if b not in pts) for pts, _m in sets]
    right, before = None, 0
    for i, (pts, members) in enumerate(sets):
        w_i = pow(v, conv.set_power(i, len(sets)), R) * (conv.c(d, i) if len(sets) > 1 else 1) % R
        l = conv.weights([z[r] for r in pts], u % R)
        for j, m in enumerate(members):
            w = w_i * pow(y, conv.poly_power(j, before), R) % R
            for a, r in enumerate(pts):
                term = S.scalar(w * l[a] % R) * node[(m, r)]
                right = term if right is None else right + term
        before += len(members)
    t = conv.t([um[r] for r in sets[0][0]], [um[r] for r in T], d[0])
    right = right + S.scalar((0 - t) % R) * S.commit(S.CommitQuery("%s_shplonk_h1" % key, h1, None))
    right = conv.with_h2(right, u, S.commit(S.CommitQuery("%s_shplonk_h2" % key, h2, None)))
    # (left = 1 * H2: a bare commitment carries no scalar, and the reference's multi_exp panics on zero pairs)
    return S.MultiOpenProof(S.scalar(1) * S.commit(S.CommitQuery("%s_shplonk_h2" % key, h2, None)), right)


@dataclass
class Tail:
    y: int
    v: int
    h1: Any
    u: int
    h2: Any


def point_bytes(make_transcript) -> int:
    """bytes of a proof point under the reader `make_transcript` builds: 32 compressed (Poseidon), 64 under ShaRead"""
    return 32 if isinstance(make_transcript(b""), P.PoseidonTranscriptRead) else 64


def build_params_shplonk(data: bytes, pchip, ctx, assigned_instances, cs, key: str, make_transcript=None, conv: Conventions = None):
    """V.build_params on the transcript without its last two points — behind the evaluations it squeezes twice and finds no W:
    the Shplonk proof's y and v — then the tail read by itself.  -> (reader, VerifierParams, Tail)"""
    conv = conv or Conventions()
    mk = make_transcript or (lambda b: P.PoseidonTranscriptRead(b))
    cut = len(data) - 2 * point_bytes(mk)
    t = mk(data[:cut])
    vp = V.build_params(t, pchip, ctx, assigned_instances, cs, key)
    if vp.w or t.pos != cut:
        raise ValueError("the proof does not end in exactly two points behind its evaluations")
    h1, u, h2 = conv.read_tail(t, data[cut:])
    return t, vp, Tail(vp.v, vp.u, h1, u, h2)


def verify_single_proof_no_eval(t_data, pchip, ctx, assigned_instances, cs, key, make_transcript=None, conv=None):
    """-> (reader, MultiOpenProof) of one Shplonk proof"""
    t, vp, tail = build_params_shplonk(t_data, pchip, ctx, assigned_instances, cs, key, make_transcript, conv)
    return t, shplonk_multi_open_proofs(vp.key, V.queries(vp), None, tail.h1, tail.h2, tail.y, tail.v, tail.u, conv)


def _proofs_of(pchip, ctx, circuit: V.CircuitProofs, kind: str, make_transcript, conv):
    """-> [(reader behind the proof, MultiOpenProof)] of a circuit's proofs; kind: "shplonk" | "gwc" """
    mk = make_transcript or (lambda b: P.PoseidonTranscriptRead(b))
    out = []
    for i, (instances, data) in enumerate(circuit.proofs):
        _plain, commitments = V.assign_instance_commitment(pchip, ctx, instances, circuit.cs, circuit.g_lagrange)
        key = "%s_p%d" % (circuit.name, i)                                             # verify_circuit.rs:140
        if kind == "shplonk":
            out.append(verify_single_proof_no_eval(data, pchip, ctx, commitments, circuit.cs, key, mk, conv))
        else:
            t = mk(data)
            out.append((t, V.verify_single_proof_no_eval(t, pchip, ctx, commitments, circuit.cs, key)[0]))
    return out


def verify_each(pchip_cls, circuits, kinds=None, make_transcript=None, conv=None):
    """every proof on its own (verify_single_proof_in_chip) -> [(left, right)]; kinds: per circuit, all "shplonk" if None"""
    out = []
    for ci, circuit in enumerate(circuits):
        pchip, ctx = pchip_cls(), S.OracleCtx()
        for _t, proof in _proofs_of(pchip, ctx, circuit, kinds[ci] if kinds else "shplonk", make_transcript, conv):
            left, right, _names = S.evaluate_multiopen_proof(ctx, S.OracleFieldChip(), pchip, proof)
            out.append((left, right))
    return out


def verify_aggregation(pchip, circuits, kinds=None, conv=None):
    """the main transcript and the fold of V.verify_aggregation_proofs_in_chip (verify.rs:835-942) over proofs of either kind
    -> (left, right, lambda)"""
    ctx = S.OracleCtx()
    main = P.PoseidonTranscriptRead(b"")
    proofs = []
    for ci, circuit in enumerate(circuits):
        got = _proofs_of(pchip, ctx, circuit, kinds[ci] if kinds else "shplonk", None, conv)
        proofs += [p for _t, p in got]
        for t, _p in got:                                                              # verify.rs:909-913
            main.common_scalar(t.squeeze_challenge_scalar())
    lam = main.squeeze_challenge_scalar()
    left, right, _names = S.evaluate_multiopen_proof(ctx, S.OracleFieldChip(), pchip, S.aggregate_fold(proofs, lam))
    return left, right, lam
