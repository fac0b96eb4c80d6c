"""Crafted inputs for the from-bytes verifier: the points and values a proof MAY hold but that a random generator reaches
with probability ~2^-127, and the byte surgery that puts them into a trapdoor proof (tests/toy_prover.py).  Python integers
and the oracle's tuples only; used by tests/test_exceptional_points_host.py (CPU) and tests/test_gpu_exceptional_proofs.py.

  X_R, X_TOP   curve points whose x lies in [r, p): PoseidonEncode reduces a coordinate mod r (mock/transcript_encode.rs:28-50),
               and p - r ~ 2^127, so only such a point takes the subtracting branch of the device's reduction
  Y_R, Y_TOP   the same for y (x is then a cube root of y^2 - 3)
  negations    the other sign bit of the compressed encoding; for Y_* a SMALL y (p - y < p - r)
  INF, G, -G   the identity (32 zero bytes on the wire) and the generator the verifier itself multiplies

No point of the curve used here has both coordinates >= r.
"""
from __future__ import annotations

import copy

from oracle import bn254 as O
from oracle import verifier as V

P, R = O.P, O.R


# ---------------------------------------------------------------------------------------------- roots in Fq
def fq_sqrt(a: int):
    """p = 3 mod 4: a^((p+1)/4), or None when a is not a square"""
    a %= P
    y = pow(a, (P + 1) // 4, P)
    return y if y * y % P == a else None


def _three_sylow():
    """p - 1 = 3^s t with 3 not dividing t -> (s, t, a generator of the subgroup of order 3^s)"""
    s, t = 0, P - 1
    while t % 3 == 0:
        s, t = s + 1, t // 3
    c = 2
    while pow(c, (P - 1) // 3, P) == 1:      # the smallest non-cube
        c += 1
    return s, t, pow(c, t, P)


_S3, _T3, _G3 = _three_sylow()
assert _S3 == 2                              # p = 1 mod 9: x -> x^3 is 3-to-1 and no single exponent inverts it


def fq_cbrt(a: int):
    """3-adic Tonelli-Shanks: x0 = a^(3^-1 mod t) has x0^3 = a * e with e in the 3-Sylow subgroup; for a cube a, e is itself a
    cube there, e = (g^j)^3, and x0 * g^-j is a root.  -> the SMALLEST of the three roots, or None when a is not a cube"""
    a %= P
    if a == 0:
        return 0
    if pow(a, (P - 1) // 3, P) != 1:
        return None
    x0 = pow(a, pow(3, -1, _T3), P)
    for j in range(3 ** _S3):
        x = x0 * pow(_G3, j, P) % P
        if pow(x, 3, P) == a:
            w = pow(_G3, 3 ** (_S3 - 1), P)  # a primitive cube root of unity
            return min(x, x * w % P, x * w % P * w % P)
    raise AssertionError("a cube without a cube root")


def point_with_x(x: int):
    y = fq_sqrt(x * x * x + O.B)
    return None if y is None else (x, y)


def point_with_y(y: int):
    x = fq_cbrt(y * y - O.B)
    return None if x is None else (x, y)


def first_point(make, start: int):
    v = start
    while make(v) is None:
        v += 1
    return make(v)


X_R = first_point(point_with_x, R)           # x = r + 2
X_TOP = point_with_x(P - 1)                  # (p - 1)^3 + 3 = 2, a square mod p
Y_R = first_point(point_with_y, R)           # y = r + 1
Y_TOP = point_with_y(P - 1)                  # (p - 1)^2 - 3 = -2, a cube mod p
INF, G, NEG_G = O.INF, O.G1, O.neg(O.G1)

BIG = {"X_R": X_R, "X_TOP": X_TOP, "Y_R": Y_R, "Y_TOP": Y_TOP}
CRAFTED = dict(BIG)
CRAFTED.update({"-" + k: O.neg(v) for k, v in BIG.items()})
NON_IDENTITY = dict(CRAFTED, G=G, **{"-G": NEG_G})
CRAFTED.update({"INF": INF, "G": G, "-G": NEG_G})


# ---------------------------------------------------------------------------------------------- a proof's slots
class ProofLayout:
    """where the items of ONE proof sit in its bytes, from the oracle's reading order (oracle/verifier.py build_params): advice
    commitments by phase, permuted lookup pairs, permutation products, lookup products, the random commitment, the vanishing
    commitments, the evaluations, the W points.  point_bytes: 32 (Poseidon: compressed) or 64 (ShaRead: uncompressed).
    A slot is (byte offset, width)."""

    def __init__(self, cs: V.ConstraintSystem, proof_len: int, point_bytes: int = 32):
        pb = self.point_bytes = point_bytes
        k = 0
        self.advice = [None] * cs.num_advice_columns
        for phase in cs.phases():
            for col, ph in enumerate(cs.advice_column_phase):
                if ph == phase:
                    self.advice[col] = (pb * k, pb)
                    k += 1
        take = lambda n: [(pb * (k + i), pb) for i in range(n)]
        self.lookup_permuted = take(2 * len(cs.lookups))
        k += 2 * len(cs.lookups)
        self.permutation_products = take(cs.num_permutation_sets)
        k += cs.num_permutation_sets
        self.lookup_products = take(len(cs.lookups))
        k += len(cs.lookups)
        self.random = (pb * k, pb)
        k += 1
        self.vanishing = take(cs.quotient_poly_degree)
        k += cs.quotient_poly_degree
        self.n_evals = len(cs.instance_queries) + len(cs.advice_queries) + len(cs.fixed_queries) + 1 + \
            len(cs.permutation_commitments) + (3 * cs.num_permutation_sets - 1 if cs.num_permutation_sets else 0) + \
            5 * len(cs.lookups)
        self.evals_at = pb * k
        w_at = self.evals_at + 32 * self.n_evals
        assert proof_len >= w_at and (proof_len - w_at) % pb == 0
        self.w = [(w_at + pb * i, pb) for i in range((proof_len - w_at) // pb)]
        self.proof_len = proof_len


def encode_point(point, width: int) -> bytes:
    return O.compress(point) if width == 32 else O.aff_to_bytes(point)


def replace_point(proof_bytes: bytes, slot, point) -> bytes:
    """point: an oracle tuple / O.INF, or the bytes to put there"""
    off, width = slot
    b = point if isinstance(point, (bytes, bytearray)) else encode_point(point, width)
    assert len(b) == width and off + width <= len(proof_bytes)
    return proof_bytes[:off] + bytes(b) + proof_bytes[off + width:]


def replace_scalars(proof_bytes: bytes, layout: ProofLayout, values) -> bytes:
    """the whole evaluation block <- values (one integer for all, or a list of n_evals)"""
    vs = [values] * layout.n_evals if isinstance(values, int) else list(values)
    assert len(vs) == layout.n_evals and len(proof_bytes) == layout.proof_len
    at = layout.evals_at
    return proof_bytes[:at] + b"".join(O.fe_to_bytes(v % R) for v in vs) + proof_bytes[at + 32 * layout.n_evals:]


def read_point(proof_bytes: bytes, slot):
    off, width = slot
    b = proof_bytes[off:off + width]
    return O.decompress(b) if width == 32 else O.aff_from_bytes(b)


# ---------------------------------------------------------------------------------------------- variants of a batch
# A variant maps the four ordinary proofs of ONE circuit ([(instances, bytes)] as V.CircuitProofs holds them) to four proofs,
# so that one run of the oracle prices several substitutions.  `touched`: the proofs whose own pairing must now fail.
def _patch(proofs, k, *subs):
    inst, data = proofs[k]
    for slot, point in subs:
        data = replace_point(data, slot, point)
    proofs[k] = (inst, data)


def big_coordinates(cs, lay, proofs):
    ps = list(proofs)
    _patch(ps, 1, (lay.advice[0], X_R), (lay.advice[1], Y_R))
    _patch(ps, 2, (lay.w[0], Y_TOP), (lay.w[-1], X_TOP))
    return ps


def identities(cs, lay, proofs):
    ps = list(proofs)
    zero = bytes(lay.point_bytes)
    _patch(ps, 1, (lay.advice[0], zero))
    _patch(ps, 2, ((lay.permutation_products or lay.lookup_products)[-1], zero))
    _patch(ps, 3, (lay.w[-1], zero))
    return ps


def dependent_points(cs, lay, proofs):
    ps = list(proofs)
    q = read_point(proofs[0][1], lay.advice[0])
    _patch(ps, 1, *[(slot, q) for slot in lay.advice])
    _patch(ps, 2, (lay.advice[0], q), (lay.advice[1], O.neg(q)))
    _patch(ps, 3, (lay.advice[0], cs.fixed_commitments[0]), (lay.w[0], G), (lay.w[-1], NEG_G))
    return ps


def flat_evaluations(cs, lay, proofs):
    ps = list(proofs)
    for k, v in ((1, 0), (2, R - 1), (3, 1)):
        ps[k] = (ps[k][0], replace_scalars(ps[k][1], lay, v))
    return ps


def repeated_proof(cs, lay, proofs):
    return [proofs[0], proofs[0], proofs[1], proofs[0]]


def flat_instances(cs, lay, proofs):
    ps = list(proofs)
    for k, v in ((1, R - 1), (2, 0), (3, 1)):
        inst, data = ps[k]
        ps[k] = ([[[v] * len(col) for col in row] for row in inst], data)
    return ps


# name -> (function, touched proofs, whether the aggregation is accepted)
VARIANTS = {
    "big_coordinates": (big_coordinates, {1, 2}, False),
    "identities": (identities, {1, 2, 3}, False),
    "dependent_points": (dependent_points, {1, 2, 3}, False),
    "flat_evaluations": (flat_evaluations, {1, 2, 3}, False),
    "repeated_proof": (repeated_proof, set(), True),
    "flat_instances": (flat_instances, {1, 2, 3}, False),
}


def apply_variant(name, circuit, point_bytes: int = 32):
    """-> a copy of `circuit` (V.CircuitProofs with four proofs) holding the variant's proofs"""
    fn, _touched, _accepted = VARIANTS[name]
    lay = ProofLayout(circuit.cs, len(circuit.proofs[0][1]), point_bytes)
    out = copy.copy(circuit)
    out.proofs = fn(circuit.cs, lay, list(circuit.proofs))
    return out


def identity_key_batch(seed: int, shape: dict, nproofs: int = 2):
    """a key that HOLDS the identity: fixed_commitments[0] (an all-zero fixed column) and the last permutation commitment are
    O.INF, discrete logarithm 0 for the trapdoor prover (DlogChip maps O.INF to 0); -> (setup, [circuit]) with valid proofs"""
    from tests import toy_prover as T
    rng = O.SplitMix64(seed)
    dlogs = {}
    setup = T.Setup(5, rng.fr(), 16)
    cs = T.make_constraint_system(rng, dlogs=dlogs, **shape)
    cs.fixed_commitments[0] = O.INF
    cs.permutation_commitments[-1] = O.INF
    c = V.CircuitProofs("circuit0", cs, setup.g_lagrange)
    for i in range(nproofs):
        instances = [[[rng.fr() for _ in range(3 + col)] for col in range(cs.num_instance_columns)]]
        c.proofs.append((instances, T.prove(cs, setup, rng, instances, dlogs, "%s_p%d" % (c.name, i))))
    return setup, [c]
