"""Test-side HONEST prover: a proof built from a witness, stage by stage, that the reference's verifier (oracle/verifier.py,
and the library's from-bytes verifier tied to it) accepts.  Unlike tests/toy_prover.py nothing here is solved for with the
trapdoor: commitments are commitments of polynomials, evaluations are their values, h is the quotient, W the GWC openings.

One driver, `prove`, owns the transcript, draws the blinding rows and the random polynomial from one seeded random.Random in
a fixed order, computes x^n and the combination sum_i (x^n)^i h_i with Python integers, and lists the opening queries in the
order of oracle/verifier.py::queries (:359-399).  It walks create_proof's order as oracle/verifier.py::build_params (:201-273)
reads it back.  Everything else is "do this stage", answered by one of two backends with one interface (columns are lists
of integers at the interface, points are oracle points):

  PyStages      the restatements of tests/*_ref.py composed; commitments are p(tau) * G in the exponent
  DeviceStages  the package's public layer only (poly.py and the engine); no field arithmetic on polynomial-sized data
                in Python — the columns are only encoded to and decoded from the 32-byte form

The two must agree byte for byte (tests/test_gpu_honest_proofs.py).  The misreadings of tests/test_honest_prover_host.py's
sensitivity table override one PyStages method or one Driver step each.  Checker-side infrastructure: the library has no
create_proof."""
from __future__ import annotations

import copy
import hashlib
from dataclasses import dataclass, field
from typing import List

from oracle import bn254 as O
from oracle import pairing as E
from oracle import poseidon as P
from oracle import verifier as V
from tests import keygen_ref as K
from tests import poly_open_ref as PO
from tests import quotient_ref as Q
from tests import toy_prover_hash as TH
from tests.fr_bytes import dec, enc, fe
from tests.grand_product_ref import DELTA, lookup_product_py, permutation_product_py
from tests.lookup_permute_ref import lookup_permute_py
from tests.toy_prover import Setup

R = O.R
INSTANCE_ROWS = 4


# ---------------------------------------------------------------------------------------------- the circuit
@dataclass
class Circuit:
    """the challenge-independent part of Q.satisfied_circuit: shape (no commitments yet), witness and fixed columns as rows, the
    copy constraints over the permutation columns, the instance values the verifier is handed"""
    cs: V.ConstraintSystem
    lag: dict
    copies: list

    @property
    def usable(self) -> int:
        return self.cs.n - self.cs.blinding_factors - 1

    @property
    def instances(self):
        """[inner proof][column][values]: the first rows of the instance column"""
        return [[list(self.lag["instance"][0][:INSTANCE_ROWS])]]

    def with_cell(self, kind: str, column: int, row: int, value: int) -> "Circuit":
        """the same circuit (shape, fixed columns, copy constraints) over a witness with one cell changed"""
        lag = {k: [list(c) for c in cols] for k, cols in self.lag.items()}
        lag[kind][column][row] = value % R
        return Circuit(self.cs, lag, self.copies)


def make_circuit(rng, k: int, degree: int) -> Circuit:
    cs, lag, classes = Q.circuit_witness(rng, k, degree)
    return Circuit(cs, lag, K.copies_from_classes(classes))


def broken_gate_cell(c: Circuit) -> Circuit:
    """row 3 of advice column c: a multiplication row"""
    assert c.lag["fixed"][0][3] == 1
    return c.with_cell("advice", 2, 3, c.lag["advice"][2][3] + 1)


def copied_cell_off_the_gates(c: Circuit):
    """-> (column, row) of a cell of advice column a that is copy-constrained, on a row where no selector is on and below which
    no gate reads it (a is read at the current row only), and away from the instance rows"""
    q_m, q_a = c.lag["fixed"][0], c.lag["fixed"][1]
    for lc, lr, rc, rr in c.copies:
        for col, row in ((lc, lr), (rc, rr)):
            if col == 0 and row >= INSTANCE_ROWS and not q_m[row] and not q_a[row]:
                return col, row
    raise AssertionError("no copied cell of column a outside the gates")


def broken_copied_cell(c: Circuit) -> Circuit:
    col, row = copied_cell_off_the_gates(c)
    return c.with_cell("advice", col, row, c.lag["advice"][col][row] + 1)


def outside_the_table(c: Circuit) -> Circuit:
    """row 2 of b, a usable row, moved to a value the table does not hold: permute_expression_pair has no answer, so the
    prover stops there (halo2: Error::ConstraintSystemFailure) and no proof is written"""
    table = set(c.lag["fixed"][2][:c.usable])
    v = 12345
    while v in table:
        v += 1
    return c.with_cell("advice", 1, 2, v)


# ---------------------------------------------------------------------------------------------- keys
@dataclass
class Key:
    sigma_lag: list
    sigma_coeff: list
    fixed_coeff: list
    fixed_commitments: list
    permutation_commitments: list


def vk_scalar(cs, key: Key) -> int:
    """the stand-in for from_bytes_wide(blake2b("Halo2-Verify-Key", pinned vk)) (verify.rs:57-70): the same hash over this
    key's shape and commitments — any scalar would do, this one moves with the key"""
    h = hashlib.blake2b(digest_size=64, person=b"Halo2-Verify-Key")
    h.update(repr((cs.k, cs.degree, cs.blinding_factors, cs.gates, cs.lookups, cs.permutation_columns)).encode())
    for pt in key.fixed_commitments + key.permutation_commitments:
        h.update(O.aff_to_bytes(pt))
    return O.fr_from_bytes_wide(h.digest())


# ---------------------------------------------------------------------------------------------- backend: the restatements
class PyStages:
    """every stage through tests/*_ref.py.  memo: a dict shared between instances — the stages are pure functions of their
    arguments, so a run that differs from an earlier one in a late step redoes only from that step"""

    def __init__(self, setup: Setup, memo=None):
        self.setup = setup
        self.memo = {} if memo is None else memo
        self.cs = None

    def close(self):
        pass

    def _memo(self, name, args, fn):
        key = (name, hashlib.sha256(repr(args).encode()).digest())
        if key not in self.memo:
            self.memo[key] = fn()
        return self.memo[key]

    def s_g2(self):
        return self.setup.s_g2

    # ---- keys
    def keygen(self, circuit: Circuit) -> Key:
        cs, k, u = circuit.cs, circuit.cs.k, circuit.usable
        m = len(cs.permutation_columns)

        def make():
            sig = K.sigmas_py(K.assembly_py(m, k, u, circuit.copies), m, k)
            fixed = circuit.lag["fixed"]
            return Key(sig, self.to_coeff(sig, k), self.to_coeff(fixed, k), self.commit_lagrange(fixed, k), self.commit_lagrange(sig, k))
        return self._memo("keygen", (k, u, m, circuit.copies, circuit.lag["fixed"], self.setup.tau), make)

    def load_key(self, cs):
        self.cs = cs

    # ---- commitments: p(tau) * G, the identity where p(tau) = 0
    def _g(self, d):
        d %= R
        return self._memo("g1", d, lambda: TH.g1_mul(d) if d else O.INF)

    def _commit(self, coeffs):
        return [self._g(Q.horner(c, self.setup.tau)) for c in coeffs]

    def commit_coeff(self, cols, k):
        """against g: the columns are coefficients"""
        return self._commit(cols)

    def commit_lagrange(self, cols, k):
        """against g_lagrange: the columns are evaluations over the domain"""
        return self._commit([Q.ntt(c, k, inverse=True) for c in cols])

    # ---- domain
    def to_coeff(self, cols, k):
        return [Q.ntt(c, k, inverse=True) for c in cols]

    # ---- lookup
    def compress(self, which, j, lag, theta):
        return Q.expressions_rows_py(self.cs, which, j, lag["advice"], lag["fixed"], lag["instance"], [], theta)

    def permute(self, a, s, k, usable, blinding):
        ap, sp = lookup_permute_py(a, s, usable)
        top = (1 << k) - usable
        return ap + (blinding[0] if blinding else [0] * top), sp + (blinding[1] if blinding else [0] * top)

    # ---- grand products
    def set_start(self, s, chunk_len, previous_last):
        """-> (delta_first, init) of permutation set s: delta^(s * chunk_len), and the previous set's z[usable] (1 for s = 0)"""
        return pow(DELTA, s * chunk_len, R), previous_last

    def product_rows(self, usable):
        """the row z ends on (where l_last sits), for the products and the quotient"""
        return usable

    def permutation_products(self, values, sigmas, k, usable, beta, gamma, chunk_len, blinding):
        u = self.product_rows(usable)
        out, last = [], 1
        for s, lo in enumerate(range(0, len(values), chunk_len)):
            delta_first, init = self.set_start(s, chunk_len, last)
            z = permutation_product_py(values[lo:lo + chunk_len], sigmas[lo:lo + chunk_len], k, u, beta, gamma, DELTA, delta_first, init)
            last = z[u]
            out.append(_z_column(z, k, blinding[s] if blinding else None))
        return out

    def lookup_product(self, a, s, ap, sp, k, usable, beta, gamma, blinding):
        return _z_column(lookup_product_py(a, s, ap, sp, self.product_rows(usable), beta, gamma), k, blinding)

    # ---- the quotient
    def quotient(self, polys, scalars):
        cs = self.cs
        u = self.product_rows(cs.n - cs.blinding_factors - 1)
        if u != cs.n - cs.blinding_factors - 1:
            cs = copy.copy(cs)
            cs.blinding_factors = cs.n - u - 1
        args = Q.quotient_args(polys, scalars)
        shape = (cs.k, cs.degree, cs.blinding_factors, cs.gates, cs.lookups, cs.permutation_columns)
        return self._memo("quotient", (shape, args), lambda: Q.quotient_py(cs, *args)[0])

    # ---- openings
    def evaluate(self, polys, k, queries, points):
        return [Q.horner(polys[p], points[z]) for p, z in queries]

    def open(self, polys, k, queries, points, v):
        ws = []
        for z, members in group_queries(queries):
            c, vm = [0] * (1 << k), 1
            for p in members:
                c = [(x + vm * y) % R for x, y in zip(c, polys[p])]
                vm = vm * v % R
            ws.append(self._commit([PO.quotient_py(c, points[z])])[0])
        return ws


def _z_column(z, k, blinding):
    top = (1 << k) - len(z)
    assert blinding is None or len(blinding) >= top
    return list(z) + (list(blinding[:top]) if blinding is not None else [0] * top)


def group_queries(queries):
    """[(poly, point index)] -> [(point index, [poly, ...])] in first-seen order (multiopen.rs:31-43)"""
    groups = []
    for p, z in queries:
        for pt, members in groups:
            if pt == z:
                members.append(p)
                break
        else:
            groups.append((z, [p]))
    return groups


# ---------------------------------------------------------------------------------------------- backend: the library
class DeviceStages:
    """every stage through the package's public layer: poly.py and the engine.  Holds two base tables and one verifying key;
    close() frees them."""

    def __init__(self, pkg, eng, poly, verifier, setup: Setup):
        self.pkg, self.eng, self.poly, self.verifier, self.setup = pkg, eng, poly, verifier, setup
        self.vk = None
        self.g, self.gl = eng.params_setup(setup.k, fe(setup.tau))

    def close(self):
        if self.vk is not None:
            self.vk.close()
            self.vk = None
        if self.g is not None:
            self.eng.bases_free(self.g)
            self.eng.bases_free(self.gl)
            self.g = self.gl = None

    def s_g2(self):
        """[tau]_2 as 128 bytes"""
        g2 = b"".join(O.fe_to_bytes(c) for c in (E.G2[0][0], E.G2[0][1], E.G2[1][0], E.G2[1][1]))
        return self.pkg.g2_scalar_mul(g2, fe(self.setup.tau))

    @staticmethod
    def _cols(cols):
        return [enc(c) for c in cols]

    @staticmethod
    def _ints(cols):
        return [dec(c) for c in cols]

    @staticmethod
    def _points(affs):
        return [O.aff_from_bytes(a) for a in affs]

    def keygen(self, circuit: Circuit) -> Key:
        cs, k, u = circuit.cs, circuit.cs.k, circuit.usable
        m = len(cs.permutation_columns)
        mapping = self.poly.permutation_mapping(m, k, u, circuit.copies)
        sig_lag, sig_coeff, sig_commit = self.poly.permutation_key(self.eng, self.gl, mapping, m, k, u, fe(DELTA))
        fixed_coeff, fixed_commit = self.poly.fixed_key(self.eng, self.gl, self._cols(circuit.lag["fixed"]), k)
        return Key(self._ints(sig_lag), self._ints(sig_coeff), self._ints(fixed_coeff), self._points(fixed_commit),
                   self._points(sig_commit))

    def load_key(self, cs):
        if self.vk is not None:
            self.vk.close()
        self.vk = self.verifier.VerifyingKey(self.eng, self.verifier.encode_vk(cs, O.aff_to_bytes))

    def commit_coeff(self, cols, k):
        return self._points(self.poly.commit_columns_coeff(self.eng, self.g, self._cols(cols), k))

    def commit_lagrange(self, cols, k):
        return self._points(self.poly.commit_columns_lagrange(self.eng, self.gl, self._cols(cols), k))

    def to_coeff(self, cols, k):
        return self._ints(self.poly.columns_lagrange_to_coeff(self.eng, self._cols(cols), k))

    def compress(self, which, j, lag, theta):
        return dec(self.poly.expressions_eval(self.eng, self.vk, which, j, self._cols(lag["advice"]), self._cols(lag["fixed"]),
                                              self._cols(lag["instance"]), [], fold=fe(theta)))

    def permute(self, a, s, k, usable, blinding):
        ap, sp = self.poly.permute_expression_pair(self.eng, enc(a), enc(s), k, usable,
                                                   None if not blinding else (enc(blinding[0]), enc(blinding[1])))
        return dec(ap), dec(sp)

    def permutation_products(self, values, sigmas, k, usable, beta, gamma, chunk_len, blinding):
        return self._ints(self.poly.permutation_products(self.eng, self._cols(values), self._cols(sigmas), k, usable, fe(beta), fe(gamma),
                                                         fe(DELTA), chunk_len, None if not blinding else self._cols(blinding)))

    def lookup_product(self, a, s, ap, sp, k, usable, beta, gamma, blinding):
        return dec(self.poly.lookup_product(self.eng, enc(a), enc(s), enc(ap), enc(sp), k, usable, fe(beta), fe(gamma),
                                            None if blinding is None else enc(blinding)))

    def quotient(self, polys, scalars):
        sc = scalars
        return self._ints(self.poly.quotient_pieces(self.eng, self.vk, *[self._cols(polys[kind]) for kind in Q.POLY_KINDS], [],
                                                    fe(sc["theta"]), fe(sc["beta"]), fe(sc["gamma"]), fe(sc["y"]), fe(sc["delta"])))

    def evaluate(self, polys, k, queries, points):
        return dec(self.eng.fr_poly_eval(b"".join(self._cols(polys)), k, queries, enc(points)))

    def open(self, polys, k, queries, points, v):
        _evals, groups, ws = self.poly.multiopen_prove(self.eng, self.g, b"".join(self._cols(polys)), k, queries, enc(points), fe(v))
        assert [pt for pt, _m in groups] == [pt for pt, _m in group_queries(queries)]
        return self._points(ws)


# ---------------------------------------------------------------------------------------------- the driver
class Driver:
    """the driver's own conventions, one method each, so a test can misread one"""

    def point(self, x, omega, rotation):
        """the point a polynomial queried at `rotation` is opened at"""
        return V.rotate_omega(x, omega, rotation)

    def h_commitment_order(self, commitments):
        """h_0 first (vanish.rs:18-72 folds them from the top with x^n)"""
        return list(commitments)

    def w_order(self, rotations, ws):
        """one W per rotation, in the order the rotations are first seen among the queries (multiopen.rs:31-43)"""
        return list(ws)


class _Recorder:
    """a transcript writer that remembers what every stretch of its output is"""

    def __init__(self, writer):
        self.w, self.fields = writer, []

    def point(self, name, pt):
        at = len(self.w.out)
        self.w.write_point(pt)
        self.fields.append((name, at, len(self.w.out)))

    def scalar(self, name, s):
        at = len(self.w.out)
        self.w.write_scalar(s)
        self.fields.append((name, at, len(self.w.out)))


@dataclass
class Proof:
    cs: V.ConstraintSystem              # the shape with the key's commitments and vk_scalar
    instances: list                     # [inner proof][column][values], as the verifier takes them
    data: bytes
    fields: list = field(default_factory=list)      # (name, start, end) of every point and scalar of data

    def __iter__(self):                 # (cs_with_commitments, instances, proof_bytes)
        return iter((self.cs, self.instances, self.data))


def prove(circuit: Circuit, setup: Setup, stages, rng, writer_cls=P.PoseidonTranscriptWrite, blinding=True, driver=None) -> Proof:
    """one proof of `circuit` under `setup` by the stages of `stages`.  rng: a random.Random — the blinding rows of a', s', of
    every permutation Z and of the lookup's Z, then the random polynomial, are drawn from it first, in that order, whatever
    the backend.  blinding None / False: the blinding rows are zero (the random polynomial is still drawn)."""
    assert stages.setup is setup and setup.k == circuit.cs.k
    driver = driver or Driver()
    cs0, lag = circuit.cs, circuit.lag
    k, n, bf, u = cs0.k, cs0.n, cs0.blinding_factors, circuit.usable
    assert len(cs0.lookups) == 1 and cs0.num_challenges == 0 and cs0.phases() == [0]
    nsets = cs0.num_permutation_sets
    rnd = lambda count: [rng.randrange(R) for _ in range(count)]
    blind_ap, blind_sp = rnd(n - u), rnd(n - u)
    blind_pz = [rnd(n - u - 1) for _ in range(nsets)]
    blind_lz = rnd(n - u - 1)
    random_poly = rnd(n)
    if not blinding:
        blind_ap = blind_sp = blind_pz = blind_lz = None

    # ---- the key
    key = stages.keygen(circuit)
    cs = copy.copy(cs0)
    cs.fixed_commitments, cs.permutation_commitments = list(key.fixed_commitments), list(key.permutation_commitments)
    cs.vk_scalar = vk_scalar(cs0, key)
    stages.load_key(cs)

    t = _Recorder(writer_cls())
    w = t.w
    w.common_scalar(cs.vk_scalar)
    for pt in stages.commit_lagrange(lag["instance"], k):
        w.common_point(pt)
    for i, pt in enumerate(stages.commit_lagrange(lag["advice"], k)):
        t.point("advice commitment %d" % i, pt)
    theta = w.squeeze_challenge_scalar()

    # ---- the lookup's permuted pair
    a_in = stages.compress(1, 0, lag, theta)
    s_in = stages.compress(2, 0, lag, theta)
    ap, sp = stages.permute(a_in, s_in, k, u, (blind_ap, blind_sp) if blinding else None)
    for name, pt in zip(("permuted input commitment", "permuted table commitment"), stages.commit_lagrange([ap, sp], k)):
        t.point(name, pt)
    beta = w.squeeze_challenge_scalar()
    gamma = w.squeeze_challenge_scalar()

    # ---- the grand products
    columns = [lag[kind][col] for kind, col in cs.permutation_columns]
    pz = stages.permutation_products(columns, key.sigma_lag, k, u, beta, gamma, cs.chunk_len, blind_pz)
    lz = stages.lookup_product(a_in, s_in, ap, sp, k, u, beta, gamma, blind_lz)
    for i, pt in enumerate(stages.commit_lagrange(pz + [lz], k)):
        t.point("permutation product commitment %d" % i if i < nsets else "lookup product commitment", pt)
    t.point("random commitment", stages.commit_coeff([random_poly], k)[0])
    y = w.squeeze_challenge_scalar()

    # ---- the quotient
    coeff = stages.to_coeff(lag["advice"] + lag["instance"] + pz + [lz, ap, sp], k)
    polys = {"advice": coeff[:3], "fixed": key.fixed_coeff, "instance": coeff[3:4], "sigma": key.sigma_coeff,
             "perm_z": coeff[4:4 + nsets], "lookup_z": [coeff[4 + nsets]], "lookup_ap": [coeff[5 + nsets]],
             "lookup_sp": [coeff[6 + nsets]]}
    scalars = {"challenges": [], "theta": theta, "beta": beta, "gamma": gamma, "y": y, "delta": DELTA}
    pieces = stages.quotient(polys, scalars)
    assert len(pieces) == cs.quotient_poly_degree
    for i, pt in enumerate(driver.h_commitment_order(stages.commit_coeff(pieces, k))):
        t.point("h piece %d" % i, pt)
    x = w.squeeze_challenge_scalar()

    # ---- the evaluations: one slab, the queries in the order of oracle/verifier.py::queries
    xn = pow(x, n, R)
    h_comb, xp = [0] * n, 1
    for piece in pieces:                                               # sum_i (x^n)^i h_i: the polynomial behind the vanishing query
        h_comb = [(acc + xp * c) % R for acc, c in zip(h_comb, piece)]
        xp = xp * xn % R
    slab, index = [], {}

    def put(name, cols):
        for i, col in enumerate(cols):
            index[(name, i)] = len(slab)
            slab.append(col)
    for name in ("instance", "advice", "perm_z", "lookup_z", "lookup_ap", "lookup_sp", "fixed", "sigma"):
        put(name, polys[name])
    put("h", [h_comb])
    put("random", [random_poly])
    last = -(bf + 1)
    named = []                                                         # (polynomial, rotation) in the order of V.queries
    named += [(("instance", c), r) for c, r in cs.instance_queries]                                    # :360-362
    named += [(("advice", c), r) for c, r in cs.advice_queries]                                        # :363-365
    for s in range(nsets):                                                                             # :368-371
        named += [(("perm_z", s), 0), (("perm_z", s), 1)]
    named += [(("perm_z", s), last) for s in range(nsets - 2, -1, -1)]                                 # :372-375
    named += [(("lookup_z", 0), 0), (("lookup_ap", 0), 0), (("lookup_sp", 0), 0), (("lookup_ap", 0), -1),
              (("lookup_z", 0), 1)]                                                                    # :376-386
    named += [(("fixed", c), r) for c, r in cs.fixed_queries]                                          # :387-389
    named += [(("sigma", g), 0) for g in range(len(cs.permutation_columns))]                           # :390-391
    named += [(("h", 0), 0), (("random", 0), 0)]                                                       # :393-399
    rotations = []
    for _p, r in named:
        if r not in rotations:
            rotations.append(r)
    points = [driver.point(x, cs.omega, r) for r in rotations]
    queries = [(index[p], rotations.index(r)) for p, r in named]
    values = dict(zip(named, stages.evaluate(slab, k, queries, points)))
    # ... written in the order build_params reads them (:229-256)
    for q, (c, r) in enumerate(cs.instance_queries):
        t.scalar("instance evaluation %d" % q, values[(("instance", c), r)])
    for q, (c, r) in enumerate(cs.advice_queries):
        t.scalar("advice evaluation %d" % q, values[(("advice", c), r)])
    for q, (c, r) in enumerate(cs.fixed_queries):
        t.scalar("fixed evaluation %d" % q, values[(("fixed", c), r)])
    t.scalar("random evaluation", values[(("random", 0), 0)])
    for g in range(len(cs.permutation_columns)):
        t.scalar("sigma evaluation %d" % g, values[(("sigma", g), 0)])
    for s in range(nsets):
        t.scalar("permutation product %d evaluation" % s, values[(("perm_z", s), 0)])
        t.scalar("permutation product %d next evaluation" % s, values[(("perm_z", s), 1)])
        if s + 1 < nsets:
            t.scalar("permutation product %d last evaluation" % s, values[(("perm_z", s), last)])
    for name, p, r in (("lookup product evaluation", "lookup_z", 0), ("lookup product next evaluation", "lookup_z", 1),
                       ("permuted input evaluation", "lookup_ap", 0), ("permuted input inverse evaluation", "lookup_ap", -1),
                       ("permuted table evaluation", "lookup_sp", 0)):
        t.scalar(name, values[((p, 0), r)])
    v = w.squeeze_challenge_scalar()

    # ---- the openings
    ws = stages.open(slab, k, queries, points, v)
    assert len(ws) == len(rotations)
    for i, pt in enumerate(driver.w_order(rotations, ws)):
        t.point("W %d" % i, pt)
    return Proof(cs, circuit.instances, w.finalize(), t.fields)


def first_difference(got: Proof, want: Proof):
    """the name of the first transcript field in which two proofs of one shape differ, or None"""
    for (name, lo, hi), (name2, lo2, hi2) in zip(got.fields, want.fields):
        assert (name, lo, hi) == (name2, lo2, hi2), "the two proofs are not laid out alike"
        if got.data[lo:hi] != want.data[lo:hi]:
            return name
    return None if got.data == want.data else "length"


# ---------------------------------------------------------------------------------------------- the oracle's verdict
def circuit_proofs(name: str, setup: Setup, proofs: List[Proof], instances=None) -> V.CircuitProofs:
    """proofs of ONE circuit (one key) as the oracle's aggregation driver takes them"""
    assert all(p.cs.vk_scalar == proofs[0].cs.vk_scalar for p in proofs)
    c = V.CircuitProofs(name, proofs[0].cs, setup.g_lagrange)
    for i, p in enumerate(proofs):
        c.proofs.append((p.instances if instances is None else instances[i], p.data))
    return c


def oracle_accepts(setup: Setup, circuits, make_transcript=None) -> bool:
    """verify_aggregation_proofs_in_chip, then the pairing check e(left, [tau]_2) e(right, -[1]_2) == 1 (verify.rs:733-739).
    Anything but a verdict (a proof that does not parse) is an exception, not False."""
    left, right, _plain, _commits, _lam = V.verify_aggregation_proofs_in_chip(TH.CrefEccChip(), circuits, make_transcript=make_transcript)
    return E.pairing_check([(left, setup.s_g2), (right, E.g2_neg(setup.g2))])
