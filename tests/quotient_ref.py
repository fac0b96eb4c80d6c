"""The definitions of include/h2agg.h's quotient block restated with Python integers, and the constructions the tests feed
them.  expressions_rows_py evaluates a key's expressions row by row through oracle/verifier.py::evaluate_expression;
quotient_py is the definition of h2agg_quotient taken literally on the WHOLE extended coset (one transform of size 2^(k+e)
per polynomial, a rotation is an index offset of t * 2^e) — not coset by coset, which is the device's route;
verifier_numerator is what the reference's verifier computes from evaluations at a point x (oracle/verifier.py::queries,
lines 348-356 and 393: params.rs:74-224, vanish.rs:18-72), which tests/test_quotient_host.py holds against quotient_py;
satisfied_circuit is a small real circuit with a witness, copy constraints, a lookup and blinding rows."""
import random

from oracle import bn254 as O
from oracle import verifier as V
from tests.grand_product_ref import DELTA, lookup_product_py, permutation_chain_py
from tests.lookup_permute_ref import compress_py, lookup_permute_py

R = O.R
# bn256::Fr::ZETA as the package's poly.py derives it from the GLV basis (a1 + b1 zeta = 0 mod r, b1 = -B1N)
ZETA = 0x6f4d8248eeb859fc8211bbeb7d4f1128 * pow(0x89d3256894d213e3, R - 2, R) % R
assert pow(ZETA, 3, R) == 1 and ZETA != 1


def omega(k):
    return V.omega_for_k(k) if k else 1


def ntt(vals, k, shift=1, inverse=False):
    """h2agg_fr_fft: out[i] = sum_j (shift^j in[j]) w^(i j); inverse: out[j] = shift^-j / n sum_i in[i] w^(-i j)"""
    n = 1 << k
    assert len(vals) == n
    w = omega(k)
    a = [v % R for v in vals]
    if inverse:
        w = pow(w, R - 2, R)
    else:
        s = 1
        for j in range(n):
            a[j] = a[j] * s % R
            s = s * shift % R
    j = 0                                              # bit reversal, then decimation in time
    for i in range(1, n):
        bit = n >> 1
        while j & bit:
            j ^= bit
            bit >>= 1
        j |= bit
        if i < j:
            a[i], a[j] = a[j], a[i]
    length = 2
    while length <= n:
        wl = pow(w, n // length, R)
        half = length >> 1
        tw = [1] * half
        for t in range(1, half):
            tw[t] = tw[t - 1] * wl % R
        for start in range(0, n, length):
            for t in range(half):
                x, y = a[start + t], a[start + t + half] * tw[t] % R
                a[start + t], a[start + t + half] = (x + y) % R, (x - y) % R
        length <<= 1
    if inverse:
        ninv, sinv, s = pow(n, R - 2, R), pow(shift, R - 2, R), 1
        for j in range(n):
            a[j] = a[j] * ninv % R * s % R
            s = s * sinv % R
    return a


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def extended_k(k, degree):
    e = 0
    while (1 << (k + e)) < (degree - 1) << k:
        e += 1
    return e


# ---------------------------------------------------------------------------------------------- keys
def make_cs(k, degree, num_advice, num_fixed, num_instance, advice_queries, fixed_queries, instance_queries, gates, lookups,
            permutation_columns, blinding_factors=5, num_challenges=0):
    """a ConstraintSystem whose commitments are the generator (the quotient reads none of them)"""
    return V.ConstraintSystem(
        k=k, num_advice_columns=num_advice, num_instance_columns=num_instance, num_challenges=num_challenges,
        advice_column_phase=[0] * num_advice, challenge_phase=[0] * num_challenges, advice_queries=list(advice_queries),
        instance_queries=list(instance_queries), fixed_queries=list(fixed_queries), gates=gates, lookups=lookups,
        permutation_columns=list(permutation_columns), degree=degree, blinding_factors=blinding_factors,
        fixed_commitments=[O.G1] * num_fixed, permutation_commitments=[O.G1] * len(permutation_columns), vk_scalar=1)


def expression_lists(cs, which, j=0):
    if which == 0:
        return [poly for gate in cs.gates for poly in gate]
    return list(cs.lookups[j][which - 1])


def expressions_rows_py(cs, which, j, advice, fixed, instance, challenges, fold=None):
    """h2agg_vk_expressions_eval on columns of integers: fold None -> one column per expression, else one column"""
    n = cs.n
    exprs = expression_lists(cs, which, j)
    cols = [[0] * n for _ in exprs]
    for i in range(n):
        fx = [fixed[c][(i + r) % n] for c, r in cs.fixed_queries]
        ad = [advice[c][(i + r) % n] for c, r in cs.advice_queries]
        ins = [instance[c][(i + r) % n] for c, r in cs.instance_queries]
        for e, expr in enumerate(exprs):
            cols[e][i] = V.evaluate_expression(expr, fx, ad, ins, challenges)
    return cols if fold is None else compress_py(cols, fold)


# ---------------------------------------------------------------------------------------------- the quotient
def quotient_py(cs, advice, fixed, instance, sigma, perm_z, lookup_z, lookup_ap, lookup_sp, challenges, theta, beta, gamma, y,
                delta):
    """every argument in front of `challenges`: a list of polynomials, n coefficients each.  -> (pieces h_0 .. h_{degree-2}, all
    2^(k+e) coefficients of H)"""
    k, n, bf = cs.k, cs.n, cs.blinding_factors
    u = n - bf - 1
    e = extended_k(k, cs.degree)
    K, N, step = k + e, n << e, 1 << e
    w_ext = omega(K)
    ext = lambda coeffs: ntt(list(coeffs) + [0] * (N - n), K, ZETA)
    lagrange = lambda rows: ext(ntt(rows, k, inverse=True))
    A, F, I = [ext(p) for p in advice], [ext(p) for p in fixed], [ext(p) for p in instance]
    SG, PZ = [ext(p) for p in sigma], [ext(p) for p in perm_z]
    LZ, LA, LS = [ext(p) for p in lookup_z], [ext(p) for p in lookup_ap], [ext(p) for p in lookup_sp]
    l0 = lagrange([1] + [0] * (n - 1))
    l_last = lagrange([int(i == u) for i in range(n)])
    l_blind = lagrange([int(i > u) for i in range(n)])
    c = cs.chunk_len
    nsets = cs.num_permutation_sets
    assert len(PZ) == nsets and len(SG) == len(cs.permutation_columns) and len(LZ) == len(cs.lookups)
    values = {"advice": A, "fixed": F, "instance": I}
    hv = [0] * N
    x = ZETA
    for j in range(N):
        at = lambda col, t=0: col[(j + t * step) % N]
        fx = [at(F[col], r) for col, r in cs.fixed_queries]
        ad = [at(A[col], r) for col, r in cs.advice_queries]
        ins = [at(I[col], r) for col, r in cs.instance_queries]
        ev = lambda expr: V.evaluate_expression(expr, fx, ad, ins, challenges)
        act = (1 - l_last[j] - l_blind[j]) % R
        E = [ev(poly) for gate in cs.gates for poly in gate]
        if nsets:
            E.append(l0[j] * (1 - at(PZ[0])) % R)
            zl = at(PZ[-1])
            E.append(l_last[j] * (zl * zl - zl) % R)
            for s in range(1, nsets):
                E.append(l0[j] * (at(PZ[s]) - at(PZ[s - 1], -(bf + 1))) % R)
            for s in range(nsets):
                left, right = at(PZ[s], 1), at(PZ[s])
                for g in range(s * c, min((s + 1) * c, len(SG))):
                    kind, col = cs.permutation_columns[g]
                    v = at(values[kind][col])
                    left = left * ((v + beta * at(SG[g]) + gamma) % R) % R
                    right = right * ((v + pow(delta, g, R) * beta % R * x + gamma) % R) % R
                E.append(act * (left - right) % R)
        for q, (inputs, tables) in enumerate(cs.lookups):
            a_in = V.mul_add_accumulate([ev(t) for t in inputs], theta)
            s_in = V.mul_add_accumulate([ev(t) for t in tables], theta)
            z, zn, ap, apm, sp = at(LZ[q]), at(LZ[q], 1), at(LA[q]), at(LA[q], -1), at(LS[q])
            E.append(l0[j] * (1 - z) % R)
            E.append(l_last[j] * (z * z - z) % R)
            E.append(act * (zn * (ap + beta) % R * (sp + gamma) - z * (a_in + beta) % R * (s_in + gamma)) % R)
            E.append(l0[j] * (ap - sp) % R)
            E.append(act * (ap - sp) % R * (ap - apm) % R)
        hv[j] = V.mul_add_accumulate(E, y) * pow(pow(x, n, R) - 1, R - 2, R) % R
        x = x * w_ext % R
    H = ntt(hv, K, ZETA, inverse=True)
    return [H[i * n:(i + 1) * n] for i in range(cs.degree - 1)], H


def verifier_numerator(cs, polys, scalars, x):
    """mul_add_accumulate(expressions at x, y) as the reference's verifier builds it (oracle/verifier.py:344-356, :393) from the
    evaluations of the polynomials at x and its rotations.  polys: the dict of satisfied_circuit / random_inputs (coefficient
    lists), scalars: the dict with challenges, theta, beta, gamma, y."""
    w = cs.omega
    at = lambda coeffs, rot=0: horner(coeffs, V.rotate_omega(x, w, rot))
    sets = []
    for s, z in enumerate(polys["perm_z"]):
        sets.append((None, at(z), at(z, 1), at(z, -(cs.blinding_factors + 1)) if s + 1 < len(polys["perm_z"]) else None))
    lookups = []
    for q, (inputs, tables) in enumerate(cs.lookups):
        lookups.append({"product_eval": at(polys["lookup_z"][q]), "product_next_eval": at(polys["lookup_z"][q], 1),
                        "permuted_input_eval": at(polys["lookup_ap"][q]), "permuted_input_inv_eval": at(polys["lookup_ap"][q], -1),
                        "permuted_table_eval": at(polys["lookup_sp"][q]), "input_expressions": inputs, "table_expressions": tables})
    vp = V.VerifierParams(
        key="", cs=cs, instance_commitments=[], instance_evals=[[at(polys["instance"][c], r) for c, r in cs.instance_queries]],
        challenges=list(scalars["challenges"]), advice_commitments=[],
        advice_evals=[[at(polys["advice"][c], r) for c, r in cs.advice_queries]],
        fixed_evals=[at(polys["fixed"][c], r) for c, r in cs.fixed_queries], permutation_evals=[at(p) for p in polys["sigma"]],
        permutation_sets=[sets], lookups=[lookups], vanish_commitments=[], random_commitment=None, random_eval=0, w=[],
        theta=scalars["theta"], beta=scalars["beta"], gamma=scalars["gamma"], y=scalars["y"], x=x, v=0, u=0, xn=pow(x, cs.n, R))
    ls = V.lagrange_commits(vp)
    l = cs.blinding_factors + 1
    l_0, l_last, l_blind = ls[0], ls[l], sum(ls[1:l]) % R
    expression = [V.evaluate_expression(poly, vp.fixed_evals, vp.advice_evals[0], vp.instance_evals[0], vp.challenges)
                  for gate in cs.gates for poly in gate]
    expression += V.permutation_expressions(vp, 0, l_0, l_last, l_blind)
    for lk in vp.lookups[0]:
        expression += V.lookup_expressions(vp, 0, lk, l_0, l_last, l_blind)
    return V.mul_add_accumulate(expression, vp.y)


def h_at(pieces, n, x):
    """(x^n - 1) sum_i x^(n i) h_i(x): the other side of the verifier's identity (vanish.rs:18-72)"""
    xn = pow(x, n, R)
    acc = 0
    for p in reversed(pieces):
        acc = (acc * xn + horner(p, x)) % R
    return (xn - 1) * acc % R


POLY_KINDS = ("advice", "fixed", "instance", "sigma", "perm_z", "lookup_z", "lookup_ap", "lookup_sp")


def quotient_args(polys, scalars):
    """the positional arguments of quotient_py behind cs"""
    return [polys[kind] for kind in POLY_KINDS] + [scalars[s] for s in ("challenges", "theta", "beta", "gamma", "y", "delta")]


def random_scalars(rng, num_challenges=0):
    return {"challenges": [rng.randrange(R) for _ in range(num_challenges)], "theta": rng.randrange(R), "beta": rng.randrange(R),
            "gamma": rng.randrange(R), "y": rng.randrange(R), "delta": DELTA}


def random_inputs(rng, cs):
    """random polynomials of the shapes the key asks for (the circuit is not satisfied), a few coefficients 0 and r - 1"""
    n = cs.n
    col = lambda: [rng.choice((0, R - 1)) if rng.randrange(16) == 0 else rng.randrange(R) for _ in range(n)]
    counts = {"advice": cs.num_advice_columns, "fixed": len(cs.fixed_commitments), "instance": cs.num_instance_columns,
              "sigma": len(cs.permutation_columns), "perm_z": cs.num_permutation_sets, "lookup_z": len(cs.lookups),
              "lookup_ap": len(cs.lookups), "lookup_sp": len(cs.lookups)}
    return {kind: [col() for _ in range(counts[kind])] for kind in POLY_KINDS}


def random_shape(rng, k, degree, n_perm, n_lookups, with_gates, blinding_factors=5, num_challenges=0):
    """a key of a given shape with random gates: 3 advice, 2 fixed, 1 instance column, rotations +1, -1 and -(bf + 1)"""
    from tests.toy_prover import random_expression

    class Rng:
        def next(self):
            return rng.randrange(1 << 32)

        def fr(self):
            return rng.randrange(R)
    advice_queries = [(0, 0), (1, 0), (2, 0), (0, 1), (2, -1), (1, -(blinding_factors + 1))]
    fixed_queries, instance_queries = [(0, 0), (1, 0), (1, 1)], [(0, 0)]
    shape = (len(fixed_queries), len(advice_queries), len(instance_queries), num_challenges)
    gates = [[random_expression(Rng(), shape, 3) for _ in range(1 + g % 2)] for g in range(3)] if with_gates else []
    lookups = [([random_expression(Rng(), shape, 2) for _ in range(1 + q)], [random_expression(Rng(), shape, 1) for _ in range(2)])
               for q in range(n_lookups)]
    kinds = [("advice", 0), ("fixed", 1), ("advice", 1), ("instance", 0), ("advice", 2), ("fixed", 0)]
    perm = [kinds[g % len(kinds)] for g in range(n_perm)]
    return make_cs(k, degree, 3, 2, 1, advice_queries, fixed_queries, instance_queries, gates, lookups, perm, blinding_factors,
                   num_challenges)


# ---------------------------------------------------------------------------------------------- a satisfied circuit
def circuit_witness(rng, k, degree):
    """The challenge-independent part of satisfied_circuit: the shape, the witness a, b, c, the fixed columns, the instance
    column, and the classes of equal cells of the usable rows (lists of (permutation column, row), in the order the cells
    are met).  Draws from rng exactly what satisfied_circuit drew in front of its challenges.  -> (cs, lagrange, classes)"""
    assert degree >= 4
    n, bf = 1 << k, 5
    u = n - bf - 1
    rnd = lambda: rng.randrange(R)
    t = [rnd() for _ in range(n)]
    b = [t[rng.randrange(u)] if i < u else rnd() for i in range(n)]
    q_m = [int(i < u and i % 3 == 0) for i in range(n)]
    q_a = [int(i < u and i % 3 == 1) for i in range(n)]
    a, c = [0] * n, [0] * n
    for i in range(n):
        a[i] = c[rng.randrange(i)] if 0 < i < u and rng.randrange(2) else rnd()
        c[i] = a[i] * b[i] % R if q_m[i] else (a[i] + b[(i + 1) % n]) % R if q_a[i] else rnd()
    inst = [a[i] if i < 4 else 0 for i in range(n)]
    advice_queries = [(0, 0), (1, 0), (2, 0), (1, 1)]
    fixed_queries, instance_queries = [(0, 0), (1, 0), (2, 0)], [(0, 0)]
    A, B, C, B1 = (("advice", q) for q in range(4))
    QM, QA, T = (("fixed", q) for q in range(3))
    gates = [[("product", QM, ("sum", ("product", A, B), ("neg", C)))],
             [("product", QA, ("sum", ("sum", A, B1), ("neg", C)))]]
    lookups = [([B, ("scaled", B, 7)], [T, ("scaled", T, 7)])]
    perm = [("advice", 0), ("advice", 1), ("advice", 2), ("fixed", 0), ("fixed", 1), ("fixed", 2), ("instance", 0)]
    cs = make_cs(k, degree, 3, 3, 1, advice_queries, fixed_queries, instance_queries, gates, lookups, perm, bf)
    assert cs.num_permutation_sets >= 2 and len(perm) % cs.chunk_len
    lag = {"advice": [a, b, c], "fixed": [q_m, q_a, t], "instance": [inst]}
    # ---- the permutation: equal cells of the usable rows form one class each
    columns = [lag[kind][col] for kind, col in perm]
    classes = {}
    for j, colv in enumerate(columns):
        for i in range(u):
            classes.setdefault(colv[i], []).append((j, i))
    assert any(len(cells) > 1 for cells in classes.values())
    return cs, lag, list(classes.values())


def satisfied_circuit(rng, k, degree):
    """A circuit that holds, with everything a prover hands to the quotient.  Advice a, b, c; fixed q_m, q_a (selectors, 0 on
    the rows from u up) and t (a table); one instance column.  Gates q_m (a b - c) and q_a (a + b(wX) - c); one lookup
    (b, 7 b) in (t, 7 t); a permutation over all seven columns — the cycles of equal cells on the usable rows — which is
    more than chunk_len columns for degree <= 8, so there are at least two sets and the last one is ragged.  Random blinding
    rows.  Z, a', s' come from tests/grand_product_ref.py and tests/lookup_permute_ref.py.  degree >= 4 (the lookup's
    identity has degree 4).  The witness is circuit_witness's; the challenges are drawn behind it.
    -> (cs, lagrange, polys, scalars): columns as rows, the same as coefficient lists, the scalars."""
    cs, lag, classes = circuit_witness(rng, k, degree)
    n, bf = cs.n, cs.blinding_factors
    u = n - bf - 1
    rnd = lambda: rng.randrange(R)
    perm = cs.permutation_columns
    sc = random_scalars(rng)
    # ---- the permutation: every class is one cycle
    columns = [lag[kind][col] for kind, col in perm]
    to = {}
    for cells in classes:
        for pos, cell in enumerate(cells):
            to[cell] = cells[(pos + 1) % len(cells)]
    w = cs.omega
    label = lambda j, i: pow(DELTA, j, R) * pow(w, i, R) % R
    sigmas = [[label(*to[(j, i)]) if i < u else label(j, i) for i in range(n)] for j in range(len(perm))]
    zs = permutation_chain_py(columns, sigmas, k, u, sc["beta"], sc["gamma"], DELTA, cs.chunk_len)
    assert zs[-1][u] == 1
    lag["sigma"] = sigmas
    lag["perm_z"] = [z + [rnd() for _ in range(n - u - 1)] for z in zs]
    # ---- the lookup
    a_in = expressions_rows_py(cs, 1, 0, lag["advice"], lag["fixed"], lag["instance"], [], sc["theta"])
    s_in = expressions_rows_py(cs, 2, 0, lag["advice"], lag["fixed"], lag["instance"], [], sc["theta"])
    ap, sp = lookup_permute_py(a_in, s_in, u)
    ap, sp = ap + [rnd() for _ in range(n - u)], sp + [rnd() for _ in range(n - u)]
    z = lookup_product_py(a_in, s_in, ap, sp, u, sc["beta"], sc["gamma"])
    assert z[u] == 1
    lag["lookup_z"], lag["lookup_ap"], lag["lookup_sp"] = [z + [rnd() for _ in range(n - u - 1)]], [ap], [sp]
    polys = {kind: [ntt(col, k, inverse=True) for col in lag[kind]] for kind in POLY_KINDS}
    return cs, lag, polys, sc
