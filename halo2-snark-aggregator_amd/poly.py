"""EvaluationDomain's conversions over the engine's Fr transform (h2agg_fr_fft), the two ways to commit to a polynomial, and
the ways to open one: eval_polynomial, kate_division and the GWC multiopen prover (h2agg_fr_poly_* / h2agg_kzg_multiopen),
the Shplonk multiopen prover and its verifier's pair (h2agg_kzg_shplonk_begin / _finish; shplonk_final_pair);
and the grand products of the permutation and lookup arguments (h2agg_fr_batch_invert, h2agg_permutation_product,
h2agg_lookup_product); and the lookup argument in front of its product (h2agg_fr_columns_compress, h2agg_lookup_permute);
and the quotient polynomial h(X) from a verifying key (h2agg_vk_expressions_eval, h2agg_quotient); and the keys those stages
take: the permutation's mapping, sigma columns and commitments, the fixed columns' (h2agg_permutation_assembly,
h2agg_permutation_sigmas, h2agg_commit_columns); and, in front of all that work, the check whether a witness satisfies the key
at all, and where it does not (h2agg_witness_check); and, for a caller that keeps its columns on the device between those
stages, ColumnStore and the resident_* spellings of the slab helpers (h2agg_columns_*).

halo2_proofs is an unvendored git dependency of the reference: the names below are recalled from upstream
(poly/domain.rs), not pinned.  What each function computes is the definition in include/h2agg.h:
polynomials are 2^k canonical 32-byte little-endian Fr elements, coefficients low degree first, evaluations in the natural
order of the domain {w^i}.  The transform runs on the device; nothing here computes in Python but the padding."""
from __future__ import annotations

from .wire import R_MOD

# The cube root of unity halo2curves calls bn256::Fr::ZETA is the eigenvalue lambda of the GLV endomorphism
# (phi(P) = lambda * P, csrc/sort_kernels.hpp): no second literal, it comes from the reduced lattice basis the MSM's scalar
# decomposition already uses (GlvConst::A1, GlvConst::B1N: a1 + b1 * lambda = 0 mod r, b1 = -B1N).
_GLV_A1 = 0x6f4d8248eeb859fc8211bbeb7d4f1128
_GLV_B1N = 0x89d3256894d213e3
ZETA_INT = _GLV_A1 * pow(_GLV_B1N, R_MOD - 2, R_MOD) % R_MOD
assert pow(ZETA_INT, 3, R_MOD) == 1 and ZETA_INT != 1
ZETA = ZETA_INT.to_bytes(32, "little")


def _poly(data, k: int, what: str):
    if data is None or len(data) != 32 << k:
        raise ValueError("%s must be 2^%d elements of 32 bytes (got %s bytes)" % (what, k, "no" if data is None else len(data)))
    return data


def lagrange_to_coeff(eng, evals: bytes, k: int) -> bytes:
    """evaluations over {w^i} -> coefficients (the inverse transform, with its 1/n)"""
    return eng.fr_fft(_poly(evals, k, "evals"), k, inverse=True)


def coeff_to_lagrange(eng, coeffs: bytes, k: int) -> bytes:
    """coefficients -> evaluations over {w^i} (best_fft)"""
    return eng.fr_fft(_poly(coeffs, k, "coeffs"), k)


def coeff_to_extended(eng, coeffs: bytes, k: int, extended_k: int, shift: bytes = ZETA) -> bytes:
    """2^k coefficients -> evaluations over the coset {shift * w_ext^i} of the 2^extended_k domain: zero-padded, then a shifted
    forward transform (halo2 multiplies coefficient j by zeta^(j mod 3) = zeta^j first)"""
    if extended_k < k:
        raise ValueError("extended_k must be >= k")
    return eng.fr_fft(bytes(_poly(coeffs, k, "coeffs")) + bytes((32 << extended_k) - (32 << k)), extended_k, shift=shift)


def extended_to_coeff(eng, evals: bytes, extended_k: int, shift: bytes = ZETA) -> bytes:
    """evaluations over the coset {shift * w_ext^i} -> all 2^extended_k coefficients (the caller truncates to its degree)"""
    return eng.fr_fft(_poly(evals, extended_k, "evals"), extended_k, inverse=True, shift=shift)


def commit_coeff(eng, g_handle: int, coeffs: bytes) -> bytes:
    """sum_j coeffs[j] * g[j] against the monomial table (ParamsKZG.g), as a 96-byte Jacobian point"""
    return eng.g1_msm_preloaded(g_handle, coeffs)


def commit_lagrange(eng, gl_handle: int, evals: bytes) -> bytes:
    """sum_i evals[i] * g_lagrange[i] against the Lagrange table (ParamsKZG.g_lagrange): the same point as commit_coeff of
    lagrange_to_coeff(evals)"""
    return eng.g1_msm_preloaded(gl_handle, evals)


def eval_polynomial(eng, coeffs: bytes, z: bytes) -> bytes:
    """a(z) for 2^k coefficients (eval_polynomial of arithmetic.rs), 32 bytes"""
    k = (len(coeffs) // 32).bit_length() - 1
    return eng.fr_poly_eval(_poly(coeffs, k, "coeffs"), k, [(0, 0)], z)


def kate_division(eng, coeffs: bytes, z: bytes) -> bytes:
    """the quotient of a(X) by (X - z): the n - 1 coefficients halo2's kate_division returns (the engine writes n, the top
    one zero; the remainder a(z) is dropped, as halo2 drops it)"""
    k = (len(coeffs) // 32).bit_length() - 1
    quot, _ = eng.fr_poly_divide(bytes(_poly(coeffs, k, "coeffs")), k, z)
    return quot[:len(quot) - 32]


def group_queries(queries):
    """[(poly, point), ...] -> [(point, [poly, ...]), ...]: one group per distinct point, in the order the points are first
    seen, every group's polynomials in query order (multiopen.rs:31-43 with the point index in the rotation's role)"""
    groups = []
    for poly, point in queries:
        for pt, members in groups:
            if pt == point:
                members.append(poly)
                break
        else:
            groups.append((point, [poly]))
    return groups


def multiopen_prove(eng, g_handle: int, polys: bytes, k: int, queries, points: bytes, v: bytes):
    """the prover half of the GWC multiopen over a slab [npoly][2^k] of coefficients: -> (evals, groups, ws) with evals[q]
    the 32-byte value of query q, groups = group_queries(queries), ws[g] the canonical affine W of group g (64 bytes)"""
    queries = [(int(p), int(z)) for p, z in queries]
    evals = eng.fr_poly_eval(polys, k, queries, points)
    group_points, ws = eng.kzg_multiopen(g_handle, polys, k, queries, points, v)
    groups = group_queries(queries)
    if [pt for pt, _ in groups] != group_points:
        raise RuntimeError("the library grouped the queries differently from group_queries")
    return [evals[32 * q:32 * q + 32] for q in range(len(queries))], groups, ws


# ---------------------------------------------------------------------------------------------- Shplonk
def shplonk_sets(queries):
    """[(poly, point), ...] -> [(points, polys), ...], the sets of the Shplonk prover (include/h2agg.h): a polynomial's point
    set is what its queries name, a repeated pair counting once; polynomials with equal point sets share a set; sets in
    first-seen order of their first polynomial, `polys` in first-seen order of their first query, `points` in the order the
    set's first polynomial first names them"""
    order, named = [], {}
    for poly, point in queries:
        poly, point = int(poly), int(point)
        if poly not in named:
            named[poly] = []
            order.append(poly)
        if point not in named[poly]:
            named[poly].append(point)
    sets = []
    for poly in order:
        for points, polys in sets:
            if set(points) == set(named[poly]):
                polys.append(poly)
                break
        else:
            sets.append((list(named[poly]), [poly]))
    return sets


def shplonk_prove(eng, g_handle: int, polys: bytes, k: int, queries, points: bytes, y: bytes, v: bytes, squeeze_u):
    """the Shplonk multiopen prover over a slab [npoly][2^k] of coefficients: evaluates the queries, runs round 1, asks
    squeeze_u(h1) for the challenge u (the caller writes H1 to its transcript there), runs round 2.  -> (evals, h1, h2):
    evals[q] the 32-byte value of query q, h1 and h2 canonical affine points (64 bytes)"""
    queries = [(int(p), int(z)) for p, z in queries]
    evals = eng.fr_poly_eval(polys, k, queries, points)
    h1, obj = eng.kzg_shplonk_begin(g_handle, polys, k, queries, points, evals, y, v)
    try:
        h2 = eng.kzg_shplonk_finish(obj, squeeze_u(h1))
    finally:
        eng.kzg_shplonk_destroy(obj)
    return [evals[32 * q:32 * q + 32] for q in range(len(queries))], h1, h2


def _interpolate_at(zs, es, u):
    """the value at u of the polynomial of degree < len(zs) through (zs[i], es[i]): Lagrange's formula in integers mod r"""
    acc = 0
    for i, zi in enumerate(zs):
        num = den = 1
        for j, zj in enumerate(zs):
            if j != i:
                num = num * (u - zj) % R_MOD
                den = den * (zi - zj) % R_MOD
        acc = (acc + es[i] * num * pow(den, R_MOD - 2, R_MOD)) % R_MOD
    return acc


def shplonk_final_pair(eng, commits, queries, points: bytes, evals, y: bytes, v: bytes, u: bytes, h1: bytes, h2: bytes):
    """the Shplonk verifier's pair (include/h2agg.h): commits[m] the canonical affine commitment of polynomial m (64 bytes),
    evals[q] the value of query q.  The scalars in Python integers, one g1_msm over {C_m, G, H1, H2}.
    -> (left, right) as canonical affine points: accepted iff final_pair_check(left, right, s_g2, g2)."""
    queries = [(int(p), int(z)) for p, z in queries]
    num = lambda b: int.from_bytes(b, "little")
    zs = [num(points[at:at + 32]) for at in range(0, len(points), 32)]
    yi, vi, ui = num(y), num(v), num(u)
    value = {}
    for (poly, point), e in zip(queries, evals):
        value.setdefault((poly, point), num(e))
    sets = shplonk_sets(queries)
    named = []
    for _poly, point in queries:
        if point not in named:
            named.append(point)

    def vanishing(pts):
        out = 1
        for p in pts:
            out = out * (ui - zs[p]) % R_MOD
        return out

    d = [vanishing([p for p in named if p not in pts]) for pts, _polys in sets]
    if d[0] == 0:
        raise ValueError("u is a point of another set than the first (d_0 == 0)")
    d0_inv = pow(d[0], R_MOD - 2, R_MOD)
    scalar = {}                                # polynomial -> its scalar
    g_scalar, vpow = 0, 1
    for (pts, members), di in zip(sets, d):
        w = vpow * di * d0_inv % R_MOD         # v^i c_i
        for poly in members:
            scalar[poly] = w
            g_scalar = (g_scalar - w * _interpolate_at([zs[p] for p in pts], [value[(poly, p)] for p in pts], ui)) % R_MOD
            w = w * yi % R_MOD
        vpow = vpow * vi % R_MOD
    t = vanishing(named) * d0_inv % R_MOD
    members = sorted(scalar)
    gen = (1).to_bytes(32, "little") + (2).to_bytes(32, "little")   # G = g[0] of ParamsKZG: the curve's generator (1, 2)
    bases = b"".join(bytes(commits[m]) for m in members) + gen + bytes(h1) + bytes(h2)
    scalars = [scalar[m] for m in members] + [g_scalar, (-t) % R_MOD, ui]
    right = eng.g1_msm(bases, b"".join(s.to_bytes(32, "little") for s in scalars))
    return bytes(h2), eng.g1_batch_to_affine(right)


# ---------------------------------------------------------------------------------------------- grand products
def batch_invert(eng, xs: bytes) -> bytes:
    """ff::BatchInvert: the inverse of every element, zeros left alone"""
    return eng.fr_batch_invert(xs)


def _z_column(z: bytes, k: int, usable: int, blinding):
    """z[0 .. usable] -> a column of 2^k rows: the n - usable - 1 top rows from `blinding` (32 bytes each), or zero"""
    top = (1 << k) - usable - 1
    if blinding is None:
        return z + bytes(32 * top)
    if len(blinding) != 32 * top:
        raise ValueError("blinding must be %d elements of 32 bytes" % top)
    return z + bytes(blinding)


def permutation_products(eng, values, sigmas, k: int, usable: int, beta: bytes, gamma: bytes, delta: bytes, chunk_len: int,
                         blinding=None):
    """permutation::prover::commit over m columns: values and sigmas are lists of m Lagrange columns (2^k elements each).
    The columns are cut into sets of chunk_len; set s starts at the previous set's z[usable] (1 for the first) and at
    delta_first = delta^(s * chunk_len).  -> one column of 2^k rows per set.  blinding: None, or one block of
    2^k - usable - 1 elements per set for the rows above `usable`."""
    if len(values) != len(sigmas) or not values or chunk_len < 1:
        raise ValueError("values and sigmas must be the same non-zero number of columns, chunk_len >= 1")
    for col in list(values) + list(sigmas):
        _poly(col, k, "column")
    d = int.from_bytes(delta, "little")
    init = (1).to_bytes(32, "little")
    out = []
    for s, lo in enumerate(range(0, len(values), chunk_len)):
        vs, ss = values[lo:lo + chunk_len], sigmas[lo:lo + chunk_len]
        delta_first = pow(d, lo, R_MOD).to_bytes(32, "little")
        z, init = eng.permutation_product(b"".join(vs), b"".join(ss), len(vs), k, usable, beta, gamma, delta, delta_first, init)
        out.append(_z_column(z, k, usable, None if blinding is None else blinding[s]))
    return out


def lookup_product(eng, a: bytes, s: bytes, ap: bytes, sp: bytes, k: int, usable: int, beta: bytes, gamma: bytes, blinding=None):
    """lookup::prover::commit_product: the Z column of one lookup from the compressed input a, the compressed table s and
    their permuted forms (permute_expression_pair, a sort, is the caller's).  -> one column of 2^k rows."""
    z, _last = eng.lookup_product(_poly(a, k, "a"), _poly(s, k, "s"), _poly(ap, k, "ap"), _poly(sp, k, "sp"), k, usable, beta, gamma)
    return _z_column(z, k, usable, blinding)


# ---------------------------------------------------------------------------------------------- lookup argument
def compress_expressions(eng, cols, k: int, theta: bytes) -> bytes:
    """the theta-fold of lookup::prover::commit_permuted: cols is a list of m >= 1 columns (2^k elements each), the first one
    ends under the highest power of theta.  -> one column of 2^k rows."""
    if not cols:
        raise ValueError("cols must hold at least one column")
    for col in cols:
        _poly(col, k, "column")
    return eng.fr_columns_compress(b"".join(cols), len(cols), k, theta)


def permute_expression_pair(eng, a: bytes, s: bytes, k: int, usable: int, blinding=None):
    """lookup::prover::permute_expression_pair: the compressed input a and table s (2^k rows each) -> (ap, sp), columns of 2^k
    rows: ap the usable rows of a in ascending order, sp the usable rows of s rearranged so that sp[i] = ap[i] wherever
    ap[i] starts a run.  The top 2^k - usable rows come from blinding = (block for ap, block for sp), or are zero.  Raises
    H2AggError(ERR_NOT_IN_TABLE) if a usable input value is not among the usable table rows."""
    top = (1 << k) - usable
    if blinding is None:
        blinding = (bytes(32 * top), bytes(32 * top))
    if len(blinding) != 2 or any(len(b) != 32 * top for b in blinding):
        raise ValueError("blinding must be two blocks of %d elements of 32 bytes" % top)
    ap, sp = eng.lookup_permute(_poly(a, k, "a"), _poly(s, k, "s"), k, usable)
    return ap + bytes(blinding[0]), sp + bytes(blinding[1])


def lookup_argument(eng, inputs, tables, k: int, usable: int, theta: bytes, beta: bytes, gamma: bytes, blinding=None):
    """one lookup from its expressions to its Z: compress_expressions of the input and the table columns,
    permute_expression_pair, lookup_product.  blinding: None, or (block for ap, block for sp, block for z) with
    2^k - usable, 2^k - usable and 2^k - usable - 1 elements.  -> (ap, sp, z), columns of 2^k rows."""
    if blinding is not None and len(blinding) != 3:
        raise ValueError("blinding must be three blocks: ap, sp, z")
    a = compress_expressions(eng, inputs, k, theta)
    s = compress_expressions(eng, tables, k, theta)
    ap, sp = permute_expression_pair(eng, a, s, k, usable, None if blinding is None else blinding[:2])
    z = lookup_product(eng, a, s, ap, sp, k, usable, beta, gamma, None if blinding is None else blinding[2])
    return ap, sp, z


# ---------------------------------------------------------------------------------------------- lookup argument, batched
def _blocks(blinding, count: int, rows: int, what: str):
    """None, or one block of `rows` elements per lookup -> a list of `count` blocks (zero for None)"""
    if blinding is None:
        return [bytes(32 * rows)] * count
    blinding = list(blinding)
    if len(blinding) != count or any(len(b) != 32 * rows for b in blinding):
        raise ValueError("%s must be %d blocks of %d elements of 32 bytes" % (what, count, rows))
    return [bytes(b) for b in blinding]


def _filled(blocks, below: int) -> bytes:
    """a slab whose columns hold zero in the rows below `below` and their block above"""
    return b"".join(bytes(32 * below) + b for b in blocks)


def permute_expression_pairs(eng, a_cols, s_cols, k: int, usable: int, blinding=None):
    """permute_expression_pair of every lookup of a list in ONE call (h2agg_lookup_batch_permute): a_cols / s_cols are the
    compressed inputs and tables, one column of 2^k rows per lookup.  blinding: None, or (blocks for ap, blocks for sp), one
    block of 2^k - usable elements per lookup.  -> (list of ap, list of sp).  Raises the H2AggError of the lowest-numbered
    failing lookup; its .partial holds (ap slab, sp slab, status words)."""
    a_cols = list(a_cols)
    count = len(a_cols)
    a, s = _columns(a_cols, k, "a"), _slab(s_cols, count, k, "s")
    top = (1 << k) - usable
    if blinding is not None and len(blinding) != 2:
        raise ValueError("blinding must be two lists of blocks: ap, sp")
    pre = [_filled(_blocks(None if blinding is None else blinding[i], count, top, "blinding"), usable) for i in range(2)]
    ap, sp, _status = eng.lookup_batch_permute(a, s, count, k, usable, pre[0], pre[1])
    return _split(ap, k), _split(sp, k)


def lookup_products(eng, a_cols, s_cols, ap_cols, sp_cols, k: int, usable: int, beta: bytes, gamma: bytes, blinding=None):
    """lookup::prover::commit_product of every lookup of a list in ONE call (h2agg_lookup_batch_product).  blinding: None, or
    one block of 2^k - usable - 1 elements per lookup.  -> a list of Z columns of 2^k rows."""
    a_cols = list(a_cols)
    count = len(a_cols)
    slabs = [_columns(a_cols, k, "a")] + [_slab(c, count, k, w) for c, w in ((s_cols, "s"), (ap_cols, "ap"), (sp_cols, "sp"))]
    pre = _filled(_blocks(blinding, count, (1 << k) - usable - 1, "blinding"), usable + 1)
    z, _last = eng.lookup_batch_product(*slabs, count, k, usable, beta, gamma, pre)
    return _split(z, k)


def lookup_arguments(eng, inputs, tables, k: int, usable: int, theta: bytes, beta: bytes, gamma: bytes, blinding=None):
    """every lookup of a circuit from its expressions to its Z: inputs[j] / tables[j] are the expression columns of lookup j.
    One compression per expression list, then ONE permutation call and ONE product call for all lookups.  blinding: None, or
    (blocks for ap, blocks for sp, blocks for z), one block per lookup.  -> (list of ap, list of sp, list of z)."""
    if len(inputs) != len(tables) or not inputs:
        raise ValueError("inputs and tables must be the same non-zero number of lookups")
    if blinding is not None and len(blinding) != 3:
        raise ValueError("blinding must be three lists of blocks: ap, sp, z")
    a = [compress_expressions(eng, cols, k, theta) for cols in inputs]
    s = [compress_expressions(eng, cols, k, theta) for cols in tables]
    ap, sp = permute_expression_pairs(eng, a, s, k, usable, None if blinding is None else blinding[:2])
    z = lookup_products(eng, a, s, ap, sp, k, usable, beta, gamma, None if blinding is None else blinding[2])
    return ap, sp, z


# ---------------------------------------------------------------------------------------------- quotient polynomial
def _slab(cols, count: int, k: int, what: str):
    """a list of `count` columns -> one slab, or None for no columns"""
    cols = list(cols or [])
    if len(cols) != count:
        raise ValueError("%s must be %d columns (got %d)" % (what, count, len(cols)))
    for col in cols:
        _poly(col, k, what)
    return b"".join(cols) if cols else None


# ---------------------------------------------------------------------------------------------- domain conversions of a slab
def _columns(cols, k: int, what: str) -> bytes:
    """a non-empty list of 2^k-element columns -> one slab"""
    cols = list(cols or [])
    if not cols:
        raise ValueError("%s must hold at least one column" % what)
    return _slab(cols, len(cols), k, what)


def _split(slab: bytes, k: int):
    return [slab[at:at + (32 << k)] for at in range(0, len(slab), 32 << k)]


def columns_lagrange_to_coeff(eng, cols, k: int):
    """lagrange_to_coeff of every column of a list, in one call (h2agg_fr_fft_batch) -> a list of columns"""
    return _split(eng.fr_fft_batch(_columns(cols, k, "evals"), k, inverse=True), k)


def columns_coeff_to_lagrange(eng, cols, k: int):
    """coeff_to_lagrange of every column of a list, in one call -> a list of columns"""
    return _split(eng.fr_fft_batch(_columns(cols, k, "coeffs"), k), k)


def columns_coeff_to_extended(eng, cols, k: int, extended_k: int, shift: bytes = ZETA):
    """coeff_to_extended of every column of a list, in one call: every column is zero-padded to 2^extended_k -> a list of
    columns of 2^extended_k evaluations"""
    if extended_k < k:
        raise ValueError("extended_k must be >= k")
    cols = list(cols or [])
    _columns(cols, k, "coeffs")
    pad = bytes((32 << extended_k) - (32 << k))
    return _split(eng.fr_fft_batch(b"".join(bytes(c) + pad for c in cols), extended_k, shift=shift), extended_k)


def columns_extended_to_coeff(eng, cols, extended_k: int, shift: bytes = ZETA):
    """extended_to_coeff of every column of a list, in one call -> a list of columns of all 2^extended_k coefficients"""
    return _split(eng.fr_fft_batch(_columns(cols, extended_k, "evals"), extended_k, inverse=True, shift=shift), extended_k)


def _challenges(vk, challenges):
    challenges = list(challenges or [])
    if len(challenges) != vk.shape["num_challenges"] or any(len(c) != 32 for c in challenges):
        raise ValueError("challenges must be %d scalars of 32 bytes" % vk.shape["num_challenges"])
    return b"".join(challenges) if challenges else None


def expressions_eval(eng, vk, which: int, j: int, advice, fixed, instance, challenges, fold=None):
    """expressions of the key on every row of value columns (lists of 2^k-element columns per kind; challenges: a list of
    32-byte scalars).  which = 0: the gate polynomials, 1 / 2: the input / table expressions of lookup j.  fold None -> a list
    with one column per expression; fold = 32 bytes -> one column, sum_j fold^(m-1-j) E_j (fold = theta on a lookup's lists:
    the compressed columns of commit_permuted; fold = y on the gates: their share of the quotient's numerator)."""
    sh = vk.shape
    k = sh["k"]
    out = eng.vk_expressions_eval(vk, which, j, k, _slab(advice, sh["num_advice"], k, "advice"), _slab(fixed, sh["num_fixed"], k, "fixed"),
                                  _slab(instance, sh["num_instance"], k, "instance"), _challenges(vk, challenges), fold)
    return out if fold is not None else [out[at:at + (32 << k)] for at in range(0, len(out), 32 << k)]


def quotient_pieces(eng, vk, advice, fixed, instance, sigma, perm_z, lookup_z, lookup_ap, lookup_sp, challenges, theta: bytes,
                    beta: bytes, gamma: bytes, y: bytes, delta: bytes):
    """the pieces h_0 .. h_{degree-2} of the quotient polynomial (include/h2agg.h): every argument in front of `challenges`
    is a list of polynomials in coefficient form, 2^k elements each — the key's advice, fixed and instance columns, the
    permutation's sigma polynomials and the Z of its sets, and Z, a', s' of every lookup.  -> a list of degree - 1
    polynomials of 2^k coefficients."""
    sh = vk.shape
    k, chunk, nl = sh["k"], sh["degree"] - 2, len(sh["lookups"])
    nsets = (sh["num_permutation_columns"] + chunk - 1) // chunk
    out = eng.quotient(vk, _slab(advice, sh["num_advice"], k, "advice"), _slab(fixed, sh["num_fixed"], k, "fixed"),
                       _slab(instance, sh["num_instance"], k, "instance"), _slab(sigma, sh["num_permutation_columns"], k, "sigma"),
                       _slab(perm_z, nsets, k, "perm_z"), _slab(lookup_z, nl, k, "lookup_z"), _slab(lookup_ap, nl, k, "lookup_ap"),
                       _slab(lookup_sp, nl, k, "lookup_sp"), _challenges(vk, challenges), theta, beta, gamma, y, delta)
    return [out[at:at + (32 << k)] for at in range(0, len(out), 32 << k)]


def quotient_work_bytes(eng, vk) -> int:
    """the device work memory a quotient_pieces call of this key holds in the context, in bytes (include/h2agg.h)"""
    return eng.quotient_work_bytes(vk)


def commit_quotient(eng, g_handle: int, pieces):
    """the commitments of h's pieces against the monomial table (ParamsKZG.g), in order: commit_coeff of each, as 96-byte
    Jacobian points (the h commitments a proof carries, vanish.rs:18-72).  (Not the slab call: that one answers canonical
    affine points, these stay the Jacobian bytes they were.)"""
    return [commit_coeff(eng, g_handle, p) for p in pieces]


# ---------------------------------------------------------------------------------------------- witness check
WC_KINDS = ("gate", "permutation", "lookup")


class WitnessReport:
    """what h2agg_witness_check answers.  counts, first_rows: one entry per constraint (gate polynomials, then permutation
    columns, then lookups); rows: per constraint the lowest max_rows failing rows, ascending (None if none were asked for);
    total: the sum of the counts; ok: total == 0; failures: [(kind, index within the kind, row), ...] over the reported rows
    (with no rows reported: the first row of every failing constraint), in constraint order, rows ascending."""

    def __init__(self, layout, counts, first_rows, rows, total):
        self.layout, self.counts, self.first_rows, self.rows, self.total = tuple(layout), counts, first_rows, rows, total
        self.ok = total == 0
        self.failures = []
        c = 0
        for kind, count in zip(WC_KINDS, self.layout):
            for index in range(count):
                if rows is not None and rows[c]:
                    self.failures += [(kind, index, r) for r in rows[c] if r != 0xFFFFFFFF]
                elif counts[c]:
                    self.failures.append((kind, index, first_rows[c]))
                c += 1

    def __repr__(self):
        return "WitnessReport(ok=%s, total=%d, failures=%r)" % (self.ok, self.total, self.failures)


def witness_check(eng, vk, advice, fixed, instance, challenges, theta=None, mapping=None, what=None, max_rows=16):
    """dev::MockProver::verify's gate, permutation and lookup checks on the device (h2agg_witness_check): does this witness —
    lists of Lagrange columns per kind, 2^k elements each — satisfy the key, and if not, which constraint fails on which
    rows?  mapping: the permutation's mapping (permutation_mapping), theta: the lookups' compression challenge.  what: a
    set of WC_* bits of the package; None: every kind the arguments allow (the permutation needs mapping, the lookups
    theta).  -> a WitnessReport."""
    from . import WC_GATES, WC_LOOKUPS, WC_PERMUTATION
    sh = vk.shape
    k = sh["k"]
    if what is None:
        what = WC_GATES | (WC_PERMUTATION if mapping is not None else 0) | (WC_LOOKUPS if theta is not None else 0)
    counts, first_rows, rows, total = eng.witness_check(
        vk, what, _slab(advice, sh["num_advice"], k, "advice"), _slab(fixed, sh["num_fixed"], k, "fixed"),
        _slab(instance, sh["num_instance"], k, "instance"), _challenges(vk, challenges), theta, mapping, max_rows, max_rows > 0)
    return WitnessReport(eng.witness_check_layout(vk), counts, first_rows, rows, total)


# ---------------------------------------------------------------------------------------------- keys
def commit_columns_lagrange(eng, gl_handle: int, cols, k: int):
    """commit_lagrange of every column of a list in one call (h2agg_commit_columns against ParamsKZG.g_lagrange) -> a list of
    canonical affine points, 64 bytes each, the identity as 64 zero bytes"""
    return eng.commit_columns(gl_handle, _columns(cols, k, "evals"), k)


def commit_columns_coeff(eng, g_handle: int, cols, k: int):
    """commit_coeff of every column of a list in one call (h2agg_commit_columns against ParamsKZG.g) -> affine points"""
    return eng.commit_columns(g_handle, _columns(cols, k, "coeffs"), k)


def permutation_mapping(m: int, k: int, usable: int, copies) -> bytes:
    """permutation::keygen::Assembly: the copy constraints [(left column, left row, right column, right row), ...] over m
    columns of 2^k rows, in order -> the mapping (h2agg_permutation_assembly), 2 * m * 2^k uint32 words"""
    from . import permutation_assembly
    return permutation_assembly(m, k, usable, copies)


def permutation_key(eng, gl_handle: int, mapping, m: int, k: int, usable: int, delta: bytes):
    """the permutation's share of keygen_vk / keygen_pk from its mapping: -> (lagrange, coeff, commitments) — the sigma columns
    in Lagrange form (what permutation_products takes), in coefficient form (what quotient_pieces takes), m columns each,
    and their commitments against g_lagrange as affine points (the permutation commitments of a verifying key)"""
    lag, coeff = eng.permutation_sigmas(mapping, m, k, usable, delta)
    return _split(lag, k), _split(coeff, k), eng.commit_columns(gl_handle, lag, k)


def fixed_key(eng, gl_handle: int, fixed_cols, k: int):
    """the fixed columns' share of keygen: Lagrange columns -> (coeff, commitments): columns_lagrange_to_coeff of them and
    their commitments against g_lagrange as affine points (the fixed commitments of a verifying key)"""
    return columns_lagrange_to_coeff(eng, fixed_cols, k), commit_columns_lagrange(eng, gl_handle, fixed_cols, k)


# ---------------------------------------------------------------------------------------------- columns that stay on the device
class ColumnView:
    """columns first .. first + count - 1 of a ColumnStore: what the resident helpers below take and answer.  The range is
    checked here, in the store's own column numbers; view() of a view counts from the view's first column."""

    def __init__(self, store, first: int, count: int):
        first, count = int(first), int(count)
        if count < 1 or first < 0 or first + count > store.m:
            raise ValueError("columns %d .. %d are outside a store of %d columns (or count < 1)" % (first, first + count - 1, store.m))
        self.store, self.first, self.count = store, first, count

    k = property(lambda self: self.store.k)
    handle = property(lambda self: self.store.handle)

    def view(self, first: int, count: int) -> "ColumnView":
        if count < 1 or first < 0 or first + count > self.count:
            raise ValueError("columns %d .. %d are outside a view of %d columns (or count < 1)" % (first, first + count - 1, self.count))
        return ColumnView(self.store, self.first + first, count)

    def overlaps(self, other: "ColumnView") -> bool:
        """one store and at least one column in common"""
        return (self.store.handle == other.store.handle and self.first < other.first + other.count
                and other.first < self.first + self.count)

    def same(self, other: "ColumnView") -> bool:
        return self.store.handle == other.store.handle and (self.first, self.count) == (other.first, other.count)

    def write(self, cols):
        self.store.write(self.first, cols, self.count)

    def read(self):
        return self.store.read(self.first, self.count)

    def ptr(self, column: int = 0) -> int:
        if not 0 <= column < self.count:
            raise ValueError("column %d is outside a view of %d columns" % (column, self.count))
        return self.store.ptr(self.first + column)


class ColumnStore:
    """A slab [m][2^k] of Fr in device memory that the engine's context owns (h2agg_columns_create): a context manager, freed
    on exit or by close().  handle=...: wraps a store that somebody else made and frees (nothing is called)."""

    def __init__(self, eng, m: int, k: int, handle=None):
        self.eng, self.m, self.k = eng, int(m), int(k)
        self.owned = handle is None
        self.handle = eng.columns_create(m, k) if handle is None else int(handle)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self.owned and self.handle:
            self.eng.columns_destroy(self.handle)
        self.handle = 0

    def view(self, first: int = 0, count=None) -> ColumnView:
        return ColumnView(self, first, self.m - first if count is None else count)

    def write(self, first: int, cols, count=None):
        """cols: a slab of whole columns, or a list of columns"""
        data = cols if isinstance(cols, (bytes, bytearray, memoryview)) else b"".join(_poly(c, self.k, "column") for c in cols)
        if len(data) % (32 << self.k) or not data or (count is not None and len(data) != (32 << self.k) * count):
            raise ValueError("cols must be %s whole columns of 2^%d elements" % ("some" if count is None else count, self.k))
        ColumnView(self, first, len(data) // (32 << self.k))
        self.eng.columns_write(self.handle, first, data)

    def read(self, first: int = 0, count=None):
        """-> a list of columns"""
        v = self.view(first, count)
        return _split(self.eng.columns_read(self.handle, v.first, v.count), self.k)

    def ptr(self, first: int = 0) -> int:
        ColumnView(self, first, 1)
        return self.eng.columns_ptr(self.handle, first)


def _resident_fft(eng, src: ColumnView, dst, inverse: bool, shift):
    dst = src if dst is None else dst
    if dst.count != src.count or dst.k != src.k:
        raise ValueError("source and destination must be as many columns of one k")
    if src.overlaps(dst) and not src.same(dst):
        raise ValueError("source and destination overlap (in place is the same range)")
    eng.columns_fft(src.handle, src.first, dst.handle, dst.first, src.count, inverse, shift)
    return dst


def resident_lagrange_to_coeff(eng, src: ColumnView, dst: ColumnView = None) -> ColumnView:
    """columns_lagrange_to_coeff over a store's columns (h2agg_columns_fft, queued): into dst, or in place -> the view that
    holds the result"""
    return _resident_fft(eng, src, dst, True, None)


def resident_coeff_to_lagrange(eng, src: ColumnView, dst: ColumnView = None) -> ColumnView:
    """columns_coeff_to_lagrange over a store's columns"""
    return _resident_fft(eng, src, dst, False, None)


def resident_extended_to_coeff(eng, src: ColumnView, dst: ColumnView = None, shift: bytes = ZETA) -> ColumnView:
    """columns_extended_to_coeff over the columns of a store of 2^extended_k rows"""
    return _resident_fft(eng, src, dst, True, shift)


def resident_extended_from_padded(eng, src: ColumnView, dst: ColumnView = None, shift: bytes = ZETA) -> ColumnView:
    """the transform of columns_coeff_to_extended over columns of a store of 2^extended_k rows that already hold the
    coefficients zero-padded (a new store is zero-filled: write the 2^k coefficients of a column in front)"""
    return _resident_fft(eng, src, dst, False, shift)


def resident_commit_columns_lagrange(eng, gl_handle: int, cols: ColumnView):
    """commit_columns_lagrange of a store's columns (h2agg_columns_commit) -> affine points, 64 bytes each"""
    return eng.columns_commit(gl_handle, cols.handle, cols.first, cols.count)


def resident_commit_columns_coeff(eng, g_handle: int, cols: ColumnView):
    """commit_columns_coeff of a store's columns"""
    return eng.columns_commit(g_handle, cols.handle, cols.first, cols.count)


def resident_permutation_key(eng, gl_handle: int, mapping, m: int, k: int, usable: int, delta: bytes):
    """permutation_key with the sigma columns left on the device: -> (lagrange, coeff, commitments), two new ColumnStores of
    m columns (the caller closes them) and the commitments against g_lagrange"""
    lag, coeff = ColumnStore(eng, m, k), None
    try:
        coeff = ColumnStore(eng, m, k)
        eng.columns_sigmas(mapping, m, k, usable, delta, lag.handle, 0, coeff.handle, 0)
        return lag, coeff, eng.columns_commit(gl_handle, lag.handle, 0, m)
    except Exception:
        lag.close()
        if coeff is not None:
            coeff.close()
        raise


def _key_place(view, count: int, k: int, what: str):
    if count == 0:
        return None
    if view is None or view.count != count or view.k != k:
        raise ValueError("%s must be a view of %d columns of 2^%d rows" % (what, count, k))
    return (view.handle, view.first)


def resident_witness_check(eng, vk, advice, fixed, instance, challenges, theta=None, mapping=None, what=None, max_rows=16):
    """witness_check over views of stores (None where the key has no column of the kind) -> a WitnessReport"""
    from . import WC_GATES, WC_LOOKUPS, WC_PERMUTATION
    sh = vk.shape
    k = sh["k"]
    if what is None:
        what = WC_GATES | (WC_PERMUTATION if mapping is not None else 0) | (WC_LOOKUPS if theta is not None else 0)
    counts, first_rows, rows, total = eng.columns_witness_check(
        vk, what, _key_place(advice, sh["num_advice"], k, "advice"), _key_place(fixed, sh["num_fixed"], k, "fixed"),
        _key_place(instance, sh["num_instance"], k, "instance"), _challenges(vk, challenges), theta, mapping, max_rows, max_rows > 0)
    return WitnessReport(eng.witness_check_layout(vk), counts, first_rows, rows, total)


def resident_shplonk_prove(eng, g_handle: int, polys: ColumnView, queries, points: bytes, y: bytes, v: bytes, squeeze_u):
    """shplonk_prove over a store's columns (coefficient form): the values through h2agg_fr_poly_eval_device over the store's
    pointer, the two rounds through h2agg_columns_shplonk_begin and the existing finish -> (evals, h1, h2)"""
    queries = [(int(p), int(z)) for p, z in queries]
    evals = eng.fr_poly_eval_device(polys.ptr(), polys.count, polys.k, queries, points)
    h1, obj = eng.columns_shplonk_begin(g_handle, polys.handle, polys.first, polys.count, queries, points, evals, y, v)
    try:
        h2 = eng.kzg_shplonk_finish(obj, squeeze_u(h1))
    finally:
        eng.kzg_shplonk_destroy(obj)
    return [evals[32 * q:32 * q + 32] for q in range(len(queries))], h1, h2


# ---------------------------------------------------------------------------------------------- proving key on the device
def pk_bytes(eng, vk, cosets: bool = True) -> int:
    """the device memory a ProvingKey of this verifying key holds, in bytes (include/h2agg.h)"""
    from . import PK_COSETS
    return eng.pk_bytes(vk, PK_COSETS if cosets else 0)


class ProvingKey:
    """What a prover of one circuit keeps on the device between proofs (h2agg_pk_create): the fixed and sigma columns in Lagrange
    and coefficient form, l_0 / l_last / l_blind, and with cosets=True their values on every coset of the extended domain, so
    that the quotient transforms the witness alone.  A context manager, freed on exit or by close(); the verifying key and
    the engine must outlive it."""

    def __init__(self, eng, vk, handle):
        self.eng, self.vk, self._pk = eng, vk, handle
        self.info = eng.pk_info(handle)

    @classmethod
    def from_lagrange(cls, eng, vk, fixed_cols, sigma_cols, cosets: bool = True) -> "ProvingKey":
        """fixed_cols / sigma_cols: lists of 2^k-element columns in Lagrange form (sigma_cols: permutation_key's first result)"""
        from . import PK_COSETS
        sh = vk.shape
        k = sh["k"]
        return cls(eng, vk, eng.pk_create(vk, _slab(fixed_cols, sh["num_fixed"], k, "fixed"),
                                          _slab(sigma_cols, sh["num_permutation_columns"], k, "sigma"), PK_COSETS if cosets else 0))

    @classmethod
    def from_views(cls, eng, vk, fixed: ColumnView, sigma: ColumnView, cosets: bool = True) -> "ProvingKey":
        """the same from views of stores that hold the Lagrange columns (None where the key has no column of the kind); the
        stores are not written and may go once this returns"""
        from . import PK_COSETS
        sh = vk.shape
        ptrs = [_key_view(v, count, sh["k"], what) for v, count, what in ((fixed, sh["num_fixed"], "fixed"),
                                                                          (sigma, sh["num_permutation_columns"], "sigma"))]
        return cls(eng, vk, eng.pk_create_resident(vk, *ptrs, PK_COSETS if cosets else 0))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self._pk:
            self.eng.pk_destroy(self._pk)

    handle = property(lambda self: self._pk)
    cosets = property(lambda self: bool(self.info["forms"] & 1))

    def ptr(self, which: int, coset: int = 0):
        """-> (device address or None, columns) of one form (PK_FIXED_LAGRANGE .. PK_COSET of the package)"""
        return self.eng.pk_ptr(self._pk, which, coset)

    def work_bytes(self) -> int:
        return self.eng.pk_quotient_work_bytes(self._pk)

    def _witness_counts(self):
        sh = self.vk.shape
        chunk, nl = sh["degree"] - 2, len(sh["lookups"])
        nsets = (sh["num_permutation_columns"] + chunk - 1) // chunk
        return (("advice", sh["num_advice"]), ("instance", sh["num_instance"]), ("perm_z", nsets), ("lookup_z", nl),
                ("lookup_ap", nl), ("lookup_sp", nl))

    def resident_quotient(self, advice, instance, perm_z, lookup_z, lookup_ap, lookup_sp, challenges, theta: bytes, beta: bytes,
                          gamma: bytes, y: bytes, delta: bytes, out: ColumnView) -> ColumnView:
        """h2agg_pk_quotient over views of stores that hold the witness polynomials in coefficient form (None where the key has
        none of the kind): the degree - 1 pieces into `out`, queued on the context's stream -> out"""
        sh = self.vk.shape
        k = sh["k"]
        views = (advice, instance, perm_z, lookup_z, lookup_ap, lookup_sp)
        ptrs = [_key_view(v, count, k, what) for v, (what, count) in zip(views, self._witness_counts())]
        if out is None or out.count != sh["degree"] - 1 or out.k != k:
            raise ValueError("out must be a view of %d columns of 2^%d rows" % (sh["degree"] - 1, k))
        if any(v is not None and count and out.overlaps(v) for v, (_w, count) in zip(views, self._witness_counts())):
            raise ValueError("out overlaps an input")
        self.eng.pk_quotient(self._pk, *ptrs, _challenges(self.vk, challenges), theta, beta, gamma, y, delta, out.ptr())
        return out

    def quotient_pieces(self, advice, instance, perm_z, lookup_z, lookup_ap, lookup_sp, challenges, theta: bytes, beta: bytes,
                        gamma: bytes, y: bytes, delta: bytes):
        """quotient_pieces with the key's polynomials taken from this object: lists of witness polynomials in coefficient form
        on the host -> the list of degree - 1 pieces.  Staged through a store that lives for the call."""
        sh = self.vk.shape
        k, pieces = sh["k"], sh["degree"] - 1
        lists = (advice, instance, perm_z, lookup_z, lookup_ap, lookup_sp)
        slabs = [_slab(cols, count, k, what) for cols, (what, count) in zip(lists, self._witness_counts())]
        total = sum(count for _w, count in self._witness_counts())
        with ColumnStore(self.eng, total + pieces, k) as store:
            views, at = [], 0
            for slab, (_what, count) in zip(slabs, self._witness_counts()):
                views.append(store.view(at, count) if count else None)
                if count:
                    store.write(at, slab, count)
                at += count
            out = self.resident_quotient(*views, challenges, theta, beta, gamma, y, delta, store.view(total, pieces))
            return out.read()


def _key_view(view, count: int, k: int, what: str):
    """the device address of a view that must hold `count` columns of 2^k rows; None where the key has none of the kind"""
    if count == 0:
        return None
    if view is None or view.count != count or view.k != k:
        raise ValueError("%s must be a view of %d columns of 2^%d rows" % (what, count, k))
    return view.ptr()


def _same_shape(views, what: str):
    first = views[0]
    if any(v.count != first.count or v.k != first.k for v in views):
        raise ValueError("%s must be as many columns of one k" % what)


def resident_lookup_permute(eng, a: ColumnView, s: ColumnView, usable: int, ap: ColumnView, sp: ColumnView, status: bool = True):
    """permute_expression_pairs over views of stores (h2agg_lookup_store_permute): column j of a and s -> rows below `usable`
    of column j of ap and sp; the rows above stay what the stores hold.  status=True: synchronous -> the per-lookup status
    words (an error carries them in .partial); False: queued on the context's stream -> None"""
    _same_shape((a, s, ap, sp), "a, s, ap, sp")
    return eng.lookup_store_permute(a.handle, a.first, s.handle, s.first, a.count, usable, ap.handle, ap.first, sp.handle, sp.first,
                                    status)


def resident_lookup_product(eng, a: ColumnView, s: ColumnView, ap: ColumnView, sp: ColumnView, usable: int, beta: bytes,
                            gamma: bytes, z: ColumnView, last: bool = True):
    """lookup_products over views of stores (h2agg_lookup_store_product): rows 0 .. usable of column j of z.  last=True:
    synchronous -> the list of z[j][usable]; False: queued on the context's stream -> None"""
    _same_shape((a, s, ap, sp, z), "a, s, ap, sp, z")
    return eng.lookup_store_product(a.handle, a.first, s.handle, s.first, ap.handle, ap.first, sp.handle, sp.first, a.count, usable,
                                    beta, gamma, z.handle, z.first, last)
