"""Shared helpers for the tests (checker side: uses the oracle)."""
from oracle import bn254 as O, cref
from oracle import schema as S

G_BYTES = O.aff_to_bytes(O.G1)


def fr_bytes(xs):
    return b"".join(O.fe_to_bytes(x % O.R) for x in xs)


def rand_frs(rng, n):
    return [rng.fr() for _ in range(n)]


def points_from_scalars(ks):
    """affine bytes of k_i * G via the C oracle"""
    n = len(ks)
    if n == 0:
        return b""
    return cref.g1_batch_to_affine(cref.g1_batch_scalar_mul(G_BYTES * n, fr_bytes(ks), n), n)


def to_jac_bytes(aff_bytes, zs):
    out = b""
    for i, z in enumerate(zs):
        out += O.jac_to_bytes(O.aff_from_bytes(aff_bytes[64 * i:64 * i + 64]), z)
    return out


def norm(eng_or_none, jac):
    """normalise Jacobian bytes with the ORACLE (checker-side normalisation)"""
    return cref.g1_batch_to_affine(jac, len(jac) // 96)


def bases_from_coefficients(gs):
    """affine bytes of g_i * G for integer coefficients g_i (0 mod r: the identity, 64 zero bytes), each distinct value
    multiplied once by the C oracle: dependent bases (small multiples of one point) cost a handful of scalar multiplications"""
    distinct = sorted({g % O.R for g in gs} - {0})
    pts = points_from_scalars(distinct)
    table = {g: pts[64 * i:64 * i + 64] for i, g in enumerate(distinct)}
    table[0] = bytes(64)
    return b"".join(table[g % O.R] for g in gs)


def msm_want(gs, ss):
    """canonical affine bytes of sum_i s_i * (g_i * G) = ((sum_i g_i s_i) mod r) * G: Python integers and one scalar
    multiplication by the oracle"""
    return O.aff_to_bytes(O.scalar_mul(sum(g * s for g, s in zip(gs, ss)) % O.R, O.G1))


class CEccChip(S.OracleEccChip):
    """MockEccChip with multi_exp = oracle_multi_exp_naive (the reference's loop, mock/arith/ecc.rs:106-129, in C)"""

    def multi_exp(self, ctx, points, scalars):
        ctx.point_list = [O.debug_fmt(p) for p in points]
        n = len(points)
        out = cref.multi_exp_naive(b"".join(O.aff_to_bytes(p) for p in points),
                                   b"".join(O.fe_to_bytes(s) for s in scalars), n)
        return O.aff_from_bytes(out)
