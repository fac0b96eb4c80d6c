"""The definitions of include/h2agg.h's grand-product block restated with Python integers (one pow(x, R - 2, R) per
element, no batching), and the constructions the tests feed them: a permutation argument that is satisfied, a lookup's
permuted pair.  tests/test_grand_product_host.py ties the restatements to the identities the reference's verifier checks
(permutation.rs:70-133, lookup.rs:98-113); tests/test_gpu_grand_product.py compares the library with them byte for byte."""
import random

from oracle import bn254 as O
from oracle import verifier as V

R = O.R
DELTA = V.FR_DELTA
BIG = (1 << 253) + 0x1234567   # a 254-bit value below r
assert BIG < R and BIG.bit_length() == 254


def omega(k):
    return V.omega_for_k(k) if k else 1


def inv0(x):
    """inv(0) = 0, as ff::BatchInvert leaves zeros alone"""
    return pow(x, R - 2, R) if x % R else 0


def batch_invert_py(xs):
    return [inv0(x) for x in xs]


def grand_product_py(num, den, u, init):
    """out[0] = init, out[i + 1] = out[i] * num[i] * inv(den[i]), i < u; den None: no denominator.  -> u + 1 values"""
    out = [init % R]
    for i in range(u):
        out.append(out[-1] * num[i] % R * (inv0(den[i]) if den is not None else 1) % R)
    return out


def permutation_terms_py(values, sigmas, k, u, beta, gamma, delta, delta_first):
    w = omega(k)
    num, den = [], []
    for i in range(u):
        a = b = 1
        dj, wi = delta_first, pow(w, i, R)
        for col, sig in zip(values, sigmas):
            a = a * ((col[i] + beta * dj % R * wi + gamma) % R) % R
            b = b * ((col[i] + beta * sig[i] + gamma) % R) % R
            dj = dj * delta % R
        num.append(a)
        den.append(b)
    return num, den


def permutation_product_py(values, sigmas, k, u, beta, gamma, delta, delta_first, init):
    num, den = permutation_terms_py(values, sigmas, k, u, beta, gamma, delta, delta_first)
    return grand_product_py(num, den, u, init)


def permutation_chain_py(values, sigmas, k, u, beta, gamma, delta, chunk_len):
    """the sets of chunk_len columns chained as the prover chains them -> [z_0[0 .. u], z_1[0 .. u], ...]"""
    zs, init = [], 1
    for lo in range(0, len(values), chunk_len):
        z = permutation_product_py(values[lo:lo + chunk_len], sigmas[lo:lo + chunk_len], k, u, beta, gamma, delta,
                                   pow(delta, lo, R), init)
        zs.append(z)
        init = z[u]
    return zs


def lookup_product_py(a, s, ap, sp, u, beta, gamma):
    num = [(a[i] + beta) * (s[i] + gamma) % R for i in range(u)]
    den = [(ap[i] + beta) * (sp[i] + gamma) % R for i in range(u)]
    return grand_product_py(num, den, u, 1)


def satisfied_permutation(seed, k, m, u, delta=DELTA):
    """m columns of 2^k rows whose values are constant on the cycles of a random permutation of the usable cells (rows < u),
    and the sigma columns of that permutation: sigma[j][i] = delta^j' w^i' for the cell (j', i') that (j, i) maps to; the
    identity delta^j w^i on the rows from u up.  -> (values, sigmas)"""
    rng = random.Random(seed)
    n, w = 1 << k, omega(k)
    cells = [(j, i) for j in range(m) for i in range(u)]
    image = cells[:]
    rng.shuffle(image)
    to = dict(zip(cells, image))
    values = [[rng.randrange(R) for _ in range(n)] for _ in range(m)]
    seen = set()
    for cell in cells:
        if cell in seen:
            continue
        v, cur = rng.randrange(R), cell
        while cur not in seen:
            seen.add(cur)
            values[cur[0]][cur[1]] = v
            cur = to[cur]
    label = lambda j, i: pow(delta, j, R) * pow(w, i, R) % R
    sigmas = [[label(*to[(j, i)]) if i < u else label(j, i) for i in range(n)] for j in range(m)]
    return values, sigmas


def permuted_pair(seed, k, u):
    """a lookup that holds on the rows < u: input a (every value taken from the table), table s, and permute_expression_pair's
    output: ap = a sorted, sp = s rearranged so that sp[i] = ap[i] wherever ap[i] starts a run.  -> (a, s, ap, sp), 2^k rows"""
    rng = random.Random(seed)
    n = 1 << k
    s = [rng.randrange(R) for _ in range(n)]
    if u > 2:
        s[1] = s[0]                                   # a repeated table value
    a = [s[rng.randrange(max(u, 1))] for _ in range(n)]
    ap, sp = sorted(a[:u]), [None] * u
    left = list(s[:u])
    for i in range(u):
        if i == 0 or ap[i] != ap[i - 1]:
            sp[i] = ap[i]
            left.remove(ap[i])
    for i in range(u):
        if sp[i] is None:
            sp[i] = left.pop()
    assert not left and sorted(sp) == sorted(s[:u])
    pad = [rng.randrange(R) for _ in range(n - u)]
    return a, s, ap + pad, sp + pad
