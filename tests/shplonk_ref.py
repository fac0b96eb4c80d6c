"""The yardstick of the Shplonk tests in Python integers over oracle.bn254's modulus (no device, no library): the definition
of include/h2agg.h, step by step — the sets, the interpolation r_{i,j}, N_i, its division by Z_{S_i} as |S_i| successive
synthetic divisions, h, L, h2, and the verifier's scalars.  tests/test_shplonk_host.py ties the pieces to one another;
tests/test_gpu_shplonk.py compares the device with them."""
from oracle import bn254 as O

R = O.R


def inv(x):
    return O.inv(x % R, R)


def horner(a, z):
    v = 0
    for c in reversed(a):
        v = (v * z + c) % R
    return v


def sets_of(queries):
    """the definition, literally: the point set of every polynomial; equal sets grouped; first-seen orders.
    -> [(points, polys), ...], points in the order the set's first polynomial first names them"""
    first_seen = []
    for poly, _pt in queries:
        if poly not in first_seen:
            first_seen.append(poly)
    point_set = {m: [] for m in first_seen}
    for poly, pt in queries:
        if pt not in point_set[poly]:
            point_set[poly].append(pt)
    out = []
    for m in first_seen:
        mine = frozenset(point_set[m])
        hit = [s for s in out if frozenset(s[0]) == mine]
        if hit:
            hit[0][1].append(m)
        else:
            out.append((point_set[m], [m]))
    return out


def named_points(queries):
    t = []
    for _poly, pt in queries:
        if pt not in t:
            t.append(pt)
    return t


def poly_mul_linear(a, z):
    """a(X) (X - z)"""
    out = [0] * (len(a) + 1)
    for i, c in enumerate(a):
        out[i + 1] = (out[i + 1] + c) % R
        out[i] = (out[i] - z * c) % R
    return out


def vanishing(zs):
    """Z_S(X), low degree first"""
    a = [1]
    for z in zs:
        a = poly_mul_linear(a, z)
    return a


def interpolate(zs, es):
    """the polynomial of degree < len(zs) through (zs[i], es[i]), low degree first: sum_i es[i] prod_{j != i} (X - z_j) / (z_i - z_j)"""
    out = [0] * len(zs)
    for i, zi in enumerate(zs):
        basis, den = [1], 1
        for j, zj in enumerate(zs):
            if j != i:
                basis = poly_mul_linear(basis, zj)
                den = den * (zi - zj) % R
        f = es[i] * inv(den) % R
        for d, c in enumerate(basis):
            out[d] = (out[d] + f * c) % R
    return out


def divide_linear(a, z):
    """(quotient with a zero on top, remainder) of a(X) by (X - z): synthetic division"""
    n = len(a)
    q = [0] * n
    for j in range(n - 1, 0, -1):
        q[j - 1] = (a[j] + z * q[j]) % R
    return q, (a[0] + z * q[0]) % R


def divide_by_roots(a, zs):
    """a / Z_S by |S| successive synthetic divisions; every remainder must be 0"""
    for z in zs:
        a, rem = divide_linear(a, z)
        assert rem == 0, "the numerator does not vanish at a point of its set"
    return a


def partial_fraction_quotient(a, zs):
    """sum_{z in S} omega_z quot(a, z), omega_z = 1 / prod_{z' != z} (z - z'): equals a / Z_S when a vanishes on S"""
    out = [0] * len(a)
    for z in zs:
        den = 1
        for z2 in zs:
            if z2 != z:
                den = den * (z - z2) % R
        w = inv(den)
        q, _rem = divide_linear(a, z)
        out = [(o + w * c) % R for o, c in zip(out, q)]
    return out


class Opening:
    """everything the definition names, for polynomials `polys` (lists of n integers), point values `zs` and the queries"""

    def __init__(self, polys, zs, queries, y, v, evals=None):
        self.polys, self.zs, self.queries, self.y, self.v = polys, zs, list(queries), y % R, v % R
        self.n = len(polys[0])
        self.sets = sets_of(self.queries)
        self.T = named_points(self.queries)
        self.evals = list(evals) if evals is not None else [horner(polys[m], zs[p]) for m, p in self.queries]
        value = {}
        for (m, p), e in zip(self.queries, self.evals):
            value.setdefault((m, p), e)
        self.value = value
        # r_{i,j}
        self.r = [[interpolate([zs[p] for p in pts], [value[(m, p)] for p in pts]) for m in members] for pts, members in self.sets]

    def numerator(self, i):
        """N_i = sum_j y^j (p_{i,j} - r_{i,j})"""
        out, yj = [0] * self.n, 1
        for j, m in enumerate(self.sets[i][1]):
            assert len(self.r[i][j]) <= self.n, "a set with more points than coefficients"
            r = self.r[i][j] + [0] * (self.n - len(self.r[i][j]))
            out = [(o + yj * (c - rc)) % R for o, c, rc in zip(out, self.polys[m], r)]
            yj = yj * self.y % R
        return out

    def h(self, divide=divide_by_roots):
        out, vi = [0] * self.n, 1
        for i, (pts, _members) in enumerate(self.sets):
            q = divide(self.numerator(i), [self.zs[p] for p in pts])
            out = [(o + vi * c) % R for o, c in zip(out, q)]
            vi = vi * self.v % R
        return out

    def z_at(self, pts, u):
        out = 1
        for p in pts:
            out = out * (u - self.zs[p]) % R
        return out

    def scalars(self, u):
        """d_i, c_i and t at u; None if d_0 == 0"""
        d = [self.z_at([p for p in self.T if p not in pts], u) for pts, _m in self.sets]
        if d[0] == 0:
            return None
        d0_inv = inv(d[0])
        return d, [di * d0_inv % R for di in d], self.z_at(self.T, u) * d0_inv % R

    def L(self, u):
        _d, c, t = self.scalars(u)
        out, vi = [0] * self.n, 1
        for i, (_pts, members) in enumerate(self.sets):
            w = vi * c[i] % R
            for j, m in enumerate(members):
                out = [(o + w * x) % R for o, x in zip(out, self.polys[m])]
                out[0] = (out[0] - w * horner(self.r[i][j], u)) % R
                w = w * self.y % R
            vi = vi * self.v % R
        return [(o - t * x) % R for o, x in zip(out, self.h())]

    def h2(self, u):
        q, rem = divide_linear(self.L(u), u)
        return q, rem

    def verifier_f(self, u, commit, h1, evals=None, y=None, v=None, c=None, t=None):
        """F = sum_i v^i c_i sum_j y^j (C_{i,j} - r_{i,j}(u) G) - t H1 in the exponent: commit[m] and h1 are discrete logarithms
        to the base G.  The keyword arguments replace what a verifier would compute (for the tests that break it)."""
        y = self.y if y is None else y
        v = self.v if v is None else v
        if evals is None:
            r = self.r
        else:
            value = {}
            for (m, p), e in zip(self.queries, evals):
                value.setdefault((m, p), e)
            r = [[interpolate([self.zs[p] for p in pts], [value[(m, p)] for p in pts]) for m in members] for pts, members in self.sets]
        _d, c0, t0 = self.scalars(u)
        c = c0 if c is None else c
        t = t0 if t is None else t
        f, vi = 0, 1
        for i, (_pts, members) in enumerate(self.sets):
            w = vi * c[i] % R
            for j, m in enumerate(members):
                f = (f + w * (commit[m] - horner(r[i][j], u))) % R
                w = w * y % R
            vi = vi * v % R
        return (f - t * h1) % R
