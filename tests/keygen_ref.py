"""The definitions of include/h2agg.h's keys block restated with Python integers, and the constructions the tests feed them.
assembly_py is halo2's permutation::keygen::Assembly (new, then copy on every constraint in order) written out from the
header's description; sigmas_py is sigma[j][i] = delta^c w^r with running products of w and delta (no pow per cell);
is_valid_mapping is the header's definition of a valid mapping.  Mappings are lists of (column, row), cell (j, i) at index
j * n + i; mapping_words / words_mapping convert to and from the 2 * m * n uint32 words of the C ABI."""
import struct

from oracle import bn254 as O
from oracle import verifier as V

R = O.R
DELTA = V.FR_DELTA


def omega(k):
    return V.omega_for_k(k) if k else 1


def mapping_words(mapping) -> bytes:
    return struct.pack("<%dI" % (2 * len(mapping)), *[x for cell in mapping for x in cell])


def words_mapping(words: bytes):
    flat = struct.unpack("<%dI" % (len(words) // 4), words)
    return list(zip(flat[0::2], flat[1::2]))


def identity_mapping(m, k):
    return [(j, i) for j in range(m) for i in range(1 << k)]


def assembly_py(m, k, usable, copies):
    """copies: (left column, left row, right column, right row), in order -> the mapping"""
    n = 1 << k
    cells = m * n
    mapping, aux, sizes = list(range(cells)), list(range(cells)), [1] * cells
    for lc, lr, rc, rr in copies:
        assert lc < m and rc < m and lr < usable and rr < usable
        left, right = lc * n + lr, rc * n + rr
        left_cycle, right_cycle = aux[left], aux[right]
        if left_cycle == right_cycle:
            continue
        if sizes[left_cycle] < sizes[right_cycle]:
            left_cycle, right_cycle = right_cycle, left_cycle
        sizes[left_cycle] += sizes[right_cycle]
        x = right_cycle
        while True:
            aux[x] = left_cycle
            x = mapping[x]
            if x == right_cycle:
                break
        mapping[left], mapping[right] = mapping[right], mapping[left]
    return [(x // n, x % n) for x in mapping]


def sigmas_py(mapping, m, k, delta=DELTA):
    """-> m columns of n integers: delta^c w^r for (c, r) = mapping[j * n + i]"""
    n = 1 << k
    w = omega(k)
    wr, dc = [1] * n, [1] * m
    for r in range(1, n):
        wr[r] = wr[r - 1] * w % R
    for c in range(1, m):
        dc[c] = dc[c - 1] * delta % R
    return [[dc[c] * wr[r] % R for c, r in mapping[j * n:(j + 1) * n]] for j in range(m)]


def is_valid_mapping(mapping, m, k, usable):
    n = 1 << k
    if len(mapping) != m * n or any(not (0 <= c < m and 0 <= r < n) for c, r in mapping):
        return False
    if len(set(mapping)) != m * n:
        return False
    return all(mapping[j * n + i] == (j, i) for j in range(m) for i in range(usable, n))


def cycles_of(mapping, m, k):
    """the cycles of a valid mapping as a set of frozensets of cells"""
    n = 1 << k
    seen, out = set(), set()
    for j in range(m):
        for i in range(n):
            if (j, i) in seen:
                continue
            cyc, cur = [], (j, i)
            while cur not in seen:
                seen.add(cur)
                cyc.append(cur)
                cur = mapping[cur[0] * n + cur[1]]
            out.add(frozenset(cyc))
    return out


def classes_of(m, k, copies):
    """the classes of the equivalence relation the copies generate over all m * n cells (union-find, nothing of the assembly)"""
    n = 1 << k
    parent = {(j, i): (j, i) for j in range(m) for i in range(n)}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for lc, lr, rc, rr in copies:
        parent[find((lc, lr))] = find((rc, rr))
    groups = {}
    for cell in parent:
        groups.setdefault(find(cell), []).append(cell)
    return {frozenset(g) for g in groups.values()}


def random_copies(rng, m, k, usable, ncopies):
    if usable == 0:
        return []
    cell = lambda: (rng.randrange(m), rng.randrange(usable))
    return [cell() + cell() for _ in range(ncopies)]


def copies_from_classes(classes):
    """lists of equal cells -> a copy list that chains each class (cell t with cell t + 1)"""
    return [cells[t] + cells[t + 1] for cells in classes for t in range(len(cells) - 1)]


def invalid_mappings(rng, m, k, usable):
    """(name, mapping, in_range) for every way a mapping can be invalid, built from a valid one.  in_range False: an entry is
    outside the m x n cells (the host scan's to refuse); True: only the device can tell."""
    n = 1 << k
    assert m * n >= 2 and 0 < usable < n
    base = assembly_py(m, k, usable, random_copies(rng, m, k, usable, m * n))
    assert is_valid_mapping(base, m, k, usable)
    out = []
    dup = list(base)
    a, b = rng.sample(range(m * usable), 2)
    cell = lambda t: (t // usable) * n + t % usable
    dup[cell(a)] = dup[cell(b)]                                   # one duplicated target (still in range, rows stay usable)
    out.append(("duplicated target", dup, True))
    swp = list(base)
    j = rng.randrange(m)
    lo, hi = j * n + rng.randrange(usable), j * n + usable + rng.randrange(n - usable)
    swp[lo], swp[hi] = swp[hi], swp[lo]                           # a bijection still, but an unusable row moves
    out.append(("swap across the usable line", swp, True))
    col = list(base)
    col[rng.randrange(m * n)] = (m, 0)
    out.append(("column == m", col, False))
    row = list(base)
    row[rng.randrange(m * n)] = (0, n)
    out.append(("row == n", row, False))
    for name, mp, in_range in out:
        assert not is_valid_mapping(mp, m, k, usable), name
        assert all(c < m and r < n for c, r in mp) == in_range, name
    return out
