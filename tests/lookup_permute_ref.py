"""The definitions of include/h2agg.h's lookup block restated with Python integers — lookup_permute_py, compress_py — the
restatement of the device's sort and rank arithmetic on the host (radix_sort_py, permute_model_py: same tile, wave-column, bin
and scan layout as csrc/lookup_kernels.hpp, with every store position checked against u), and the inputs the tests feed them.
tests/test_lookup_permute_host.py ties the definition to the conditions the reference's verifier checks (lookup.rs:98-113) and
the model to sorted(); tests/test_gpu_lookup_permute.py compares the library with the definition byte for byte."""
import random
from collections import Counter

from tests.grand_product_ref import BIG, R

WAVES, BINS, PASSES, LANES = 4, 256, 32, 64
THREADS, TILE_LOG = 256, 11


class NotInTable(Exception):
    """halo2: Error::ConstraintSystemFailure; the library: H2AGG_ERR_NOT_IN_TABLE"""


def lookup_permute_py(a, s, u):
    """-> (ap[0 .. u), sp[0 .. u)): ap = a[:u] ascending; sp[i] = ap[i] where ap[i] starts a run, each such value taken out of
    the multiset s[:u] once; the rest of the multiset, ascending, fills the other rows from the highest row down"""
    ap = sorted(a[:u])
    table = Counter(s[:u])
    sp, free = [None] * u, []
    for i in range(u):
        if i == 0 or ap[i] != ap[i - 1]:
            if table[ap[i]] == 0:
                raise NotInTable(ap[i])
            table[ap[i]] -= 1
            sp[i] = ap[i]
        else:
            free.append(i)
    left = sorted(table.elements())
    assert len(left) == len(free)
    for j, row in enumerate(reversed(free)):
        sp[row] = left[j]
    return ap, sp


def compress_py(cols, theta):
    """out[i] = sum_j theta^(m - 1 - j) cols[j][i]: the fold acc * theta + expr"""
    out = [0] * len(cols[0])
    for col in cols:
        out = [(acc * theta + x) % R for acc, x in zip(out, col)]
    return out


# ---------------------------------------------------------------------------------------------- the device's arithmetic
def digit(x, p):
    return (x >> (8 * p)) & 0xFF


def geometry(t):
    """lookup.inc lk_geom: -> (entries per step of k_lk_scan_rows, threads of a workgroup of k_lk_digit_hist that take keys, its
    most workgroups).  Below the default tile all three shrink with the tile."""
    if t >= TILE_LOG:
        return 4 * THREADS, THREADS, 1024
    return 1 << (t - 2), 1 << (t - 2), 2


def loop_counts(u, t):
    """how often the three loops that depend on the geometry run for u rows: -> (steps of k_lk_scan_rows over a row of the count
    matrix, its steps over the tile sums, strides of thread 0 of k_lk_digit_hist)"""
    step, lanes, cap = geometry(t)
    tiles = (u + (1 << t) - 1) >> t
    grid = min((u + lanes - 1) // lanes, cap)
    return -(-WAVES * tiles // step), -(-tiles // step), -(-u // (grid * lanes))


def digit_hist_py(keys, t):
    """k_lk_digit_hist: thread x < lanes of workgroup b takes the keys b lanes + x + j grid lanes.  -> hist[32][256]"""
    u = len(keys)
    _step, lanes, cap = geometry(t)
    grid = min((u + lanes - 1) // lanes, cap)
    hist = [[0] * BINS for _ in range(PASSES)]
    seen = [0] * u
    for b in range(grid):
        for x in range(THREADS):
            i = b * lanes + x if x < lanes else u
            while i < u:
                seen[i] += 1
                for p in range(PASSES):
                    hist[p][digit(keys[i], p)] += 1
                i += grid * lanes
    assert seen == [1] * u, "a key counted twice or not at all"
    return hist


def scan_row_py(row, step, base):
    """k_lk_scan_rows over one row, in place: steps of `step` entries, thread x < step / 4 holds the entries start + 4 x .. + 3
    (all loaded before the step's first store), the step's sum is carried.  Every index is checked to be inside the row and
    inside the step."""
    ncols, carry = len(row), base
    assert step % 4 == 0 and 4 <= step <= 4 * THREADS
    for start in range(0, ncols, step):
        threads = min(step // 4, (ncols - start + 3) // 4)          # (the threads beyond hold zeros and store nothing)
        held = []
        for x in range(threads):
            e = start + 4 * x
            assert x < THREADS and e + 3 < start + step
            held.append([row[e + q] if e + q < ncols else 0 for q in range(4)])
        run = carry
        for x in range(threads):
            for q in range(4):
                e = start + 4 * x + q
                if e < ncols:
                    row[e] = run
                run += held[x][q]
        carry = run
    return row


def radix_sort_py(keys, t):
    """csrc/lookup_kernels.hpp on the host: k_lk_digit_hist, k_lk_plan, then per pass k_lk_tile_hist, k_lk_scan_rows and
    k_lk_scatter over tiles of 2^t keys.  -> (the keys of the final state, the passes that moved, the final state)"""
    u = len(keys)
    T, S = 1 << t, 1 << (t - 2)
    tiles = (u + T - 1) // T
    ncols = WAVES * tiles
    rounds = 1 if S <= LANES else S // LANES
    step = geometry(t)[0]
    hist = digit_hist_py(keys, t)
    plan, state = [], 0
    for p in range(PASSES):
        uniform = any(h == u for h in hist[p])
        plan.append((uniform, state))
        if not uniform:
            state = 2 if state == 1 else 1
    bufs = {0: list(keys), 1: [None] * u, 2: [None] * u}
    moved = []
    for p, (skip, st) in enumerate(plan):
        if skip:
            continue
        moved.append(p)
        src, dst = bufs[st], bufs[2 if st == 1 else 1]
        counts = [[0] * ncols for _ in range(BINS)]
        for col in range(ncols):                                   # k_lk_tile_hist
            for j in range(S):
                i = col * S + j
                if i < u:
                    counts[digit(src[i], p)][col] += 1
        for d in range(BINS):                                      # k_lk_scan_rows: base, then the exclusive prefix of the row
            scan_row_py(counts[d], step, sum(hist[p][:d]))
        for col in range(ncols):                                   # k_lk_scatter: one wave per column, rounds of 64 lanes
            off = [counts[d][col] for d in range(BINS)]
            for r in range(rounds):
                lanes = [(lane, col * S + LANES * r + lane) for lane in range(LANES)]
                act = [(lane, i) for lane, i in lanes if LANES * r + lane < S and i < u]
                pos = {}
                for lane, i in act:
                    d = digit(src[i], p)
                    rank = sum(1 for l2, i2 in act if l2 < lane and digit(src[i2], p) == d)
                    pos[i] = off[d] + rank
                for d, c in Counter(digit(src[i], p) for _, i in act).items():
                    off[d] += c
                for i, where in pos.items():
                    assert 0 <= where < u and dst[where] is None, (p, col, r, where)
                    dst[where] = src[i]
        if st:
            bufs[st] = [None] * u                                  # a work buffer is free again once it has been read (state 0 is never written)
    return bufs[state], moved, state


def prefix_py(flags, t):
    """k_lk_block_reduce, k_lk_scan_rows over the tile sums, k_lk_block_scan: -> len(flags) + 1 exclusive prefix sums"""
    n, T = len(flags), 1 << t
    sums = [sum(flags[b:b + T]) for b in range(0, n, T)]
    base = scan_row_py(list(sums), geometry(t)[0], 0)
    out = [None] * (n + 1)
    for b, lo in enumerate(range(0, n, T)):
        run = base[b]
        for i in range(lo, min(lo + T, n)):
            out[i] = run
            run += flags[i]
            if i + 1 == n:
                out[n] = run
    return out


def permute_model_py(a, s, u, t):
    """the whole device route: two sorts, k_lk_heads (binary search), two prefix sums, k_lk_leftovers, k_lk_fill.  -> (ap, sp,
    not_in_table)"""
    if u == 0:
        return [], [], False
    A, S = radix_sort_py(a[:u], t)[0], radix_sort_py(s[:u], t)[0]
    non_head, left, absent = [0] * u, [1] * u, False
    for i in range(u):
        if i and A[i] == A[i - 1]:
            non_head[i] = 1
            continue
        lo, hi = 0, u
        while lo < hi:
            mid = lo + ((hi - lo) >> 1)
            if S[mid] < A[i]:
                lo = mid + 1
            else:
                hi = mid
        if lo < u and S[lo] == A[i]:
            left[lo] = 0
        else:
            absent = True
    nh, lf = prefix_py(non_head, t), prefix_py(left, t)
    left_idx = [None] * u
    for q in range(u):
        if lf[q + 1] != lf[q]:
            left_idx[lf[q]] = q
    ap, sp = list(A), list(A)
    for i in range(u):
        if nh[i + 1] != nh[i]:
            j = nh[u] - 1 - nh[i]
            if j < lf[u] and left_idx[j] is not None:
                sp[i] = S[left_idx[j]]
    return ap, sp, absent


# ---------------------------------------------------------------------------------------------- inputs
def only_byte(seed, b, u):
    """u keys that differ in byte b only (top byte below 0x30: below r)"""
    rng = random.Random(seed)
    base = rng.randrange(1 << 248) | (rng.randrange(0x30) << 248)
    mask = ~(0xFF << (8 * b))
    span = 0x30 if b == 31 else 256
    return [(base & mask) | (((i * 37 + b) % span) << (8 * b)) for i in range(u)]


def key_patterns(seed, u):
    """-> [(name, a, s)], u rows each; every value of a occurs in s unless the name says otherwise"""
    rng = random.Random(seed)
    draw = lambda s: [s[rng.randrange(len(s))] for _ in range(u)]
    out = []
    s = [rng.randrange(1 << 253, R) for _ in range(u)]
    assert all(x.bit_length() == 254 for x in s)
    out.append(("random 254-bit", draw(s), s))
    for bits in (8, 16):
        s = [rng.randrange(1 << bits) for _ in range(u)]
        out.append(("below 2^%d" % bits, draw(s), s))
    for b in range(PASSES):
        s = only_byte(seed + b, b, u)
        out.append(("byte %d only" % b, draw(s), s))
    s = [rng.randrange(R) for _ in range(u)]
    special = [0, 1, R - 1, BIG]
    for j, v in enumerate(special[:u]):
        s[(j * 17) % u] = v
    a = draw(s)
    for j, v in enumerate(special[:u]):
        if v in s:
            a[(j * 29 + 1) % u] = v
    out.append(("0, 1, r - 1, BIG", a, s))
    s = sorted(rng.randrange(R) for _ in range(u))
    out.append(("ascending", list(s), s))
    out.append(("descending", s[::-1], s[::-1]))
    s = [rng.randrange(R) for _ in range(u)]
    out.append(("all inputs equal", [s[u // 2]] * u, s))
    s = [(1 << 200) + (x << 64) + rng.randrange(1 << 64) for x in rng.sample(range(1 << 40), u)]   # duplicate-free
    a = list(s)
    rng.shuffle(a)
    out.append(("a permutation of a duplicate-free table", a, s))
    # repeated table values below and above every input: two different ones on each side, one of them three times
    mid = [rng.randrange(1 << 100, 1 << 101) for _ in range(max(u - 10, 1))]
    lo, hi = [5, 5, 5, 9, 9], [R - 2, R - 2, R - 2, R - 7, R - 7]
    s = (lo + hi + mid)[:u] if u > 10 else (mid * u)[:u]
    s = s + [mid[0]] * (u - len(s))
    rng.shuffle(s)
    out.append(("table repeats below and above the inputs", [mid[rng.randrange(len(mid))] for _ in range(u)], s))
    for name, a, s in out:
        assert len(a) == u and len(s) == u, name
    return out
