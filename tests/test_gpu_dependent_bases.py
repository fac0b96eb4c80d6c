"""multi_exp over DEPENDENT bases: every base is m_i * P for one random point P = k * G and known small integers m_i, so that
operands of the group additions behind the bucket insertion are equal, opposite or the identity BY CONSTRUCTION — the branches
`a == b`, `a == -b` and "the accumulator became the identity mid-run" of the bucket accumulation's fix-up list, of the
reductions / window sums, of the Horner tail (lp_add_points) and of the segmented multi_exp's window kernel, which independent
random bases reach with probability ~2^-27.

The reference is exact: ((sum_i m_i s_i) mod r) * P — the sum in Python integers, one scalar multiplication by the oracle,
canonical affine bytes compared for equality; for n <= 1024 also the restated reference algorithm (cref.multi_exp_naive).
Bases come from the oracle, never from the engine.  The conditions that make an input meet its target (pigeonhole, divisible run
lengths, 2^c * (window sum) == +- (next window sum), equal weighted buckets) are asserted on the inputs with the oracle alone.
"""
import functools
from contextlib import contextmanager

import pytest

from oracle import bn254 as O, cref
from tests.util import bases_from_coefficients, fr_bytes, msm_want, norm, rand_frs, to_jac_bytes

pytestmark = pytest.mark.gpu

DEFAULT_C_SMALL = 8          # the documented default plan: 8-bit windows up to 2^12 points, GLV or not
DEBUG_DEFAULTS = {"small_sort": 1, "pcie_slices": 0, "pcie_chain": 1, "seg_c": 0, "seg_chunk": 0, "comb_msm": 1}


@contextmanager
def configured(eng, window_bits=0, reduce_segment=0, big=0, glv=0, sort=(0, 0), lanes=0, debug=()):
    """one MSM configuration, restored whatever happens"""
    try:
        eng.msm_configure(window_bits=window_bits, reduce_segment=reduce_segment, big_bucket_threshold=big)
        eng.msm_configure_glv(glv)
        eng.msm_configure_sort(*sort)
        eng.msm_configure_lanes_per_bucket(lanes)
        for key, value in debug:
            eng.debug_configure(key, value)
        yield
    finally:
        eng.msm_configure()
        eng.msm_configure_glv(0)
        eng.msm_configure_sort()
        eng.msm_configure_lanes_per_bucket(0)
        for key, _ in debug:
            eng.debug_configure(key, DEBUG_DEFAULTS[key])


# ------------------------------------------------------------------ input families: (n, seed) -> k, m_i, s_i
def one_point(n, seed):
    rng = O.SplitMix64(seed)
    return rng.fr(), [1] * n, rand_frs(rng, n)


def alternating_sign(n, seed):
    """+P, -P, +P, ... with blocks of 7 consecutive entries sharing a scalar: a bucket's running sum goes P, identity, P, ...
    and ends at +-P (an odd block length: the multi_exp as a whole is not the identity)"""
    rng = O.SplitMix64(seed)
    k = rng.fr()
    blocks = rand_frs(rng, (n + 6) // 7)
    return k, [1 if i % 2 == 0 else -1 for i in range(n)], [blocks[i // 7] for i in range(n)]


def small_multiples(n, seed):
    rng = O.SplitMix64(seed)
    k = rng.fr()
    return k, [rng.next() % 9 - 4 for _ in range(n)], rand_frs(rng, n)


def one_point_equal_scalars(n, seed):
    rng = O.SplitMix64(seed)
    k = rng.fr()
    return k, [1] * n, [rng.fr()] * n


FAMILIES = {"one_point": one_point, "alternating_sign": alternating_sign, "small_multiples": small_multiples,
            "one_point_equal_scalars": one_point_equal_scalars}


class Case:
    """bases / scalars as bytes and the expected multi_exp, computed once per (family, n) and shared read-only"""

    def __init__(self, gs, ss, ms=None):
        self.n, self.gs, self.ss, self.ms = len(gs), gs, ss, ms
        self.bases = bases_from_coefficients(gs)
        self.scalars = fr_bytes(ss)
        self.want = msm_want(gs, ss)
        if self.n <= 1024:
            assert cref.multi_exp_naive(self.bases, self.scalars, self.n) == self.want   # the reference algorithm agrees

    def want_prefix(self, m):
        return msm_want(self.gs[:m], self.ss[:m])


@functools.lru_cache(maxsize=None)
def family_case(name, n):
    k, ms, ss = FAMILIES[name](n, 0xDE9 + 31 * n + len(name))
    assert set(ms) <= set(range(-4, 5))
    return Case([m * k % O.R for m in ms], ss, ms)


def check_msm(eng, case):
    got = norm(eng, eng.g1_msm(case.bases, case.scalars))
    assert got == case.want


# ------------------------------------------------------------------ families 1 - 3 through every g1_msm route
ROUTES = {
    "default": {},
    "c2": {"window_bits": 2},
    "c5": {"window_bits": 5},
    "c8": {"window_bits": 8},
    "c13": {"window_bits": 13},
    "c16": {"window_bits": 16},                              # the 256 x 128 two-dimensional reduction
    "c8_seg4": {"window_bits": 8, "reduce_segment": 4},      # the running-sum segment kernels
    "glv_on": {"glv": 1},
    "glv_off": {"glv": -1},
    "small_sort_off": {"debug": (("small_sort", 0),)},
    "sort_direct": {"sort": (0, -1)},
    "sort_sub4": {"sort": (4, 0)},
    "lanes1": {"lanes": 1},
    "lanes2": {"lanes": 2},
    "lanes4": {"lanes": 4},
    "lanes8": {"lanes": 8},
    "lanes16": {"lanes": 16},
    "big64": {"big": 64},
}


@pytest.mark.parametrize("n", [600, 3000])
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("family", ["one_point", "alternating_sign", "small_multiples"])
def test_family_through_route(eng, family, route, n):
    case = family_case(family, n)
    cfg = ROUTES[route]
    c = cfg.get("window_bits", DEFAULT_C_SMALL)
    if family == "one_point" and c <= 8:
        # pigeonhole: more points than a window has digit values (GLV: than a half has), so some bucket's second insertion is
        # P + P.  (Wider windows get their own sizes: test_one_point_fills_wide_windows.)
        assert n > 2 ** c
    with configured(eng, **cfg):
        check_msm(eng, case)


@pytest.mark.parametrize("c,n", [(13, 20000), (16, 70000)])
@pytest.mark.parametrize("glv", [1, -1])
def test_one_point_fills_wide_windows(eng, c, n, glv):
    """the same pigeonhole for 13- and 16-bit windows: n > 2^c copies of one point"""
    assert n > 2 ** c
    case = family_case("one_point", n)
    with configured(eng, window_bits=c, glv=glv):
        check_msm(eng, case)


@pytest.mark.parametrize("chain", [1, 0])
@pytest.mark.parametrize("family", ["one_point", "alternating_sign", "small_multiples"])
def test_family_through_host_slices(eng, family, chain):
    """four host-buffer slices: chained (pcie_chain 1), the buckets of slices 2 .. 4 resume from the stored sums of equal,
    opposite and identity values; unchained, four partial results that are multiples of one point are added"""
    n = 20000
    assert n >= 4 * 1024          # (what the library asks before it takes a forced slice count)
    case = family_case(family, n)
    with configured(eng, debug=(("pcie_slices", 4), ("pcie_chain", chain))):
        check_msm(eng, case)
    with configured(eng, window_bits=8, debug=(("pcie_slices", 4), ("pcie_chain", chain))):
        check_msm(eng, case)


# ------------------------------------------------------------------ family 4: equal slice sums, equal chunk sums
@pytest.mark.parametrize("glv", [1, -1])
@pytest.mark.parametrize("n", [600, 3000])
def test_equal_scalars_big_bucket_chunks(eng, n, glv):
    """one bucket per window, over the threshold: the chunk sums of k_msm_accumulate_big are multiples of P (equal where the
    chunks are equally long) and k_msm_big_combine adds them"""
    case = family_case("one_point_equal_scalars", n)
    assert n > 64
    with configured(eng, window_bits=8, big=64, glv=glv):
        check_msm(eng, case)
    with configured(eng, big=64, glv=glv):
        check_msm(eng, case)


@pytest.mark.parametrize("glv", [1, -1])
@pytest.mark.parametrize("lanes", [2, 4, 8])
@pytest.mark.parametrize("n", [600, 3000])
def test_equal_scalars_lane_slices(eng, n, lanes, glv):
    """one bucket per window, under the threshold, cut into `lanes` slices of the same length: every slice sum is the same
    multiple of P and k_msm_bucket_combine adds equal operands; inside a slice the second insertion is P + P (fix-up list on a
    slice)"""
    case = family_case("one_point_equal_scalars", n)
    assert n % lanes == 0 and n < 4096
    with configured(eng, window_bits=8, big=4096, lanes=lanes, glv=glv):
        check_msm(eng, case)


# ------------------------------------------------------------------ other entry points
@pytest.mark.parametrize("n", [600, 3000])
@pytest.mark.parametrize("family", ["one_point", "alternating_sign", "small_multiples"])
def test_family_over_projective_points(eng, family, n):
    case = family_case(family, n)
    rng = O.SplitMix64(0x7AC + n)
    jac = to_jac_bytes(case.bases, [rng.fr() % O.P or 1 for _ in range(n)])
    assert norm(eng, eng.g1_msm_jac(jac, case.scalars)) == case.want


@pytest.mark.parametrize("n", [600, 3000])
@pytest.mark.parametrize("family", ["one_point", "alternating_sign", "small_multiples"])
def test_family_preloaded_prefix_and_batch(eng, family, n):
    """a resident table: the whole table, a prefix, and the batch entry point (three scalar vectors over one table)"""
    import numpy as np
    import torch
    case = family_case(family, n)
    h = eng.bases_upload(case.bases)
    try:
        assert norm(eng, eng.g1_msm_preloaded(h, case.scalars)) == case.want
        m = n - 77
        assert norm(eng, eng.g1_msm_preloaded(h, case.scalars[:32 * m])) == case.want_prefix(m)
        rows = [case.ss, case.ss[::-1], [case.ss[0]] * n]
        dev = torch.device("cuda", 0)
        d_s = torch.from_numpy(np.frombuffer(b"".join(fr_bytes(r) for r in rows), dtype=np.uint8).copy()).to(dev)
        d_out = torch.zeros(96 * len(rows), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        eng.g1_msm_device_batch_async(h, d_s.data_ptr(), n, len(rows), d_out.data_ptr())
        eng.synchronize()
        got = norm(eng, bytes(d_out.cpu().numpy().tobytes()))
        assert got == b"".join(msm_want(case.gs, r) for r in rows)
    finally:
        eng.bases_free(h)


@pytest.mark.parametrize("cw,n", [(11, 5000), (20, 300)])
@pytest.mark.parametrize("family", ["one_point", "alternating_sign", "small_multiples"])
def test_family_over_fixed_base_levels(eng, family, cw, n):
    """h2agg_bases_precompute: the levels 2^(c w) * (m_i P) are dependent too; one bucket set, folded and summed by k_fb_fold /
    k_fb_wsum"""
    case = family_case(family, n)
    h = eng.bases_upload(case.bases)
    try:
        eng.bases_precompute(h, cw)
        assert norm(eng, eng.g1_msm_preloaded(h, case.scalars)) == case.want
        m = n - 33
        assert norm(eng, eng.g1_msm_preloaded(h, case.scalars[:32 * m])) == case.want_prefix(m)
    finally:
        eng.bases_free(h)


@pytest.mark.parametrize("comb", [1, 0])
@pytest.mark.parametrize("precompute", [False, True])
def test_instance_commitment_over_one_point_table(eng, comb, precompute):
    """a g_lagrange table that is one point repeated: a short column (the table's comb where it has one) and a long one"""
    n_table = 600
    rng = O.SplitMix64(0x1C0)
    k = rng.fr()
    gs = [k] * n_table
    h = eng.bases_upload(bases_from_coefficients(gs))
    try:
        if precompute:
            eng.bases_precompute(h)
        with configured(eng, debug=(("comb_msm", comb),)):
            for m in (7, 300, 500):
                inst = rand_frs(rng, m)
                if m == 7:
                    inst[1] = inst[0]
                    inst[3] = O.R - inst[2]          # v P + (-v) P inside the column
                assert norm(eng, eng.instance_commitment(h, fr_bytes(inst), n_table - 6)) == msm_want(gs[:m], inst), m
    finally:
        eng.bases_free(h)


@pytest.mark.parametrize("n", [600, 3000])
@pytest.mark.parametrize("family", ["one_point", "alternating_sign", "small_multiples"])
def test_eval_flat_tail_meets_its_own_result(eng, family, n):
    """k_eval_tail adds the scalar-less points to the multi_exp's result: that result itself (a doubling), its negative (the
    identity), the identity, and runs of them"""
    case = family_case(family, n)
    total = sum(g * s for g, s in zip(case.gs, case.ss)) % O.R
    assert total != 0
    for tail in ([1], [-1], [0], [0, -1, 1, 1], [-1, -1, 0, 1, 1, 1]):
        gs = case.gs + [t * total % O.R for t in tail]
        pts = case.bases + bases_from_coefficients(gs[n:])
        has = bytes([1] * n + [0] * len(tail))
        want = O.aff_to_bytes(O.scalar_mul((1 + sum(tail)) * total % O.R, O.G1))
        assert norm(eng, eng.eval_flat(pts, case.scalars + bytes(32 * len(tail)), has)) == want, tail


@pytest.mark.parametrize("n", [2, 8, 300])
@pytest.mark.parametrize("alternate", [False, True])
def test_g1_sum_of_one_point(eng, n, alternate):
    rng = O.SplitMix64(0x5A + n)
    k = rng.fr()
    gs = [(O.R - k if alternate and i % 2 else k) for i in range(n)]
    jac = to_jac_bytes(bases_from_coefficients(gs), [rng.fr() % O.P or 1 for _ in range(n)])
    assert norm(eng, eng.g1_sum(jac)) == msm_want(gs, [1] * n)
    n_odd = n - 1
    assert norm(eng, eng.g1_sum(jac[:96 * n_odd])) == msm_want(gs[:n_odd], [1] * n_odd)


# ------------------------------------------------------------------ family 5: the Horner chain
def horner_case(c, events, seed, low_base=True):
    """bases / scalars whose c-bit digits are 0 or 1 (so any recoding keeps them) such that at every event (w, sign) the Horner
    accumulator, after the c doublings below window w, is `sign` times the sum of window w - 1: equal (the doubling fallback of
    lp_add_points) or opposite (the chain goes on from the identity).  events: descending w, two windows apart at least.
    low_base: an unrelated third base fills the windows below the last event so that the chain goes on after it.
    -> (Case, checks) with checks = [(coefficient of the accumulator after the doublings, coefficient of the next window sum,
    sign)] as multiples of P."""
    rng = O.SplitMix64(seed)
    k = rng.fr()
    ms, ss = [1], [sum(1 << (c * w) for w, _ in events)]            # P carries a digit 1 in every event's window
    checks = []

    def window_sums():   # plain c-bit digits (all 0 / 1 here) times the m_i
        top = max(s.bit_length() for s in ss) // c + 1
        return [sum(m * ((s >> (c * w)) & ((1 << c) - 1)) for m, s in zip(ms, ss)) for w in range(top)]

    for j, (w, sign) in enumerate(events):
        assert w >= 1 and (j == 0 or w <= events[j - 1][0] - 2)
        sums = window_sums()
        acc = 0
        for v in range(len(sums) - 1, w - 1, -1):                   # Horner down to window w, with what is defined so far
            acc = (acc << c) + sums[v]
        assert sums[w - 1] == 0                                     # window w - 1 is this event's alone
        q = sign * (acc << c)                                       # first event: Q = +-2^c P
        ms.append(q)
        ss.append(1 << (c * (w - 1)))
        checks.append((acc << c, q, sign))
    gs = [m * k % O.R for m in ms]
    w_last = events[-1][0]
    if low_base and c * (w_last - 1) - 2 > 0:
        gs.append(rng.fr())                                         # unrelated to P
        ss.append(rng.fr() % (1 << (c * (w_last - 1) - 2)))         # (two clear bits: no signed-digit carry into the event's window)
    P = O.scalar_mul(k, O.G1)
    for acc_c, q, sign in checks:                                   # the input meets its target: 2^c * (sum so far) == +- (next window sum)
        lhs, rhs = O.scalar_mul(acc_c % O.R, P), O.scalar_mul(q % O.R, P)
        assert lhs == (rhs if sign > 0 else O.neg(rhs)) and lhs is not O.INF
    assert all(0 <= s < O.R for s in ss)
    return Case(gs, ss), checks


def horner_variants(c, top_w):
    """top_w: the highest window an event may use"""
    mid = max(2, top_w // 2)
    return {
        "equal_at_bottom": ([(1, +1)], False),
        "opposite_at_bottom": ([(1, -1)], False),
        "middle_equal": ([(mid, +1)], True),
        "middle_opposite": ([(mid, -1)], True),
        "twice_equal_opposite": ([(top_w, +1), (mid, -1)], True),
        "twice_opposite_equal": ([(top_w, -1), (mid, +1)], True),
        "twice_equal_equal_bottom": ([(top_w, +1), (1, +1)], False),
    }


HORNER_NAMES = list(horner_variants(8, 10))


@pytest.mark.parametrize("variant", HORNER_NAMES)
@pytest.mark.parametrize("c", [5, 8, 13, 16])
@pytest.mark.parametrize("glv", [-1, 1])
def test_horner_chain_meets_equal_and_opposite(eng, c, variant, glv):
    if glv > 0:
        top_w = 112 // c             # scalars under 2^112 + c bits: their own k1, k2 = 0
    else:
        top_w = 250 // c - 1         # 2^(c top_w) well under r
    events, low = horner_variants(c, top_w)[variant]
    assert top_w >= 4 and all(c * w <= (112 if glv > 0 else 250) for w, _ in events)
    case, _ = horner_case(c, events, 0x40A + c, low)
    with configured(eng, window_bits=c, glv=glv):
        check_msm(eng, case)


# ------------------------------------------------------------------ family 6: the endomorphism column next to lambda * P
@functools.lru_cache(maxsize=None)
def endo_cases():
    """bases P and root * P with the scalars (root, 1), (-root, -1), (root, -1), (-root, 1), for both primitive cube roots of
    unity in Fr (one of them is the library's lambda); each alone and inside an ordinary MSM"""
    lam = pow(5, (O.R - 1) // 3, O.R)
    assert lam != 1 and pow(lam, 3, O.R) == 1
    k = O.SplitMix64(0xE7D0).fr()
    filler = family_case("small_multiples", 600)
    cases = []
    for root in (lam, lam * lam % O.R):
        gs = [k, root * k % O.R]
        for ss in ([root, 1], [O.R - root, O.R - 1], [root, O.R - 1], [O.R - root, 1]):
            cases.append(Case(gs, ss))
            cases.append(Case(gs + filler.gs, ss + filler.ss))
    return cases


@pytest.mark.parametrize("c", [0, 5, 13, 16])
def test_endo_collision(eng, c):
    """GLV on: the scalar lambda splits into k1 = 0, k2 = 1, so phi(P) = lambda * P (from the endomorphism column) lands in
    digit-1's bucket of window 0 next to the plain base lambda * P with the scalar 1 — equal points; with -1 / r - lambda
    opposite ones.  The assertion is the oracle's result only."""
    for case in endo_cases():
        with configured(eng, window_bits=c, glv=1):
            check_msm(eng, case)


# ------------------------------------------------------------------ the segmented multi_exp, every window width
SEG_LENS = [1, 2, 2, 40, 64, 65, 300, 1, 700]       # 700 > seg_chunk = 500: an ordinary msm_run of its own


def check_segmented(eng, C, seg_chunk, gs, ss, lens):
    assert sum(lens) == len(gs) == len(ss)
    with configured(eng, debug=(("seg_c", C), ("seg_chunk", seg_chunk))):
        got = eng.g1_msm_segmented(bases_from_coefficients(gs), fr_bytes(ss), lens)
    aff = norm(eng, b"".join(got))
    at = 0
    for s, ln in enumerate(lens):
        assert aff[64 * s:64 * s + 64] == msm_want(gs[at:at + ln], ss[at:at + ln]), (s, ln)
        at += ln


@pytest.mark.parametrize("seg_chunk", [0, 500])
@pytest.mark.parametrize("C", [4, 5, 6, 7, 8])
@pytest.mark.parametrize("family", ["one_point", "alternating_sign", "small_multiples"])
def test_segmented_families(eng, family, C, seg_chunk):
    case = family_case(family, sum(SEG_LENS))
    if family == "one_point":
        assert max(SEG_LENS[:-1]) > 2 ** C                # pigeonhole inside the 300-point segment
    check_segmented(eng, C, seg_chunk, case.gs, case.ss, SEG_LENS)


def seg_tree_segments(C, k, rng):
    """segments aimed at the workgroup sum of k_seg_window<C>: lane b holds b * (bucket b); lanes 1 and 2 meet at the last
    level of the tree.  -> [(coefficients, scalars)]"""
    P = O.scalar_mul(k, O.G1)
    segs = []
    for m0 in (2, -2):      # [m0 P, P] with window-0 digits 1 and 2: the weighted buckets 1 * (m0 P) and 2 * P
        d = [1, 2]
        ms = [m0, 1]
        a, b = O.scalar_mul(d[0] * ms[0] % O.R, P), O.scalar_mul(d[1] * ms[1] % O.R, P)
        assert a == (b if m0 > 0 else O.neg(b))                       # 2P + 2P, resp. -2P + 2P
        hi = rng.fr() >> (C + 8) << C                                 # the other windows: the same random digits for both
        segs.append(([m * k % O.R for m in ms], [hi + d[0], hi + d[1]]))
    s = rng.fr()
    segs.append(([k] * 40, [s] * 40))                                 # 40 copies of P, equal scalars: every bucket 40 P, P + P first
    W = (255 + C - 1) // C
    top_bit = C * (W - 1)
    assert top_bit <= 252                                             # digits 1 and 2 there stay under r
    top = [(1 + i % 2) << top_bit for i in range(64)]                 # only the top window is occupied
    assert all(t < O.R and t % (1 << top_bit) == 0 for t in top)
    segs.append(([k] * 64, top))
    return segs


@pytest.mark.parametrize("seg_chunk", [0, 500])
@pytest.mark.parametrize("C", [4, 5, 6, 7, 8])
def test_segmented_tree_and_horner(eng, C, seg_chunk):
    """crafted segments: the seg_tree_* inputs, and the Horner constructions with C-bit windows (the segmented multi_exp's
    digits are plain C-bit fields), each a segment of its own, between ordinary ones"""
    rng = O.SplitMix64(0x5E67 + C)
    k = rng.fr()
    segs = seg_tree_segments(C, k, rng)
    top_w = 250 // C - 1
    for name, (events, low) in horner_variants(C, top_w).items():
        case, _ = horner_case(C, events, 0x5E0 + C + len(name), low)
        segs.append((case.gs, case.ss))
    filler = family_case("small_multiples", 600)
    segs.insert(2, (filler.gs[:65], filler.ss[:65]))
    segs.append((filler.gs, filler.ss))                               # 600 > seg_chunk = 500
    gs = [g for seg in segs for g in seg[0]]
    ss = [s for seg in segs for s in seg[1]]
    check_segmented(eng, C, seg_chunk, gs, ss, [len(seg[0]) for seg in segs])
