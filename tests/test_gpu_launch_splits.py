"""GPU: launches that are cut because a grid dimension ends at 65535, and the segmented multi_exp at its longest segment.

  * h2agg_columns_move queues one launch per 65535 columns (csrc/columns.inc): stores of 65537 columns at k = 0 and 65536 at
    k = 1, whose contents encode their own column index, so a launch applied at the wrong offset shows.
  * seg_msm_run (csrc/seg_msm.inc) takes whole segments in groups of at most 16384 points and at most 65535 segments: 65537
    one-point segments end a group at the point limit; with the debug key seg_chunk above that, at the segment limit.
  * k_seg_window at SEG_MAX_LEN = 16384 points, where its 16-bit LDS indices and its dynamic LDS are largest, one point below
    it and one above (an ordinary MSM), at window widths 4, 5 and 8; one lane walking a run of all 16384 indices; groups
    packed against the 16384-point limit.
Bases are multiples of G with known coefficients (tests/test_gpu_dependent_bases.py), so every expected value is exact."""
import pytest

from oracle import bn254 as O
from tests.util import bases_from_coefficients, fr_bytes, msm_want, norm, rand_frs

pytestmark = pytest.mark.gpu

GRID_Y = 65535
SEG_MAX_LEN = 16384


# ---------------------------------------------------------------------------------------------- columns_move
def index_columns(m, k, tag):
    """m columns of 2^k rows, row i of column j holding tag + j * 2^k + i: every element names its place"""
    return fr_bytes(range(tag, tag + (m << k)))


def test_columns_move_across_the_grid_split_at_k0(eng):
    m, k = GRID_Y + 2, 0
    src, old = index_columns(m, k, 1), index_columns(m, k, 1 << 40)
    a, b = eng.columns_create(m, k), eng.columns_create(m, k)
    try:
        eng.columns_write(a, 0, src)
        for count in (GRID_Y, GRID_Y + 1, GRID_Y + 2):
            for rotation in (0, 1):                               # n = 1: every rotation is the identity
                eng.columns_write(b, 0, old)
                eng.columns_move(a, 0, b, 0, count, rotation)
                got = eng.columns_read(b, 0, m)
                assert got[:32 * count] == src[:32 * count], (count, rotation)
                assert got[32 * count:] == old[32 * count:], (count, rotation, "columns behind the range")
        # a range that starts inside the store: the second launch's offset is relative to the range
        eng.columns_write(b, 0, old)
        eng.columns_move(a, 1, b, 0, GRID_Y + 1, 0)
        got = eng.columns_read(b, 0, m)
        assert got[:32 * (GRID_Y + 1)] == src[32:] and got[32 * (GRID_Y + 1):] == old[32 * (GRID_Y + 1):]
        assert eng.columns_read(a, 0, m) == src
    finally:
        eng.columns_destroy(a)
        eng.columns_destroy(b)


@pytest.mark.parametrize("rotation", [1, -1])
def test_columns_move_across_the_grid_split_at_k1(eng, rotation):
    m, k = GRID_Y + 1, 1
    src = index_columns(m, k, 1)
    a, b = eng.columns_create(m, k), eng.columns_create(m, k)
    try:
        eng.columns_write(a, 0, src)
        eng.columns_move(a, 0, b, 0, m, rotation)
        got = eng.columns_read(b, 0, m)
        want = b"".join(src[64 * j + 32:64 * j + 64] + src[64 * j:64 * j + 32] for j in range(m))   # the two rows swap
        bad = [j for j in range(m) if got[64 * j:64 * j + 64] != want[64 * j:64 * j + 64]]
        assert not bad, bad[:8]
    finally:
        eng.columns_destroy(a)
        eng.columns_destroy(b)


# ---------------------------------------------------------------------------------------------- segmented multi_exp
@pytest.fixture(scope="module")
def pairs():
    """16 (coefficient, scalar) pairs with g * s * G for each, and 64 coefficients for longer segments"""
    rng = O.SplitMix64(0x5E65)
    gs, ss = rand_frs(rng, 16), rand_frs(rng, 16)
    ss[3], ss[5], gs[7] = O.R - 1, 1, 0
    return gs, ss, [msm_want([g], [s]) for g, s in zip(gs, ss)], rand_frs(rng, 64)


def one_point_segments(pairs, nseg):
    gs16, ss16, want16, _ = pairs
    gs = [gs16[i % 16] for i in range(nseg)]
    ss = [ss16[i % 16] for i in range(nseg)]
    return gs, ss, [want16[i % 16] for i in range(nseg)]


@pytest.mark.parametrize("seg_chunk", [0, 1 << 20])
def test_segmented_65537_one_point_segments(eng, pairs, seg_chunk):
    """seg_chunk 0: groups end at 16384 points, four whole groups and one segment; 2^20: at 65535 segments, the grid's limit"""
    nseg = GRID_Y + 2
    gs, ss, want = one_point_segments(pairs, nseg)
    assert nseg > 4 * SEG_MAX_LEN and nseg - GRID_Y == 2 and nseg < (seg_chunk or nseg + 1)
    try:
        eng.debug_configure("seg_chunk", seg_chunk)
        got = eng.g1_msm_segmented(bases_from_coefficients(gs), fr_bytes(ss), [1] * nseg)
    finally:
        eng.debug_configure("seg_chunk", 0)
    aff = norm(None, b"".join(got))
    bad = [s for s in range(nseg) if aff[64 * s:64 * s + 64] != want[s]]
    assert not bad, bad[:8]


@pytest.mark.parametrize("seg_chunk", [0, 1 << 20])
def test_segmented_65536_one_point_segments_then_forty(eng, pairs, seg_chunk):
    nseg = GRID_Y + 1
    gs, ss, want = one_point_segments(pairs, nseg)
    rng = O.SplitMix64(0x40)
    tail_g, tail_s = [pairs[3][i] for i in range(40)], rand_frs(rng, 40)
    try:
        eng.debug_configure("seg_chunk", seg_chunk)
        got = eng.g1_msm_segmented(bases_from_coefficients(gs + tail_g), fr_bytes(ss + tail_s), [1] * nseg + [40])
    finally:
        eng.debug_configure("seg_chunk", 0)
    aff = norm(None, b"".join(got))
    bad = [s for s in range(nseg) if aff[64 * s:64 * s + 64] != want[s]]
    assert not bad, bad[:8]
    assert aff[64 * nseg:] == msm_want(tail_g, tail_s)


def check_segments(eng, pairs, lens, seed, C=0, ss=None):
    pool64 = pairs[3]
    n = sum(lens)
    rng = O.SplitMix64(seed)
    gs = [pool64[(5 * i + i // 64) % 64] for i in range(n)]
    ss = rand_frs(rng, n) if ss is None else ss
    try:
        eng.debug_configure("seg_c", C)
        got = eng.g1_msm_segmented(bases_from_coefficients(gs), fr_bytes(ss), lens)
    finally:
        eng.debug_configure("seg_c", 0)
    aff = norm(None, b"".join(got))
    at = 0
    for s, ln in enumerate(lens):
        assert aff[64 * s:64 * s + 64] == msm_want(gs[at:at + ln], ss[at:at + ln]), (s, ln)
        at += ln


@pytest.mark.parametrize("C", [4, 5, 8])
@pytest.mark.parametrize("length", [SEG_MAX_LEN - 1, SEG_MAX_LEN, SEG_MAX_LEN + 1])
def test_one_segment_around_the_longest_the_window_kernel_takes(eng, pairs, length, C):
    """16384 is the last length through k_seg_window (indices up to 0x3fff in 16 bits, 2 * 16384 + 8 * 2^C + 4 bytes of
    sort area); 16385 is an ordinary msm_run of its own"""
    check_segments(eng, pairs, [length], 0x16000 + length + C, C)


def test_one_lane_walks_a_run_of_16384_indices(eng, pairs):
    """every scalar the same, every 5-bit digit of it 1: bucket 1 of every window holds the whole segment"""
    s = sum(1 << (5 * w) for w in range(51))
    assert s < O.R and all((s >> (5 * w)) & 31 == 1 for w in range(51))
    check_segments(eng, pairs, [SEG_MAX_LEN], 0x1A4E, ss=[s] * SEG_MAX_LEN)


@pytest.mark.parametrize("lens", [[16000, 384, 1], [16000, 385]])
def test_groups_packed_against_the_point_limit(eng, pairs, lens):
    """16000 + 384 points fill a group to the last point, so the one-point segment starts the next; 16000 + 385 is one point
    over, so the second segment does"""
    assert sum(lens[:2]) - SEG_MAX_LEN in (0, 1)
    check_segments(eng, pairs, lens, 0x9AC + len(lens))
