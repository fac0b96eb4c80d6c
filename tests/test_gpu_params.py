"""GPU: KZG parameters made on the device — h2agg_params_setup (ParamsKZG::setup with a known trapdoor) and h2agg_bases_fft
(g_to_lagrange / ParamsKZG::downsize), through fs.setup_params / fs.downsize_params.

halo2_proofs is not vendored in the reference, so the yardstick is the definition: g[i] = s^i G, g_lagrange[i] = L_i(s) G,
out[i] = sum_j w^(+-ij) in[j] (times 1/n for the inverse), each evaluated by the oracle's C code (one scalar multiplication or
one Pippenger multi_exp per output point) and compared byte for byte."""
import importlib

import pytest

import __graft_entry__ as entry
from oracle import bn254 as O
from oracle import cref
from oracle import verifier as V

pytestmark = pytest.mark.gpu

G = O.aff_to_bytes(O.G1)
ID = bytes(64)


def fb(x):
    return O.fe_to_bytes(x % O.R)


def mul_g(dlogs):
    """[d * G for d in dlogs] as affine bytes (identity = zeros), by the oracle"""
    n = len(dlogs)
    return cref.g1_batch_to_affine(cref.g1_batch_scalar_mul(G * n, b"".join(fb(d) for d in dlogs), n), n)


def lagrange_dlogs(k, s):
    n = 1 << k
    w = V.omega_for_k(k)
    c = (pow(s, n, O.R) - 1) * O.inv(n, O.R) % O.R
    return [pow(w, i, O.R) * c % O.R * O.inv((s - pow(w, i, O.R)) % O.R, O.R) % O.R for i in range(n)]


def dft_rows(k, inverse, rows):
    """the scalars [w^(+-ij) * (1/n or 1)]_j of output i, for i in rows"""
    n = 1 << k
    w = V.omega_for_k(k)
    if inverse:
        w = O.inv(w, O.R)
    f = O.inv(n, O.R) if inverse else 1
    return {i: b"".join(fb(pow(w, i * j, O.R) * f) for j in range(n)) for i in rows}


def oracle_fft(points, k, inverse, rows=None):
    n = 1 << k
    rows = list(range(n)) if rows is None else rows
    sc = dft_rows(k, inverse, rows)
    return {i: cref.msm_pippenger(points, sc[i], n) for i in rows}


def table(eng, h, n):
    return eng.bases_download(h, 0, n)


def split(b):
    return [b[i:i + 64] for i in range(0, len(b), 64)]


def run_fft(eng, points, k, inverse):
    """upload, transform, download, free; also checks that the input table is left as it was"""
    n = 1 << k
    h = eng.bases_upload(points)
    try:
        o = eng.bases_fft(h, k, inverse)
        try:
            got = table(eng, o, n)
        finally:
            eng.bases_free(o)
        assert table(eng, h, len(points) // 64) == points, "bases_fft changed its input table"
    finally:
        eng.bases_free(h)
    return split(got)


SMALL_S = 5
BIG_S = O.SplitMix64(0x5E7).fr() | (1 << 253)
assert BIG_S < O.R


@pytest.fixture(scope="module")
def random_points():
    """2^10 points with no structure the transform could exploit: k_i * G for random k_i, by the oracle, once"""
    rng = O.SplitMix64(0xFF7)
    return mul_g([rng.fr() for _ in range(1 << 10)])


@pytest.fixture(scope="module")
def one_point():
    return mul_g([O.SplitMix64(0xE8C).fr()])


# ---------------------------------------------------------------------------------------------- setup
@pytest.mark.parametrize("s", [SMALL_S, BIG_S], ids=["small", "254bit"])
@pytest.mark.parametrize("k", [0, 1, 2, 5, 9])
def test_setup_against_the_definition(eng, k, s):
    n = 1 << k
    hg, hl = eng.params_setup(k, fb(s))
    try:
        g, gl = table(eng, hg, n), table(eng, hl, n)
    finally:
        eng.bases_free(hg)
        eng.bases_free(hl)
    assert g == mul_g([pow(s, i, O.R) for i in range(n)])
    assert gl == mul_g(lagrange_dlogs(k, s))
    if k == 0:
        assert gl == G


def test_setup_refusals_leave_the_context_usable(eng, pkg):
    for k, s, code in [(3, bytes(32), pkg.ERR_INVALID),
                       (3, fb(V.omega_for_k(3)), pkg.ERR_INVALID),            # s^n == 1
                       (3, O.R.to_bytes(32, "little"), pkg.ERR_NONCANONICAL),
                       (3, b"\xff" * 32, pkg.ERR_NONCANONICAL),
                       (25, fb(SMALL_S), pkg.ERR_INVALID)]:
        with pytest.raises(pkg.H2AggError) as ei:
            eng.params_setup(k, s)
        assert ei.value.code == code, (k, s.hex())
    hg, hl = eng.params_setup(2, fb(SMALL_S))
    try:
        for k, code in [(25, pkg.ERR_INVALID), (3, pkg.ERR_INVALID)]:         # 2^3 > the table's 4 points
            with pytest.raises(pkg.H2AggError) as ei:
                eng.bases_fft(hg, k)
            assert ei.value.code == code
        with pytest.raises(pkg.H2AggError) as ei:
            eng.bases_fft(hg + 1000, 1)
        assert ei.value.code == pkg.ERR_INVALID
        assert table(eng, hl, 4) == mul_g(lagrange_dlogs(2, SMALL_S))
    finally:
        eng.bases_free(hg)
        eng.bases_free(hl)


# ---------------------------------------------------------------------------------------------- FFT against the definition
@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("k", [1, 2, 3, 6, 10])
def test_fft_against_the_definition(eng, random_points, k, inverse):
    n = 1 << k
    pts = random_points[:64 * n]
    rows = None
    if k == 10:
        rng = O.SplitMix64(0xA11 + inverse)
        rows = sorted({0, 1, n // 2, n - 1} | {rng.next() % n for _ in range(60)})
        while len(rows) < 64:
            rows = sorted(set(rows) | {rng.next() % n})
    want = oracle_fft(pts, k, inverse, rows)
    got = run_fft(eng, pts, k, inverse)
    bad = [i for i in want if got[i] != want[i]]
    assert not bad, bad[:8]


def exceptional_inputs(P, k):
    n = 1 << k
    negP = O.aff_to_bytes(O.neg(O.aff_from_bytes(P)))
    return {
        "all_equal": P * n,
        "alternating_sign": (P + negP) * (n // 2),
        "identities_at_0_1_last": ID * 2 + P * (n - 3) + ID,
        "delta": P + ID * (n - 1),
    }


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("case", ["all_equal", "alternating_sign", "identities_at_0_1_last", "delta"])
@pytest.mark.parametrize("k", [3, 7])
def test_fft_exceptional_inputs(eng, one_point, k, case, inverse):
    """P + P and P - P in the first butterflies, a + (-a), identity operands on either side of a butterfly"""
    n = 1 << k
    pts = exceptional_inputs(one_point, k)[case]
    want = oracle_fft(pts, k, inverse)
    got = run_fft(eng, pts, k, inverse)
    bad = [i for i in range(n) if got[i] != want[i]]
    assert not bad, bad[:8]
    if not inverse:
        if case == "all_equal":
            assert got[0] != ID and got[1:] == [ID] * (n - 1)       # [n * P, identity, ...]
        if case == "delta":
            assert got == [one_point] * n


# ---------------------------------------------------------------------------------------------- the two routes agree
# A stage with 2^(k-s) >= 64 butterflies per twiddle is wave-uniform; stage 1 multiplies nothing.  k = 4: per-group digits only;
# k = 7 and 8: either side of the first k with a wave-uniform stage that multiplies (stage 2: 2^(k-2) >= 64); k = 12: both
# paths over several stages
@pytest.mark.parametrize("k", [4, 7, 8, 12])
def test_fft_of_g_is_the_setups_own_g_lagrange(eng, k):
    n = 1 << k
    s = fb(BIG_S + k)
    hg, hl = eng.params_setup(k, s)
    hbig = eng.params_setup(k + 2, s)
    try:
        want = table(eng, hl, n)
        for src in (hg, hbig[0]):                                     # the second: truncated from a larger table
            o = eng.bases_fft(src, k, inverse=True)
            try:
                assert table(eng, o, n) == want
            finally:
                eng.bases_free(o)
    finally:
        for h in (hg, hl) + tuple(hbig):
            eng.bases_free(h)


# ---------------------------------------------------------------------------------------------- a size the oracle does not reach
def test_round_trip_and_interpolation_at_k14(eng):
    k = 14
    n = 1 << k
    rng = O.SplitMix64(0x14C)
    import torch
    ks = b"".join(fb(rng.fr()) for _ in range(n))
    d_k = torch.frombuffer(bytearray(ks), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    hx = eng.bases_generate(d_k.data_ptr(), n)
    hf = eng.bases_fft(hx, k, inverse=False)
    hb = eng.bases_fft(hf, k, inverse=True)
    try:
        assert table(eng, hb, n) == table(eng, hx, n)
    finally:
        for h in (hx, hf, hb):
            eng.bases_free(h)
    s = rng.fr()
    hg, hl = eng.params_setup(k, fb(s))
    try:
        g = split(table(eng, hg, n))
        aff = lambda jac: eng.g1_batch_to_affine(jac)
        assert aff(eng.g1_msm_preloaded(hl, fb(1) * n)) == g[0]                     # sum_i L_i = 1
        w = V.omega_for_k(k)
        for j in [rng.next() % n for _ in range(8)]:                                  # sum_i w^(ij) L_i(s) = s^j
            wj, cur, sc = pow(w, j, O.R), 1, []
            for _ in range(n):
                sc.append(fb(cur))
                cur = cur * wj % O.R
            assert aff(eng.g1_msm_preloaded(hl, b"".join(sc))) == g[j], j
    finally:
        eng.bases_free(hg)
        eng.bases_free(hl)


# ---------------------------------------------------------------------------------------------- used for what it is for
def test_instance_commitment_over_the_device_made_table(eng):
    k, s = 6, BIG_S
    rng = O.SplitMix64(0x1C6)
    inst = [rng.fr() for _ in range(11)]
    _hg, hl = eng.params_setup(k, fb(s))
    try:
        got = eng.g1_batch_to_affine(eng.instance_commitment(hl, b"".join(fb(v) for v in inst), (1 << k) - 6))
    finally:
        eng.bases_free(_hg)
        eng.bases_free(hl)
    L = lagrange_dlogs(k, s)
    assert got == mul_g([sum(v * l for v, l in zip(inst, L))])


def test_params_files_and_a_toy_proof_over_them(eng, pkg):
    """fs.setup_params / fs.downsize_params through write_params / read_params / upload_g_lagrange / pairing_g2 unchanged;
    a toy proof made for the same trapdoor verifies against the device-made table and s_g2, a changed instance does not"""
    from tests.test_verifier_pipeline import SHAPES, make_batch
    fs = importlib.import_module(entry.PKG_NAME + ".fs")
    ver = importlib.import_module(entry.PKG_NAME + ".verifier")
    # k = 3: both builders give the same file content, and it survives the round trip
    s3 = fb(BIG_S)
    p5, p3 = fs.setup_params(eng, 5, s3), fs.setup_params(eng, 3, s3)
    d3 = fs.downsize_params(eng, p5, 3)
    for p in (p3, d3):
        b = fs.write_params(p)
        assert fs.write_params(fs.read_params(b)) == b
    assert fs.write_params(d3) == fs.write_params(p3)
    assert p3.g == b"".join(O.compress(O.scalar_mul(pow(BIG_S, i, O.R), O.G1)) for i in range(8))
    # the toy batch's trapdoor: make_batch draws tau first from the seed's generator
    seed = 0x51
    setup, circuits = make_batch(seed, [SHAPES[0]], 1)
    params = fs.read_params(fs.write_params(fs.setup_params(eng, setup.k, fb(setup.tau))))
    assert params.g_lagrange[:32 * 16] == b"".join(O.compress(p) for p in setup.g_lagrange)
    h = fs.upload_g_lagrange(eng, params)
    s_g2, g2 = fs.pairing_g2(eng, params)
    c = circuits[0]
    vk = ver.VerifyingKey(eng, ver.encode_vk(c.cs, O.aff_to_bytes))
    try:
        inst, data = c.proofs[0]
        cols = [b"".join(fb(v) for v in col) for col in inst[0]]
        rec = ver.verify_proofs(eng, [(vk, c.name, h, [(cols, data)])], s_g2, g2)[0]
        assert rec[2] == pkg.OK and rec[3] is True
        changed = [fb(inst[0][0][0] + 1) + cols[0][32:]] + cols[1:]
        rec = ver.verify_proofs(eng, [(vk, c.name, h, [(changed, data)])], s_g2, g2)[0]
        assert not (rec[2] == pkg.OK and rec[3] is True)
    finally:
        vk.close()
        eng.bases_free(h)
