"""GPU: per-proof verification of a batch (h2agg_verify_proofs: verify_single_proof_in_chip, verify.rs:779-833, for every
proof in one call) and the segmented multi_exp underneath it (h2agg_g1_msm_segmented).

Every proof's (left, right) must equal the oracle's verify_single_proof_no_eval + evaluate_multiopen_proof bit for bit; the
aggregation's pair must be the lambda-weighted sum of the per-proof pairs (evaluation is linear); a bad proof is named by its
own status or verdict while the others still verify."""
import importlib

import pytest

import __graft_entry__ as entry
from oracle import bn254 as O
from oracle import schema as S
from oracle import verifier as V
from tests.test_pairing_capi import g2b
from tests.test_verifier_pipeline import SHAPES, make_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["device", "host"])
def backend(request, eng):
    """both sponge backends (h2agg_transcript_configure): the device kernel and the host worker threads"""
    eng.transcript_configure(request.param)
    yield request.param
    eng.transcript_configure("auto")


@pytest.fixture
def ver():
    return importlib.import_module(entry.PKG_NAME + ".verifier")


class Product:
    """the product's view of a toy batch: verifying keys, one g_lagrange table, the circuits argument of verify_*"""

    def __init__(self, eng, ver, setup, circuits):
        self.eng, self.ver = eng, ver
        self.table = eng.bases_upload(b"".join(O.aff_to_bytes(p) for p in setup.g_lagrange))
        self.vks = [ver.VerifyingKey(eng, ver.encode_vk(c.cs, O.aff_to_bytes)) for c in circuits]
        self.g2 = (g2b(setup.s_g2), g2b(setup.g2))
        self.arg = []
        for vk, c in zip(self.vks, circuits):
            proofs = [([b"".join(O.fe_to_bytes(v) for v in col) for col in inst[0]], data) for inst, data in c.proofs]
            self.arg.append((vk, c.name, self.table, proofs))

    def each(self, arg=None):
        return self.ver.verify_proofs(self.eng, arg or self.arg, *self.g2)

    def aggregate(self, arg=None):
        return self.ver.verify_aggregation(self.eng, arg or self.arg, *self.g2)

    def close(self):
        for vk in self.vks:
            vk.close()
        self.eng.bases_free(self.table)


def oracle_pairs(circuits, chip=S.OracleEccChip):
    """verify_single_proof_in_chip per proof: (left, right) as 128 bytes; chip: the MockEccChip restatement to run it over"""
    out = []
    for c in circuits:
        for i, (inst, data) in enumerate(c.proofs):
            pchip, ctx = chip(), S.OracleCtx()
            _plain, commitments = V.assign_instance_commitment(pchip, ctx, inst, c.cs, c.g_lagrange)
            t = V.P.PoseidonTranscriptRead(data)
            proof, _adv, _vp = V.verify_single_proof_no_eval(t, pchip, ctx, commitments, c.cs, "%s_p%d" % (c.name, i))
            left, right, _names = S.evaluate_multiopen_proof(ctx, S.OracleFieldChip(), pchip, proof)
            out.append(S.final_pair_bytes(left, right))
    return out


def fold(records, lam):
    """sum_i lam^(N-1-i) (left_i, right_i) with the oracle's group law"""
    n = len(records)
    acc_l, acc_r = O.INF, O.INF
    for i, (left, right, *_rest) in enumerate(records):
        e = pow(lam, n - 1 - i, O.R)
        acc_l = O.add(acc_l, O.scalar_mul(e, O.aff_from_bytes(left)))
        acc_r = O.add(acc_r, O.scalar_mul(e, O.aff_from_bytes(right)))
    return O.aff_to_bytes(acc_l) + O.aff_to_bytes(acc_r)


@pytest.mark.parametrize("shape_ids", [(0,), (1,), (2,), (0, 1, 2)])
def test_each_proof_matches_oracle_and_folds_to_the_aggregation(eng, ver, backend, shape_ids):
    setup, circuits = make_batch(0xE0 + len(shape_ids) * 8 + shape_ids[0], [SHAPES[i] for i in shape_ids], 2)
    prod = Product(eng, ver, setup, circuits)
    try:
        got = prod.each()
        agg_l, agg_r, lam, agg_ok = prod.aggregate()
    finally:
        prod.close()
    assert [r[0] + r[1] for r in got] == oracle_pairs(circuits)
    assert [r[2] for r in got] == [0] * len(got)
    assert [r[3] for r in got] == [True] * len(got)
    assert agg_ok is True
    assert fold(got, O.fe_from_bytes(lam)) == agg_l + agg_r


def syn_batch(eng, nproofs):
    """nproofs synthetic transcripts of the bench's EVM-like key (P = 347 queries) with a small g_lagrange table"""
    syn = importlib.import_module(entry.PKG_NAME + ".synthetic")
    ver = importlib.import_module(entry.PKG_NAME + ".verifier")
    pool = syn.point_pool(eng, 0xA66)
    comp = eng.g1_batch_compress(b"".join(pool))
    pool_c = [comp[32 * i:32 * i + 32] for i in range(len(pool))]
    shape = syn.CircuitShape(10, 300, pool)
    vk = ver.VerifyingKey(eng, ver.encode_vk(shape, lambda p: p))
    table = eng.bases_upload(b"".join(pool[i % len(pool)] for i in range(1 << 10)))
    fr = syn.fr_stream(0xBEEF)
    proofs = [([b"".join(fr() for _ in range(64))], shape.random_transcript(pool_c, 500 + i)) for i in range(nproofs)]
    return vk, table, [(vk, "syn", table, proofs)]


@pytest.mark.parametrize("seg_chunk", [700, 0])
def test_fold_identity_at_real_sizes(eng, ver, seg_chunk):
    vk, table, arg = syn_batch(eng, 48)
    try:
        eng.debug_configure("seg_chunk", seg_chunk)
        got = ver.verify_proofs(eng, arg)
        left, right, lam, _ok = ver.verify_aggregation(eng, arg)
    finally:
        eng.debug_configure("seg_chunk", 0)
        vk.close()
        eng.bases_free(table)
    assert [r[2] for r in got] == [0] * 48
    assert fold(got, O.fe_from_bytes(lam)) == left + right


def non_square_x():
    x = 5
    while pow((x ** 3 + 3) % O.P, (O.P - 1) // 2, O.P) == 1:
        x += 1
    return x


def test_one_bad_proof_among_six(eng, ver):
    setup, circuits = make_batch(0xB6, [SHAPES[0]], 6)
    want = oracle_pairs(circuits)
    prod = Product(eng, ver, setup, circuits)
    vk, name, table, proofs = prod.arg[0]

    def with_proof(k, data):
        ps = list(proofs)
        ps[k] = (ps[k][0], data)
        return [(vk, name, table, ps)]

    def others_pass(got, k):
        for i, rec in enumerate(got):
            if i != k:
                assert rec[0] + rec[1] == want[i] and rec[2] == 0 and rec[3] is True, i
    try:
        last_eval = len(proofs[0][1]) - 32 * 5          # the four W points close the transcript; the last evaluation before them
        # a changed (still canonical) evaluation: that proof's pairing fails, the aggregation of the six fails
        data = bytearray(proofs[2][1])
        v = (O.fe_from_bytes(bytes(data[last_eval:last_eval + 32])) + 1) % O.R
        data[last_eval:last_eval + 32] = O.fe_to_bytes(v)
        got = prod.each(with_proof(2, bytes(data)))
        assert [r[2] for r in got] == [0] * 6
        assert [r[3] for r in got] == [i != 2 for i in range(6)]
        others_pass(got, 2)
        assert prod.aggregate(with_proof(2, bytes(data)))[3] is False
        # a point that does not decode
        data = bytearray(proofs[4][1])
        data[0:32] = non_square_x().to_bytes(32, "little")
        got = prod.each(with_proof(4, bytes(data)))
        assert got[4][2] == entry.load_package().ERR_BAD_POINT and got[4][3] is False
        others_pass(got, 4)
        # a scalar >= r
        data = bytearray(proofs[1][1])
        data[last_eval:last_eval + 32] = O.R.to_bytes(32, "little")
        got = prod.each(with_proof(1, bytes(data)))
        assert got[1][2] == entry.load_package().ERR_NONCANONICAL and got[1][3] is False
        others_pass(got, 1)
        # a transcript of the wrong length (one W point too many for the key's rotation groups)
        got = prod.each(with_proof(5, proofs[5][1] + proofs[5][1][-32:]))
        assert got[5][2] == entry.load_package().ERR_INVALID and got[5][3] is False
        others_pass(got, 5)
    finally:
        prod.close()


@pytest.mark.parametrize("plan_cache", [1, 0])
def test_aggregation_and_per_proof_calls_do_not_share_recordings(eng, ver, plan_cache):
    setup, circuits = make_batch(0xCA, [SHAPES[0]], 2)
    want_l, want_r, _plain, _commits, want_lam = V.verify_aggregation_proofs_in_chip(S.OracleEccChip(), circuits)
    want_each = oracle_pairs(circuits)
    prod = Product(eng, ver, setup, circuits)
    try:
        eng.debug_configure("plan_cache", plan_cache)
        for _ in range(2):
            left, right, lam, ok = prod.aggregate()
            assert left + right == S.final_pair_bytes(want_l, want_r) and lam == O.fe_to_bytes(want_lam) and ok is True
            got = prod.each()
            assert [r[0] + r[1] for r in got] == want_each and all(r[3] for r in got)
    finally:
        eng.debug_configure("plan_cache", 1)
        prod.close()


@pytest.mark.parametrize("seg_chunk", [500, 0])
def test_segmented_msm_against_scalar_identity(eng, pkg, seg_chunk):
    rng = O.SplitMix64(0x5E6)
    lens = [1, 1, 5, 3, 700, 2, 17000, 40, 260, 300, 1]
    n = sum(lens)
    a = [rng.fr() for _ in range(n)]
    s = [rng.fr() for _ in range(n)]
    starts = [sum(lens[:k]) for k in range(len(lens) + 1)]
    for i in range(starts[2], starts[3]):        # a segment of zero scalars
        s[i] = 0
    for i in range(starts[3], starts[4]):        # a segment of identity bases
        a[i] = 0
    s[starts[8]] = O.R - 1
    g = O.aff_to_bytes(O.G1)
    bases = bytearray(eng.g1_batch_to_affine(eng.g1_batch_scalar_mul(g * n, b"".join(O.fe_to_bytes(x) for x in a))))
    for i in range(starts[3], starts[4]):
        bases[64 * i:64 * i + 64] = bytes(64)
    scal = b"".join(O.fe_to_bytes(x) for x in s)
    try:
        eng.debug_configure("seg_chunk", seg_chunk)
        got = eng.g1_msm_segmented(bytes(bases), scal, lens)
    finally:
        eng.debug_configure("seg_chunk", 0)
    aff = eng.g1_batch_to_affine(b"".join(got))
    for k in range(len(lens)):
        tot = sum(a[i] * s[i] for i in range(starts[k], starts[k + 1])) % O.R
        assert aff[64 * k:64 * k + 64] == O.aff_to_bytes(O.scalar_mul(tot, O.G1)), k
    with pytest.raises(pkg.EmptyMultiExp):
        eng.g1_msm_segmented(bytes(bases[:64 * 3]), scal[:32 * 3], [1, 0, 2])
    bad = bytearray(scal[:32 * 3])
    bad[32:64] = O.R.to_bytes(32, "little")
    with pytest.raises(pkg.H2AggError) as ei:
        eng.g1_msm_segmented(bytes(bases[:64 * 3]), bytes(bad), [1, 2])
    assert ei.value.code == pkg.ERR_NONCANONICAL
