"""CPU: the crafted inputs of tests/exceptional_points.py are what they claim to be, the oracle distinguishes them (a transcript
whose reduction mod r of a point coordinate yields any other element squeezes OTHER challenges: without that, the GPU
comparison could pass on a product that reduces wrongly), and the oracle verifier prices every variant of
tests/test_gpu_exceptional_proofs.py without raising — where a reader refuses a proof, which refusal it is."""
import pytest

from oracle import bn254 as O
from oracle import pairing as E
from oracle import poseidon as P
from oracle import schema as S
from oracle import verifier as V
from tests import exceptional_points as X
from tests import hash_transcript_ref as H
from tests import toy_prover_hash as TH
from tests.test_verifier_pipeline import SHAPES, make_batch
from tests.util import CEccChip


def test_roots():
    rng = O.SplitMix64(0xCB27)
    for _ in range(20):
        a = rng.fr()
        assert pow(X.fq_cbrt(pow(a, 3, O.P)), 3, O.P) == pow(a, 3, O.P)
        assert X.fq_sqrt(a * a) in (a % O.P, O.P - a % O.P)
    assert X.fq_cbrt(2) is None or pow(X.fq_cbrt(2), 3, O.P) == 2
    assert X.fq_sqrt(O.P - 1) is None                      # p = 3 mod 4


def test_crafted_points_are_what_they_claim():
    r, p = O.R, O.P
    assert X.X_R[0] == r + 2 and X.point_with_x(r + 5) and X.point_with_x(r + 8)
    assert not any(X.point_with_x(x) for x in (r, r + 1, r + 3, r + 4, r + 6, r + 7))
    assert X.X_TOP[0] == p - 1
    assert X.Y_R[1] == r + 1 and X.point_with_y(r + 2) and X.point_with_y(r + 3)
    assert X.point_with_y(r) is None
    assert X.Y_TOP[1] == p - 1
    for name, pt in X.CRAFTED.items():
        assert O.is_on_curve(pt), name
        if pt is not O.INF:
            assert 0 <= pt[0] < p and 0 <= pt[1] < p, name
            assert not (pt[0] >= r and pt[1] >= r), name
        assert O.decompress(O.compress(pt)) == pt, name
        assert O.aff_from_bytes(O.aff_to_bytes(pt)) == pt, name
    for name in ("X_R", "X_TOP"):
        assert X.CRAFTED[name][0] >= r and X.CRAFTED["-" + name][0] >= r
        assert X.CRAFTED[name][1] < r and X.CRAFTED["-" + name][1] < r
        assert O.compress(X.CRAFTED[name])[31] >> 7 != O.compress(X.CRAFTED["-" + name])[31] >> 7
    for name in ("Y_R", "Y_TOP"):
        assert X.CRAFTED[name][1] >= r and X.CRAFTED[name][0] < r
        assert X.CRAFTED["-" + name][1] <= p - r                       # a small y
        assert O.compress(X.CRAFTED[name])[31] >> 7 != O.compress(X.CRAFTED["-" + name])[31] >> 7
    assert len({O.compress(pt) for pt in X.CRAFTED.values()}) == len(X.CRAFTED) == 11


def test_encode_point_reduces_the_big_coordinate():
    assert P.encode_point(X.X_R) == [2, X.X_R[1]] != list(X.X_R)
    assert P.encode_point(X.Y_R) == [X.Y_R[0], 1] != list(X.Y_R)
    assert P.encode_point(X.X_TOP) == [O.P - 1 - O.R, X.X_TOP[1]]
    assert P.encode_point(O.neg(X.Y_R)) == list(O.neg(X.Y_R))          # its y is small: nothing to reduce


# the script of tests/test_gpu_poseidon.py with three external points, and the placement the GPU test uses:
# (proof, "X", index) or (proof, P index) -> point name
SCRIPT = "CXXX" + "PPP" + "Q" + "PP" + "QQ" + "PPPP" + "Q" + "PP" + "Q" + "SSSSSSSSSSS" + "Q" + "PPP" + "Q" + "Q"
NPROOFS = 6
NX = SCRIPT.count("X")


def placement():
    """every crafted point at an X slot and at a P slot, spread over proofs 0, 3, 4 and 5 (PSD_PER_BLOCK = 4: proofs 3 and 4
    straddle a workgroup, proof 5 sits in a partial one); proofs 1 and 2 hold random points only"""
    names = list(X.CRAFTED)
    where = {}
    homes = [0, 3, 4, 5]
    npts = SCRIPT.count("P")
    for i, name in enumerate(names):
        where[(homes[i % 4], 1 + (3 * i) % (npts - 1))] = name        # P slots 1.. (slot 0 keeps a random point in proof 0)
    for i, name in enumerate(names):
        where[(homes[i % 4], "X", i // 4)] = name
    return where


def scripted_proofs(writer_cls=P.PoseidonTranscriptWrite):
    """-> (vk_scalar, proofs, ext points, want points, want challenges) of the script above, written by the oracle"""
    rng = O.SplitMix64(0xE7C)
    vk_scalar = rng.fr()
    where = placement()
    proofs, ext, want_pts, want_ch = [], [], [], []
    for i in range(NPROOFS):
        w = writer_cls()
        inst = [X.CRAFTED[where[(i, "X", j)]] if (i, "X", j) in where else TH.g1_mul(rng.fr()) for j in range(NX)]
        pts, ch, nx = [], [], 0
        for op in SCRIPT:
            if op == "C":
                w.common_scalar(vk_scalar)
            elif op == "X":
                w.common_point(inst[nx])
                nx += 1
            elif op == "P":
                key = (i, len(pts))
                p = X.CRAFTED[where[key]] if key in where else TH.g1_mul(rng.fr())
                w.write_point(p)
                pts.append(p)
            elif op == "S":
                w.write_scalar(rng.fr())
            else:
                ch.append(w.squeeze_challenge_scalar())
        proofs.append(w.finalize())
        ext.append(inst)
        want_pts.append(pts)
        want_ch.append(ch)
    return vk_scalar, proofs, ext, want_pts, want_ch


def read_script(reader, vk_scalar, inst):
    reader.common_scalar(vk_scalar)
    for p in inst:
        reader.common_point(p)
    pts, ch = [], []
    for op in SCRIPT[1 + NX:]:
        if op == "P":
            pts.append(reader.read_point())
        elif op == "S":
            reader.read_scalar()
        else:
            ch.append(reader.squeeze_challenge_scalar())
    return pts, ch


def reader_with_encoding(encode):
    """PoseidonTranscriptRead whose point encoding maps a coordinate through `encode` (an integer, absorbed as it is)"""
    class Reader(P.PoseidonTranscriptRead):
        def common_point(self, pt):
            self.hash.absorbing.extend([0, 0] if pt is None else [encode(pt[0]), encode(pt[1])])
    return Reader


def test_placement_covers_every_point_twice():
    where = placement()
    assert {k[0] for k in where} == {0, 3, 4, 5}
    at_p = [n for k, n in where.items() if len(k) == 2]
    at_x = [n for k, n in where.items() if len(k) == 3]
    assert sorted(at_p) == sorted(at_x) == sorted(X.CRAFTED)
    assert all(k[2] < NX for k in where if len(k) == 3)
    assert all(where[(h, "X", 0)] in X.BIG for h in (0, 3, 4, 5))     # a big coordinate in front of every first squeeze


def test_challenges_change_without_the_reduction():
    """What a reduction that is wrong does to the challenges, through local readers (oracle/ is not edited).

    Leaving `% R` out of the oracle's encode_point alone changes nothing HERE: the sponge is arithmetic in Fr, and x and x mod r
    are one field element.  On the device they are not one thing: the sponge kernels refuse an element >= r (FLAG_NONCANONICAL;
    tests/test_gpu_exceptional_proofs.py checks that refusal at r + 2), so a product that skips the reduction fails the GPU
    comparison with an error.  A reduction that yields ANOTHER element must change the challenges, which is shown here for the
    two ways the device's routine (subtract r, keep the difference unless it is negative) can go wrong:
      wrong_sign   the difference kept for a coordinate < r too (it wraps mod 2^256): every proof's challenges change
      lost_borrow  the difference off by 2^32 in the subtracting branch: the challenges change exactly where a proof holds a
                   coordinate >= r, from the first squeeze on"""
    vk_scalar, proofs, ext, want_pts, want_ch = scripted_proofs()
    where = placement()
    omitted = reader_with_encoding(lambda a: a)
    wrong_sign = reader_with_encoding(lambda a: (a - O.R) % (1 << 256))
    lost_borrow = reader_with_encoding(lambda a: a - O.R + (1 << 32) if a >= O.R else a)
    nbig = 0
    for i in range(NPROOFS):
        pts, ch = read_script(P.PoseidonTranscriptRead(proofs[i]), vk_scalar, ext[i])
        assert (pts, ch) == (want_pts[i], want_ch[i]), i
        assert read_script(omitted(proofs[i]), vk_scalar, ext[i]) == (pts, ch)
        pts2, ch2 = read_script(wrong_sign(proofs[i]), vk_scalar, ext[i])
        assert pts2 == pts and all(a != b for a, b in zip(ch2, ch)), i
        pts3, ch3 = read_script(lost_borrow(proofs[i]), vk_scalar, ext[i])
        big = any(X.CRAFTED[n] is not None and max(X.CRAFTED[n]) >= O.R for k, n in where.items() if k[0] == i)
        nbig += big
        assert pts3 == pts and (ch3 != ch) == big, i
        if big:
            assert all(a != b for a, b in zip(ch3, ch)), i             # the X slot holds one: from the first squeeze on
    assert nbig == 4


# ---- the verifier ------------------------------------------------------------------------------------------------------
SEED = 0xE9C


@pytest.fixture(scope="module")
def batch():
    return make_batch(SEED, [SHAPES[0]], 4)


def accepted(setup, left, right):
    """e(left, [tau]_2) = e(right, [1]_2) iff tau * left = right (a non-degenerate pairing on groups of prime order r): with
    the trapdoor this costs one scalar multiplication by the C oracle, not two Miller loops in Python"""
    return TH.CrefEccChip().scalar_mul(None, setup.tau, left) == right


def test_the_trapdoor_verdict_is_the_pairing_verdict(batch):
    setup, (c,) = batch
    good = single_pair(c, 0)
    bad = single_pair(X.apply_variant("identities", c), 1)
    for (left, right), want in ((good, True), (bad, False)):
        assert accepted(setup, left, right) is want
        assert E.pairing_check([(left, setup.s_g2), (right, E.g2_neg(setup.g2))]) is want


def single_pair(c, i, reader=P.PoseidonTranscriptRead):
    inst, data = c.proofs[i]
    pchip, ctx = CEccChip(), S.OracleCtx()
    _plain, commitments = V.assign_instance_commitment(pchip, ctx, inst, c.cs, c.g_lagrange)
    proof, _adv, _vp = V.verify_single_proof_no_eval(reader(data), pchip, ctx, commitments, c.cs, "%s_p%d" % (c.name, i))
    left, right, _names = S.evaluate_multiopen_proof(ctx, S.OracleFieldChip(), pchip, proof)
    return left, right


def test_layout_names_the_slots_the_oracle_reads(batch):
    _setup, (c,) = batch
    data = c.proofs[0][1]
    lay = X.ProofLayout(c.cs, len(data))
    vp = V.build_params(P.PoseidonTranscriptRead(data), S.OracleEccChip(), S.OracleCtx(), [[O.INF]], c.cs, "k")
    rd = lambda slot: X.read_point(data, slot)
    assert [rd(s) for s in lay.advice] == vp.advice_commitments[0]
    assert [rd(s) for s in lay.permutation_products] == [st[0] for st in vp.permutation_sets[0]]
    assert [rd(s) for s in lay.lookup_products] == [lk["product_commitment"] for lk in vp.lookups[0]]
    assert rd(lay.random) == vp.random_commitment
    assert [rd(s) for s in lay.vanishing] == vp.vanish_commitments
    assert [rd(s) for s in lay.w] == vp.w and len(vp.w) == 4
    assert O.fe_from_bytes(data[lay.evals_at:lay.evals_at + 32]) == vp.instance_evals[0][0]
    last = lay.evals_at + 32 * (lay.n_evals - 1)
    assert O.fe_from_bytes(data[last:last + 32]) == vp.lookups[0][-1]["permuted_table_eval"]
    assert len(lay.permutation_products) == 2 and len(lay.lookup_products) == 1


@pytest.mark.parametrize("name", list(X.VARIANTS))
def test_oracle_prices_every_variant(batch, name):
    """no variant makes the oracle raise: the product owes the oracle's pair, status 0 everywhere.  The aggregation's verdict
    and every proof's own verdict are the ones tests/exceptional_points.py states."""
    setup, (c,) = batch
    _fn, touched, agg_accepted = X.VARIANTS[name]
    v = X.apply_variant(name, c)
    assert len(v.proofs) == 4
    left, right, _plain, _commits, _lam = V.verify_aggregation_proofs_in_chip(CEccChip(), [v])
    assert left is not O.INF and right is not O.INF
    assert accepted(setup, left, right) is agg_accepted
    for i in range(4):
        l, r = single_pair(v, i)
        assert accepted(setup, l, r) is (i not in touched), i
    if name != "repeated_proof":
        assert [v.proofs[i] == c.proofs[i] for i in range(4)] == [i not in touched for i in range(4)]


def test_oracle_accepts_a_key_that_holds_the_identity():
    setup, (c,) = X.identity_key_batch(SEED + 7, SHAPES[0])
    assert c.cs.fixed_commitments[0] is O.INF and c.cs.permutation_commitments[-1] is O.INF
    assert c.cs.fixed_commitments[1] is not O.INF
    left, right, *_ = V.verify_aggregation_proofs_in_chip(CEccChip(), [c])
    assert accepted(setup, left, right)
    for i in range(2):
        assert accepted(setup, *single_pair(c, i))
    # the identity is what the proofs were made for: with any other point there the pairing fails
    c.cs.fixed_commitments[0] = O.G1
    left, right, *_ = V.verify_aggregation_proofs_in_chip(CEccChip(), [c])
    assert not accepted(setup, left, right)


@pytest.mark.parametrize("kind", ["sha256", "keccak256"])
def test_hash_transcript_variants(kind):
    """ShaRead proofs: big coordinates, dependent points and a repeated proof are priced; the identity (64 zero bytes, off the
    curve) is refused by the READER — "invalid point encoding in proof", the product's H2AGG_ERR_BAD_POINT — as an advice
    commitment, as a product commitment and as a W point (there the reference's `while let Ok(..)` ends the W list early and
    the count check fails: the cause is the same refusal)"""
    setup, (c,) = TH.make_batch(0x5E0 + len(kind), [SHAPES[0]], 4, kind)
    reader = H.READERS[kind]
    for name in ("big_coordinates", "dependent_points", "repeated_proof"):
        _fn, touched, _acc = X.VARIANTS[name]
        v = X.apply_variant(name, c, point_bytes=64)
        for i in range(4):
            assert accepted(setup, *single_pair(v, i, reader)) is (i not in touched), (name, i)
    v = X.apply_variant("identities", c, point_bytes=64)
    assert accepted(setup, *single_pair(v, 0, reader))
    for i in (1, 2):
        with pytest.raises(H.TranscriptError, match="invalid point encoding"):
            single_pair(v, i, reader)
    with pytest.raises(AssertionError):
        single_pair(v, 3, reader)
    lay = X.ProofLayout(c.cs, len(c.proofs[0][1]), 64)
    rd = reader(v.proofs[3][1])
    rd.pos = lay.w[-1][0]
    with pytest.raises(H.TranscriptError, match="invalid point encoding"):
        rd.read_point()
