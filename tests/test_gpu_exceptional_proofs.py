"""GPU: what a proof MAY hold but no random generator reaches, through every layer that reads proof bytes — coordinates in
[r, p) (the subtracting branch of the device's reduction mod r), the identity inside a proof and inside a key, equal / opposite
/ copied commitments, a proof repeated in a batch, evaluations and instance values that are all 0, 1 or r - 1, and kept
recordings (csrc/verifier.inc `AggPlan`) refilled across such proofs.  The inputs are tests/exceptional_points.py's; every
expected value is the oracle's (oracle/verifier.py over the C restatement's multi_exp), bit for bit, on rejected proofs too;
tests/test_exceptional_points_host.py shows on the CPU that the oracle tells these inputs apart.

  first part    element and wire level: transcript_read_batch, hash_transcript_read_batch, decompress / compress, to_affine, add
  second part   h2agg_verify_aggregation (both sponge backends), h2agg_verify_proofs (seg_chunk 0 and 500), ShaRead keys, the
                sharded call
  third part    recordings: ordinary first and exceptional first, against plan_cache 0"""
import copy
import importlib

import pytest

import __graft_entry__ as entry
from oracle import bn254 as O
from oracle import schema as S
from oracle import verifier as V
from tests import exceptional_points as X
from tests import toy_prover_hash as TH
from tests.test_exceptional_points_host import NPROOFS, SCRIPT, SEED, placement, scripted_proofs
from tests.test_gpu_hash_transcript import Product as HashProduct
from tests.test_gpu_sharded import run_threads
from tests.test_gpu_verifier import run_product
from tests.test_gpu_verify_each import Product, fold, oracle_pairs
from tests.test_hash_transcript_host import reference
from tests.test_verifier_pipeline import SHAPES, make_batch
from tests.util import CEccChip

pytestmark = pytest.mark.gpu
KINDS = ["sha256", "keccak256"]


@pytest.fixture
def ver():
    return importlib.import_module(entry.PKG_NAME + ".verifier")


def fe(xs):
    return b"".join(O.fe_to_bytes(x) for x in xs)


def aff(pts):
    return b"".join(O.aff_to_bytes(p) for p in pts)


# ---- first part: elements and wire -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scripted():
    return scripted_proofs()


@pytest.mark.parametrize("backend", ["device", "host"])
def test_poseidon_reader_with_crafted_points(eng, scripted, backend):
    """every crafted point at an external slot and at a proof slot, over proofs 0, 3, 4 and 5 of 6 (PSD_PER_BLOCK = 4)"""
    vk_scalar, proofs, ext, want_pts, want_ch = scripted
    assert len(proofs) == NPROOFS == 6 and {k[0] for k in placement()} == {0, 3, 4, 5}
    try:
        eng.transcript_configure(backend)
        got_pts, got_ch = eng.transcript_read_batch(proofs, SCRIPT, O.fe_to_bytes(vk_scalar), b"".join(aff(x) for x in ext))
    finally:
        eng.transcript_configure("auto")
    assert got_pts == [aff(p) for p in want_pts]
    assert got_ch == [fe(c) for c in want_ch]


def test_sponge_refuses_an_unreduced_coordinate(eng, pkg):
    """x = r + 2 absorbed as it is: the sponge wants canonical elements, so a reader that skipped the reduction would fail"""
    for v in (X.X_R[0], X.Y_TOP[1]):
        with pytest.raises(pkg.H2AggError) as ei:
            eng.poseidon_squeeze_batch(O.fe_to_bytes(v), 1, [1])
        assert ei.value.code == pkg.ERR_NONCANONICAL


HASH_SCRIPT = "CXXXXPPQPQQPPPQSSSSSQPPPPQQ"


@pytest.fixture(scope="module")
def hash_proofs():
    """65 ShaRead proofs (one past an interleaving group); the ten crafted non-identity points fill the P slots of proofs 0, 63
    and 64 (rotated) and their X slots"""
    rng = O.SplitMix64(0x5AE)
    pool = [TH.g1_mul(rng.fr()) for _ in range(32)]
    crafted = list(X.NON_IDENTITY.values())
    assert len(crafted) == 10 == HASH_SCRIPT.count("P")
    consts = [rng.fr()]
    proofs, exts = [], []
    for i in range(65):
        rot = {0: 0, 63: 3, 64: 7}.get(i)
        out, k = bytearray(), 0
        for ch in HASH_SCRIPT:
            if ch == "P":
                out += O.aff_to_bytes(pool[rng.next() % 32] if rot is None else crafted[(k + rot) % 10])
                k += 1
            elif ch == "S":
                out += O.fe_to_bytes(rng.fr())
        proofs.append(bytes(out))
        exts.append([pool[rng.next() % 32] if rot is None else crafted[(4 * [0, 63, 64].index(i) + j) % 10] for j in range(4)])
    assert {O.aff_to_bytes(p) for i in (0, 63, 64) for p in exts[i]} == {O.aff_to_bytes(p) for p in crafted}
    return proofs, consts, exts


@pytest.mark.parametrize("kind", KINDS)
def test_hash_reader_with_crafted_points(eng, pkg, hash_proofs, kind):
    proofs, consts, exts = hash_proofs
    want_pts, want_ch, _lens = reference(kind, HASH_SCRIPT, proofs, consts, exts)
    xb = b"".join(aff(x) for x in exts)
    try:
        for backend in ("device", "host"):
            eng.transcript_configure(backend)
            got_pts, got_ch = eng.hash_transcript_read_batch(kind, proofs, HASH_SCRIPT, fe(consts), xb)
            assert got_pts == want_pts, backend
            assert got_ch == want_ch, backend
            # the identity stays refused: as a proof point and as an external point, in the proofs that hold the crafted ones
            for k in (0, 63, 64):
                bad = list(proofs)
                bad[k] = bytes(64) + bad[k][64:]
                with pytest.raises(pkg.BadPoint):
                    eng.hash_transcript_read_batch(kind, bad, HASH_SCRIPT, fe(consts), xb)
                bx = bytearray(xb)
                bx[64 * (4 * k + 3):64 * (4 * k + 4)] = bytes(64)
                with pytest.raises(pkg.BadPoint):
                    eng.hash_transcript_read_batch(kind, proofs, HASH_SCRIPT, fe(consts), bytes(bx))
    finally:
        eng.transcript_configure("auto")


def test_decompress_and_compress(eng):
    pts = list(X.CRAFTED.values())
    wire = b"".join(O.compress(p) for p in pts)
    out, ok = eng.g1_batch_decompress(wire, with_ok=True)
    assert ok == bytes([1]) * len(pts)
    assert out == aff(pts)
    assert eng.g1_batch_compress(aff(pts)) == wire


def test_to_affine_and_add(eng):
    rng = O.SplitMix64(0xADD)
    pts = list(X.CRAFTED.values())
    n = len(pts)
    jac = lambda ps: b"".join(O.jac_to_bytes(p, rng.fr()) for p in ps)
    assert eng.g1_batch_to_affine(jac(pts)) == aff(pts)
    assert eng.g1_batch_to_affine(b"".join(O.jac_to_bytes(p) for p in pts)) == aff(pts)
    for what, other in (("P + P", pts), ("P - P", [O.neg(p) for p in pts]), ("P + 0", [O.INF] * n), ("P + G", [O.G1] * n)):
        want = aff([O.add(a, b) for a, b in zip(pts, other)])
        got = eng.g1_batch_add(jac(pts), jac(other))
        assert b"".join(O.aff_to_bytes(O.jac_from_bytes(got[96 * i:96 * i + 96])) for i in range(n)) == want, what
        got = eng.g1_batch_add(jac(other), jac(pts))
        assert b"".join(O.aff_to_bytes(O.jac_from_bytes(got[96 * i:96 * i + 96])) for i in range(n)) == want, what
    got = eng.g1_batch_add(jac(pts), jac(pts), subtract=True)
    assert all(O.jac_from_bytes(got[96 * i:96 * i + 96]) is O.INF for i in range(n))


# ---- second part: the from-bytes verifier ------------------------------------------------------------------------------
_CACHE = {}


def poseidon_case(name):
    """-> (setup, circuit, touched, accepted, expected): the variant's circuit and the oracle's results, made once per module:
    expected = (pair, lambda, advice commitments, per-proof pairs)"""
    if "batch" not in _CACHE:
        _CACHE["batch"] = make_batch(SEED, [SHAPES[0]], 4)
    if name not in _CACHE:
        if name == "identity_key":
            setup, (c,) = X.identity_key_batch(SEED + 7, SHAPES[0])
            touched, accepted = set(), True
        else:
            setup, (base,) = _CACHE["batch"]
            c = X.apply_variant(name, base)
            _fn, touched, accepted = X.VARIANTS[name]
        _CACHE[name] = (setup, c, touched, accepted, oracle_aggregation([c]) + (oracle_pairs([c], CEccChip),))
    return _CACHE[name]


def oracle_aggregation(circuits):
    left, right, _plain, commits, lam = V.verify_aggregation_proofs_in_chip(CEccChip(), circuits)
    return S.final_pair_bytes(left, right), O.fe_to_bytes(lam), [[O.aff_to_bytes(p) for p in per] for per in commits]


ALL_VARIANTS = list(X.VARIANTS) + ["identity_key"]


@pytest.mark.parametrize("backend", ["device", "host"])
@pytest.mark.parametrize("name", ALL_VARIANTS)
def test_aggregation_matches_the_oracle(eng, ver, name, backend):
    setup, c, _touched, accepted, (want_pair, want_lam, want_commits, _each) = poseidon_case(name)
    prod = Product(eng, ver, setup, [c])
    try:
        eng.transcript_configure(backend)
        left, right, lam, ok, commits = ver.verify_aggregation(eng, prod.arg, *prod.g2, with_commits=True)
    finally:
        eng.transcript_configure("auto")
        prod.close()
    assert lam == want_lam
    assert left + right == want_pair
    assert commits == want_commits
    assert ok is accepted


@pytest.mark.parametrize("seg_chunk", [0, 500])
@pytest.mark.parametrize("name", ALL_VARIANTS)
def test_each_proof_matches_the_oracle(eng, ver, name, seg_chunk):
    setup, c, touched, _accepted, (want_pair, want_lam, _commits, want_each) = poseidon_case(name)
    prod = Product(eng, ver, setup, [c])
    try:
        eng.debug_configure("seg_chunk", seg_chunk)
        got = prod.each()
    finally:
        eng.debug_configure("seg_chunk", 0)
        prod.close()
    n = len(c.proofs)
    assert [r[0] + r[1] for r in got] == want_each
    assert [r[2] for r in got] == [0] * n
    assert [r[3] for r in got] == [i not in touched for i in range(n)]
    assert fold(got, O.fe_from_bytes(want_lam)) == want_pair


@pytest.mark.parametrize("kind", KINDS)
def test_hash_transcript_keys(eng, pkg, ver, kind):
    """ShaRead proofs (64-byte points, no reduction mod r): big coordinates, dependent points and a repeated proof are priced
    as the oracle prices them; the identity is the reader's refusal, named for that proof alone"""
    setup, (base,) = TH.make_batch(0x5E0 + len(kind), [SHAPES[0]], 4, kind)
    for name in ("big_coordinates", "dependent_points", "repeated_proof", "identities"):
        _fn, touched, _accepted = X.VARIANTS[name]
        c = X.apply_variant(name, base, point_bytes=64)
        refused = touched if name == "identities" else set()
        want = [None if i in refused else S.final_pair_bytes(*TH.oracle_pair(c, i, kind, fast=True)) for i in range(4)]
        prod = HashProduct(eng, ver, setup, [c], [kind])
        try:
            got = prod.each()
        finally:
            prod.close()
        for i, rec in enumerate(got):
            if i in refused:
                assert rec[2] == pkg.ERR_BAD_POINT and rec[3] is False, (name, i)
            else:
                assert rec[0] + rec[1] == want[i] and rec[2] == 0 and rec[3] is (i not in touched), (name, i)


@pytest.mark.parametrize("backend", ["device", "host"])
def test_sharded_call_with_big_coordinates_and_identities(eng, pkg, backend):
    """the four proofs of the big-coordinate variant and the four of the identity variant as one batch of eight over two ranks"""
    setup, c1, _t, _a, _e = poseidon_case("big_coordinates")
    c2 = poseidon_case("identities")[1]
    c = copy.copy(c1)
    c.proofs = list(c1.proofs) + list(c2.proofs)
    eng.transcript_configure(backend)
    try:
        want = run_product(pkg, eng, setup, [c])
    finally:
        eng.transcript_configure("auto")
    want_pair, want_lam, _commits = oracle_aggregation([c])
    assert (want[0] + want[1], want[2], want[3]) == (want_pair, want_lam, False)
    for rank, res in enumerate(run_threads(pkg, setup, [c], 2, backend)):
        assert res == want, "rank %d differs from the one-context aggregation" % rank


# ---- third part: recordings ----------------------------------------------------------------------------------------------
def pair_of(name, i, j):
    """two proofs of a variant (or of the ordinary batch) as a circuit of their own, with the oracle's aggregation"""
    key = ("pair", name, i, j)
    if key not in _CACHE:
        setup, c = (_CACHE["batch"][0], _CACHE["batch"][1][0]) if name == "ordinary" else poseidon_case(name)[:2]
        c2 = copy.copy(c)
        c2.proofs = [c.proofs[i], c.proofs[j]]
        _CACHE[key] = (c2, oracle_aggregation([c2]))
    return _CACHE[key]


@pytest.mark.parametrize("order", ["ordinary_first", "exceptional_first"])
def test_recordings_are_refilled_across_exceptional_proofs(eng, ver, order):
    """"the recording is good whatever this call's VALUES were" (csrc/verify_run.inc): a recording made from ordinary proofs
    serves proofs with identities and big coordinates, and one made from proofs with identities in them serves ordinary,
    dependent and flat-evaluation proofs — every result the oracle's, and the bytes of the same calls with plan_cache 0"""
    poseidon_case("identities")
    calls = {"ordinary_first": [("ordinary", 0, 1), ("identities", 1, 2), ("ordinary", 2, 3), ("big_coordinates", 1, 2)],
             "exceptional_first": [("identities", 1, 3), ("ordinary", 0, 1), ("dependent_points", 2, 3),
                                   ("flat_evaluations", 1, 2)]}[order]
    cases = [pair_of(*call) for call in calls]
    setup = _CACHE["batch"][0]
    cached, fresh = [], []
    prod = Product(eng, ver, setup, [cases[0][0]])          # a NEW key of the same description: its first call records
    vk, _name, table, _proofs = prod.arg[0]

    def run(c):
        proofs = [([fe(col) for col in inst[0]], data) for inst, data in c.proofs]
        return ver.verify_aggregation(eng, [(vk, c.name, table, proofs)], *prod.g2, with_commits=True)
    try:
        h0, m0, _ = eng.verify_plan_stats()
        for k, (c, _want) in enumerate(cases):
            cached.append(run(c))
            h, m, _ = eng.verify_plan_stats()
            assert (h - h0, m - m0) == (k, 1), calls[k]      # recorded by the first call, reused by every later one
        eng.debug_configure("plan_cache", 0)
        try:
            for c, _want in cases:
                fresh.append(run(c))
            assert eng.verify_plan_stats()[:2] == (h, m)
        finally:
            eng.debug_configure("plan_cache", 1)
    finally:
        prod.close()
    for call, (c, (want_pair, want_lam, want_commits)), got, twin in zip(calls, cases, cached, fresh):
        left, right, lam, ok, commits = got
        assert (left + right, lam, commits) == (want_pair, want_lam, want_commits), call
        assert ok is (call[0] == "ordinary"), call
        assert twin == got, call
