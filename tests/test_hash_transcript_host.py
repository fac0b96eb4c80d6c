"""CPU: the ShaRead transcript family (halo2-snark-aggregator-api/src/transcript/sha.rs:23-232) on the library's host backend.

  * the library's own SHA-256 / Keccak-256 (csrc/hash_transcript_host.hpp) against published vectors (tests/golden/
    hash_kats.json), against hashlib / the pinned pure-Python Keccak at every message length 0..300 — every padding boundary
    of both digests included (55 / 56 / 63 / 64 mod 64; 134 / 135 / 136 mod 136);
  * the pure-Python Keccak-f[1600] of tests/hash_transcript_ref.py pinned two ways: padding 0x06 == hashlib.sha3_256, padding
    0x01 == the published Keccak-256 vectors;
  * h2agg_hash_transcript_read_batch_host against the reference reader over generated scripts, byte for byte;
  * its error mapping;
  * the test infrastructure itself: the oracle verifier accepts trapdoor proofs written with each digest under the pairing
    check and rejects them after a one-bit change.

On the padding boundaries: a transcript only ever hashes messages of 32 k + 1 bytes (blocks of 64 / 96 bytes, a 32-byte
restart, one squeeze byte), i.e. 1 or 33 mod 64 and 1 + 8 j mod 136 — the residues 55 / 56 / 63 / 0 mod 64 and 134 / 135 / 0
mod 136 cannot be produced by ANY script.  They are therefore exercised on the digest itself (h2agg_hash_digest_host, the code
the chains run), and the scripts are asserted to reach every residue class a transcript CAN reach: both classes mod 64, all
17 classes mod 136."""
import hashlib
import json
import os

import pytest

from oracle import bn254 as O
from oracle import pairing as E
from oracle import schema as S
from oracle import verifier as V
from tests import hash_transcript_ref as H
from tests import toy_prover_hash as TH
from tests.test_verifier_pipeline import SHAPES

KINDS = ["sha256", "keccak256"]
PY_DIGEST = {"sha256": lambda m: hashlib.sha256(m).digest(), "keccak256": H.keccak256}
KATS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hash_kats.json")))


def test_pure_python_keccak_is_pinned_two_ways():
    rng = O.SplitMix64(0x6EC)
    for n in list(range(0, 301, 7)) + [134, 135, 136, 137, 271, 272, 273]:
        m = bytes(rng.next() & 0xFF for _ in range(n))
        assert H.keccak_sponge256(m, 0x06) == hashlib.sha3_256(m).digest(), n
    for kat in KATS["keccak256"]:
        assert H.keccak256(kat["msg"].encode()).hex() == kat["digest"]
    for kat in KATS["sha256"]:
        assert hashlib.sha256(kat["msg"].encode()).hexdigest() == kat["digest"]


@pytest.mark.parametrize("kind", KINDS)
def test_library_digests_match_the_published_vectors(pkg, kind):
    for kat in KATS[kind]:
        assert pkg.hash_digest_host(kind, kat["msg"].encode()).hex() == kat["digest"], kat["msg"]


@pytest.mark.parametrize("kind", KINDS)
def test_library_digests_at_every_length_and_padding_boundary(pkg, kind):
    rng = O.SplitMix64(0xD16)
    seen64, seen136 = set(), set()
    for n in range(0, 301):
        m = bytes(rng.next() & 0xFF for _ in range(n))
        assert pkg.hash_digest_host(kind, m) == PY_DIGEST[kind](m), n
        seen64.add(n % 64)
        seen136.add(n % 136)
    assert {55, 56, 63, 0} <= seen64 and {134, 135, 0} <= seen136
    with pytest.raises(pkg.H2AggError) as ei:
        pkg.hash_digest_host(0, b"")
    assert ei.value.code == pkg.ERR_INVALID


# scripts: Q first, QQ, C and X items, zero P items, and enough different segment lengths for every reachable residue
SCRIPTS = [
    "Q",
    "QQQ",
    "QCQ",
    "CXQPQQSSQ",
    "SQSSQQCQ",
    "XXQ",
    "CSQ",
    "PPPQSQPQ",
    "CXPPQPQQPPPQSSSSSQPPPPQQ",
] + ["S" * k + "Q" + "P" * (17 - k) + "Q" for k in range(1, 18)]


def make_proofs(rng, script, nproofs):
    """random proofs for a script -> (proofs, consts as ints, ext points per proof)"""
    consts = [rng.fr() for _ in range(script.count("C"))]
    proofs, exts = [], []
    for _ in range(nproofs):
        out = bytearray()
        for ch in script:
            if ch == "P":
                out += O.aff_to_bytes(O.scalar_mul(rng.fr(), O.G1))
            elif ch == "S":
                out += O.fe_to_bytes(rng.fr())
        proofs.append(bytes(out))
        exts.append([O.scalar_mul(rng.fr(), O.G1) for _ in range(script.count("X"))])
    return proofs, consts, exts


def reference(kind, script, proofs, consts, exts):
    pts, chal, lens = [], [], []
    for p, x in zip(proofs, exts):
        a, b, l = H.run_script(kind, p, script, consts, x)
        pts.append(a)
        chal.append(b)
        lens += l
    return pts, chal, lens


@pytest.mark.parametrize("kind", KINDS)
def test_host_backend_matches_the_reference_reader(pkg, kind):
    rng = O.SplitMix64(0x5A4 + len(kind))
    hashed_lengths = []
    for si, script in enumerate(SCRIPTS):
        nproofs = 1 + si % 3
        proofs, consts, exts = make_proofs(rng, script, nproofs)
        want_pts, want_chal, lens = reference(kind, script, proofs, consts, exts)
        hashed_lengths += lens
        got_pts, got_chal = pkg.hash_transcript_read_batch_host(
            kind, proofs, script, b"".join(O.fe_to_bytes(c) for c in consts),
            b"".join(O.aff_to_bytes(p) for x in exts for p in x), max_threads=1 + si % 2)
        assert got_pts == want_pts, script
        assert got_chal == want_chal, script
    # every residue class a transcript can reach, on both sides of the block boundary
    assert all(n % 32 == 1 for n in hashed_lengths)
    assert {n % 64 for n in hashed_lengths} == {1, 33}
    assert {n % 136 for n in hashed_lengths} == {1 + 8 * j for j in range(17)}
    assert any(n > 136 for n in hashed_lengths) and any(n > 2 * 136 for n in hashed_lengths) and 1 in hashed_lengths


def off_curve_point():
    x = 1
    while (pow(x, 3, O.P) + 3) % O.P == 4:       # (x, 2) on the curve only if x^3 + 3 == 4
        x += 1
    return x.to_bytes(32, "little") + (2).to_bytes(32, "little")


@pytest.mark.parametrize("kind", KINDS)
def test_error_mapping(pkg, kind):
    rng = O.SplitMix64(0xE44)
    script = "CPSQPQ"
    proofs, consts, exts = make_proofs(rng, script, 3)
    cb = b"".join(O.fe_to_bytes(c) for c in consts)

    def call(ps, sc=script, c=cb, k=kind):
        return pkg.hash_transcript_read_batch_host(k, ps, sc, c)
    call(proofs)
    g = O.aff_to_bytes(O.G1)

    def with_bytes(off, b):
        bad = bytearray(proofs[1])
        bad[off:off + len(b)] = b
        return [proofs[0], bytes(bad), proofs[2]]
    second_point = 64 + 32
    for what, ps in [("x = p", with_bytes(0, O.P.to_bytes(32, "little"))),
                     ("y = p", with_bytes(second_point + 32, O.P.to_bytes(32, "little"))),
                     ("off the curve", with_bytes(second_point, off_curve_point())),
                     ("(0, 0)", with_bytes(0, bytes(64)))]:
        with pytest.raises(pkg.H2AggError) as ei:
            call(ps)
        assert ei.value.code == pkg.ERR_BAD_POINT, what
    with pytest.raises(pkg.H2AggError) as ei:
        call(with_bytes(64, O.R.to_bytes(32, "little")))
    assert ei.value.code == pkg.ERR_NONCANONICAL
    with pytest.raises(pkg.H2AggError) as ei:
        call(proofs, c=O.R.to_bytes(32, "little"))
    assert ei.value.code == pkg.ERR_NONCANONICAL
    # an identity external point: "cannot write points at infinity to the transcript"
    with pytest.raises(pkg.H2AggError) as ei:
        pkg.hash_transcript_read_batch_host(kind, [g], "XPQ", b"", bytes(64))
    assert ei.value.code == pkg.ERR_BAD_POINT
    # wrong proof_len (a compressed-size proof), unknown kind, unknown script operation
    lib = pkg.load_library()
    import ctypes as C
    pts, ch = C.create_string_buffer(256), C.create_string_buffer(256)
    assert lib.h2agg_hash_transcript_read_batch_host(pkg.TRANSCRIPT_KINDS[kind], g[:32], 32, 1, b"PQ", 2, None, 0, None, 0, pts, ch, 1) == pkg.ERR_INVALID
    assert lib.h2agg_hash_transcript_read_batch_host(pkg.TRANSCRIPT_KINDS[kind], g, 64, 1, b"PQ", 2, None, 0, None, 0, pts, ch, 1) == pkg.OK
    for k in (0, 3, -1):
        assert lib.h2agg_hash_transcript_read_batch_host(k, g, 64, 1, b"PQ", 2, None, 0, None, 0, pts, ch, 1) == pkg.ERR_INVALID
    assert lib.h2agg_hash_transcript_read_batch_host(pkg.TRANSCRIPT_KINDS[kind], g, 64, 1, b"PZ", 2, None, 0, None, 0, pts, ch, 1) == pkg.ERR_INVALID


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape_id", [0, 1])
def test_oracle_accepts_trapdoor_proofs_and_rejects_one_bit_changes(kind, shape_id):
    """validates the test infrastructure: hash_transcript_ref + toy_prover_hash under the reference's pairing check"""
    setup, circuits = TH.make_batch(0x4A0 + shape_id, [SHAPES[shape_id]], 1, kind)
    c = circuits[0]
    inst, data = c.proofs[0]

    def accepted():
        try:
            left, right = TH.oracle_pair(c, 0, kind)
        except (AssertionError, ValueError, V.P.TranscriptError):
            return False
        return E.pairing_check([(left, setup.s_g2), (right, E.g2_neg(setup.g2))])
    assert accepted()
    last_eval = len(data) - 64 * 4 - 32          # four W points close the transcript; the last evaluation before them
    for off in (5, last_eval + 3, len(data) - 64 * 2 + 40):   # a point's x, a scalar, a W point's y
        bad = bytearray(data)
        bad[off] ^= 1
        c.proofs[0] = (inst, bytes(bad))
        assert not accepted(), off
    inst2 = [[list(col) for col in row] for row in inst]
    inst2[0][0][0] ^= 1
    c.proofs[0] = (inst2, data)
    assert not accepted()
    c.proofs[0] = (inst, data)
    assert accepted()
    # the same key's proof written with the OTHER digest is not accepted either
    other = "keccak256" if kind == "sha256" else "sha256"
    try:
        left, right = TH.oracle_pair(c, 0, other)
        ok = E.pairing_check([(left, setup.s_g2), (right, E.g2_neg(setup.g2))])
    except (AssertionError, ValueError, V.P.TranscriptError):
        ok = False
    assert not ok
