"""CPU, no context: the G2 half of a params file (h2agg_g2_scalar_mul, h2agg_g2_batch_compress) against the oracle's twist
arithmetic, and the params layout over host-made pieces."""
import ctypes as C
import importlib

import pytest

import __graft_entry__ as entry
from oracle import bn254 as O
from oracle import pairing as E


def g2b(q):
    if q is O.INF:
        return bytes(128)
    return b"".join(O.fe_to_bytes(v) for v in (q[0][0], q[0][1], q[1][0], q[1][1]))


def g2_compress(q):
    """halo2curves 0.2.1 G2Affine::to_bytes (recalled): x.c0 || x.c1, parity of y.c0 in bit 7 of the last byte"""
    if q is O.INF:
        return bytes(64)
    b = bytearray(O.fe_to_bytes(q[0][0]) + O.fe_to_bytes(q[0][1]))
    b[63] |= (q[1][0] & 1) << 7
    return bytes(b)


def scalars():
    rng = O.SplitMix64(0x6732)
    return [1, 2, O.R - 1] + [rng.fr() for _ in range(3)]


@pytest.fixture(scope="module")
def points():
    """s * G2 by the oracle, once, for every scalar of the tests"""
    return [(s, E.g2_mul(s, E.G2)) for s in scalars()]


def test_g2_scalar_mul_matches_the_oracle(pkg, points):
    for s, want in points:
        assert pkg.g2_scalar_mul(g2b(E.G2), O.fe_to_bytes(s)) == g2b(want), s
    # a base other than the generator, the identity on either side, s = 0
    s0, q0 = points[3]
    s1 = points[4][0]
    assert pkg.g2_scalar_mul(g2b(q0), O.fe_to_bytes(s1)) == g2b(E.g2_mul(s0 * s1 % O.R, E.G2))
    assert pkg.g2_scalar_mul(g2b(E.G2), bytes(32)) == bytes(128)
    assert pkg.g2_scalar_mul(bytes(128), O.fe_to_bytes(5)) == bytes(128)


def test_g2_scalar_mul_refuses_bad_inputs(pkg):
    with pytest.raises(pkg.H2AggError) as ei:
        pkg.g2_scalar_mul(g2b(E.G2), O.R.to_bytes(32, "little"))
    assert ei.value.code == pkg.ERR_NONCANONICAL
    off = bytearray(g2b(E.G2))
    off[0] ^= 1
    with pytest.raises(pkg.BadPoint):
        pkg.g2_scalar_mul(bytes(off), O.fe_to_bytes(3))
    big = O.P.to_bytes(32, "little") + g2b(E.G2)[32:]
    with pytest.raises(pkg.H2AggError) as ei:
        pkg.g2_scalar_mul(big, O.fe_to_bytes(3))
    assert ei.value.code == pkg.ERR_NONCANONICAL


def test_g2_compress_is_the_inverse_of_decompress(pkg, points):
    lib = pkg.load_library()
    pts = [q for _s, q in points] + [O.INF]
    aff = b"".join(g2b(q) for q in pts)
    comp = pkg.g2_batch_compress(aff)
    assert comp == b"".join(g2_compress(q) for q in pts)
    assert {c[63] >> 7 for c in (comp[i:i + 64] for i in range(0, len(comp) - 64, 64))} == {0, 1}   # both parities occur
    out = C.create_string_buffer(128 * len(pts))
    assert lib.h2agg_g2_batch_decompress(None, comp, len(pts), out) == 0
    assert out.raw == aff
    assert pkg.g2_batch_compress(b"") == b""
    off = bytearray(g2b(E.G2))
    off[64] ^= 1
    with pytest.raises(pkg.BadPoint):
        pkg.g2_batch_compress(bytes(off))


def test_compressed_generator_is_the_one_params_files_hold(pkg):
    """tests/golden holds no params file; the generator's encoding is pinned against halo2curves' published G2 generator
    (oracle/pairing.py G2) instead: x.c0 || x.c1 with the parity of y.c0"""
    comp = pkg.g2_batch_compress(g2b(E.G2))
    assert comp == g2_compress(E.G2)
    assert int.from_bytes(comp[:32], "little") == E.G2[0][0]


def test_params_layout_round_trip_over_host_made_pieces(pkg):
    entry.load_package()
    fs = importlib.import_module(entry.PKG_NAME + ".fs")
    rng = O.SplitMix64(0x9A7A)
    k, tau = 2, rng.fr()
    g = b"".join(O.compress(O.scalar_mul(pow(tau, i, O.R), O.G1)) for i in range(4))
    gl = b"".join(O.compress(O.scalar_mul(rng.fr(), O.G1)) for _ in range(4))
    s_g2 = pkg.g2_scalar_mul(g2b(E.G2), O.fe_to_bytes(tau))
    p = fs.KzgParams(k, g, gl, pkg.g2_batch_compress(g2b(E.G2)), pkg.g2_batch_compress(s_g2))
    b = fs.write_params(p)
    assert len(b) == 4 + 64 * 4 + 128
    assert fs.write_params(fs.read_params(b)) == b
    q = fs.read_params(b)
    out = C.create_string_buffer(256)
    assert pkg.load_library().h2agg_g2_batch_decompress(None, q.s_g2 + q.g2, 2, out) == 0
    assert out.raw == s_g2 + g2b(E.G2) == g2b(E.g2_mul(tau, E.G2)) + g2b(E.G2)
