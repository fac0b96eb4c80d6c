"""GPU: the coset-split ending of h2agg_quotient — per-coset inverse transforms of size 2^k and
k_qe_cross_cosets instead of one inverse transform of size 2^(k+e).

Below 2^24 both routes are legal, and h2agg_quotient_configure(ctx, 1) forces the new one: its pieces must be the default
route's and tests/quotient_ref.py's byte for byte, from both entry points.  Above 2^24 only the new route exists (and only
the resident entry point takes such keys: the host-buffer form keeps k + e <= 24) and no Python restatement is affordable: there the pieces are held against the identity the verifier checks, N(x) = (x^n - 1) sum_i x^(n i)
h_i(x), with the numerator built by the oracle's own expression functions from evaluations the device took.

A context of its own carries the setting (the session's engine is never left with a non-default one); a verifying key belongs
to the context that made it, so every shape has one key per context.  h2agg_vk_create refuses degree < 3, so no key reaches
e = 0 on either route; tests/test_quotient_split_host.py holds the decomposition at e = 0."""
import importlib
import random

import pytest

import __graft_entry__ as entry
from tests import honest_prover as HP
from tests import quotient_ref as Q
from tests.fr_bytes import enc
from tests.test_gpu_honest_proofs import BIG, TAU, verdicts
from tests.test_gpu_quotient import BF, cols, device_slab, make_vk, quotient_device, quotient_host, scalars

pytestmark = pytest.mark.gpu

R = Q.R


@pytest.fixture(scope="module")
def poly(pkg):
    return importlib.import_module(entry.PKG_NAME + ".poly")


@pytest.fixture(scope="module")
def verifier(pkg):
    return importlib.import_module(entry.PKG_NAME + ".verifier")


@pytest.fixture(scope="module")
def split(pkg):
    """a context on which every quotient takes the split route"""
    e = pkg.H2Agg(0)
    e.quotient_configure(1)
    yield e
    e.close()


def device_pieces(eng, vk, polys, sc, pieces, n, others=()):
    """h2agg_quotient_device over fresh device slabs, then (for `others`) further calls queued behind it with those scalars;
    one synchronisation behind all of them -> the outputs, one bytes object per call"""
    import torch
    slabs = [device_slab(polys[kind]) for kind in Q.POLY_KINDS]
    size = 32 * n * pieces
    d_out = torch.zeros(size * (1 + len(others)), dtype=torch.uint8, device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    for i, s in enumerate((sc,) + tuple(others)):
        quotient_device(eng, vk, [p for _t, p in slabs], s, d_out.data_ptr() + i * size)
    eng.synchronize()
    got = bytes(d_out.cpu().numpy())
    return [got[i * size:(i + 1) * size] for i in range(1 + len(others))]


# ---------------------------------------------------------------------------------------------- byte equality of the routes
# k = 5: every transform one workgroup; 7: several workgroups of the row kernels.  degree 3 / 4, 5 / 6, 9: e = 1 / 2 / 3.
# degree - 1 = 2, 4, 8 are powers of two (every output of the cross-coset transform is a piece); 3 and 5 are not (fewer pieces
# than cosets; 5 = one full group of four pieces and a group of one).  Permutation columns 0 (no argument), one set, ragged
# sets; lookups 0, 1, 2; with and without gates and challenges.
SHAPES = [  # k, degree, permutation columns, lookups, gates, challenges
    (5, 3, 3, 1, False, 0), (5, 4, 1, 2, True, 0), (5, 6, 5, 1, True, 2), (5, 9, 0, 1, True, 0),
    (7, 3, 2, 0, True, 0), (7, 5, 0, 1, True, 2), (7, 4, 5, 2, False, 0), (7, 9, 9, 1, True, 0)]


@pytest.mark.parametrize("k,degree,n_perm,n_lookups,with_gates,n_challenges", SHAPES)
def test_both_routes_give_the_reference_pieces(eng, split, poly, verifier, k, degree, n_perm, n_lookups, with_gates, n_challenges):
    rng = random.Random(hash((0xE60, k, degree, n_perm, n_lookups, with_gates)) & 0xFFFFFFFF)
    cs = Q.random_shape(rng, k, degree, n_perm, n_lookups, with_gates, BF, n_challenges)
    assert Q.extended_k(k, degree) == {3: 1, 4: 2, 5: 2, 6: 3, 9: 3}[degree]
    polys, sc = Q.random_inputs(rng, cs), Q.random_scalars(rng, n_challenges)
    want, _H = Q.quotient_py(cs, *Q.quotient_args(polys, sc))
    want = cols(want)
    for name, e in (("default", eng), ("split", split)):
        vk = make_vk(e, verifier, cs)
        assert quotient_host(e, poly, vk, polys, sc) == want, name + ", host buffers"
        assert device_pieces(e, vk, polys, sc, degree - 1, cs.n) == [b"".join(want)], name + ", device buffers"
        vk.close()


def test_two_queued_calls_keep_their_own_constants(split, verifier):
    """two _device calls with different scalars back to back on one context, read behind both: the programs and the cross-coset
    constants of the second travel in stream order and cannot reach the first one's kernels"""
    rng = random.Random(0xE61)
    cs, _lag, polys, sc = Q.satisfied_circuit(rng, 5, 4)
    other = dict(sc, theta=(sc["theta"] + 1) % R, beta=(sc["beta"] + 2) % R, gamma=(sc["gamma"] + 4) % R, y=(sc["y"] + 8) % R)
    want, _H = Q.quotient_py(cs, *Q.quotient_args(polys, sc))
    want_other, _H = Q.quotient_py(cs, *Q.quotient_args(polys, other))
    assert want != want_other
    vk = make_vk(split, verifier, cs)
    got = device_pieces(split, vk, polys, sc, cs.degree - 1, cs.n, others=(other, sc))
    assert got == [b"".join(cols(want)), b"".join(cols(want_other)), b"".join(cols(want))]
    vk.close()


def test_the_honest_circuit_at_k_12(pkg, eng, split, poly, verifier):
    """the honest prover's circuit at k = 12 (tests/test_gpu_honest_proofs.py BIG: every row kernel on several workgroups,
    two-pass transforms): the quotient's inputs as the device prover hands them over, through both routes and both entry
    points.  No Python quotient at this size: the yardstick is the default route, which the proof's acceptance holds."""
    k, degree = BIG
    setup = HP.Setup(k, TAU, HP.INSTANCE_ROWS)
    circuit = HP.make_circuit(random.Random(0xD00 + 16 * k + degree), k, degree)
    seen = {}

    class Recording(HP.DeviceStages):
        def quotient(self, polys, scalars):
            seen["polys"], seen["scalars"] = polys, scalars
            seen["pieces"] = super().quotient(polys, scalars)
            return seen["pieces"]

    stages = Recording(pkg, eng, poly, verifier, setup)
    try:
        proof = HP.prove(circuit, setup, stages, random.Random(1))
    finally:
        stages.close()
    each, agg = verdicts(eng, verifier, {k: setup}, [[proof]])
    assert [(s, ok) for _pair, s, ok in each] == [(0, True)] and agg is True
    polys, sc = seen["polys"], dict(seen["scalars"], challenges=[])
    want = cols(seen["pieces"])
    vk = make_vk(split, verifier, proof.cs)
    assert quotient_host(split, poly, vk, polys, sc) == want
    assert device_pieces(split, vk, polys, sc, degree - 1, 1 << k) == [b"".join(want)]
    vk.close()


# ---------------------------------------------------------------------------------------------- one honest proof
def test_an_honest_proof_through_the_split_route(pkg, split, poly, verifier):
    k, degree = 7, 4
    setup = HP.Setup(k, TAU, HP.INSTANCE_ROWS)
    circuit = HP.make_circuit(random.Random(0xE62), k, degree)
    want = HP.prove(circuit, setup, HP.PyStages(setup), random.Random(1))
    stages = HP.DeviceStages(pkg, split, poly, verifier, setup)
    try:
        got = HP.prove(circuit, setup, stages, random.Random(1))
    finally:
        stages.close()
    assert HP.first_difference(got, want) is None, "first differing field: %s" % HP.first_difference(got, want)
    assert got.data == want.data
    each, _agg = verdicts(split, verifier, {k: setup}, [[got]])
    assert [(s, ok) for _pair, s, ok in each] == [(0, True)], "h2agg_verify_proofs: status 0, verdict True"


# ---------------------------------------------------------------------------------------------- beyond the old cap
def test_a_quotient_beyond_two_to_the_24(pkg, eng, poly, verifier, monkeypatch):
    """k = 20 with the one gate q (a^17 - a): degree 18, e = 5, an extended domain of 2^25 — h2agg_quotient refused it before.
    q is 1 on the usable rows, a holds random bits there and random elements on the blinding rows, so the gate holds; one
    permutation set over (a, q) without copy constraints; one lookup of 0 in 0.  Sigmas, both Z and the permuted pair are the
    library's.  The pieces must satisfy the verifier's identity at two random points, with every evaluation taken on the
    device (h2agg_fr_poly_eval) and the numerator built by the oracle (tests/quotient_ref.py verifier_numerator)."""
    import numpy as np
    import torch
    k, degree, e = 20, 18, 5
    n, pieces = 1 << k, degree - 1
    u = n - BF - 1
    a17 = ("advice", 0)
    for _ in range(16):
        a17 = ("product", a17, ("advice", 0))
    gates = [[("product", ("fixed", 0), ("sum", a17, ("neg", ("advice", 0))))]]
    lookups = [([("const", 0)], [("const", 0)])]
    cs = Q.make_cs(k, degree, 1, 1, 0, [(0, 0)], [(0, 0)], [], gates, lookups, [("advice", 0), ("fixed", 0)], BF)
    assert Q.extended_k(k, degree) == e and k + e == 25 and cs.num_permutation_sets == 1
    vk = make_vk(eng, verifier, cs)

    gen = np.random.default_rng(0xE63)
    rng = random.Random(0xE63)

    def random_rows(count):
        rows = gen.integers(0, 256, (count, 32), dtype=np.uint8)
        rows[:, 31] &= 0x1F                                 # below 2^253 < r
        return rows

    a = np.zeros((n, 32), dtype=np.uint8)
    a[:u, 0] = gen.integers(0, 2, u, dtype=np.uint8)
    a[u:] = random_rows(n - u)
    q = np.zeros((n, 32), dtype=np.uint8)
    q[:u, 0] = 1
    a, q, zero = a.tobytes(), q.tobytes(), bytes(32 * n)
    sc = Q.random_scalars(rng)
    _ch, theta, beta, gamma, y, delta = scalars(sc)

    # the witness holds by construction: a failure here is a mistake of this test
    mapping = poly.permutation_mapping(2, k, u, [])
    report = poly.witness_check(eng, vk, [a], [q], [], [], theta, mapping)
    assert report.total == 0, "the witness of this test does not satisfy its own circuit"

    sigma_lag, sigma = eng.permutation_sigmas(mapping, 2, k, u, delta)
    sigma_lag = [sigma_lag[:32 * n], sigma_lag[32 * n:]]
    z = poly.permutation_products(eng, [a, q], sigma_lag, k, u, beta, gamma, delta, degree - 2, [random_rows(n - u - 1).tobytes()])
    ap, sp = poly.permute_expression_pair(eng, zero, zero, k, u, (random_rows(n - u).tobytes(), random_rows(n - u).tobytes()))
    lz = poly.lookup_product(eng, zero, zero, ap, sp, k, u, beta, gamma, random_rows(n - u - 1).tobytes())
    coeff = poly.columns_lagrange_to_coeff(eng, [a, q, z[0], lz, ap, sp], k)
    inputs = {"advice": [coeff[0]], "fixed": [coeff[1]], "instance": [], "sigma": [sigma[:32 * n], sigma[32 * n:]],
              "perm_z": [coeff[2]], "lookup_z": [coeff[3]], "lookup_ap": [coeff[4]], "lookup_sp": [coeff[5]]}

    dev = torch.device("cuda:0")
    flat = [c for kind in Q.POLY_KINDS for c in inputs[kind]]
    d_in = torch.frombuffer(bytearray(b"".join(flat)), dtype=torch.uint8).to(dev)
    d_h = torch.zeros(32 * n * pieces, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ptrs, at = [], 0
    for kind in Q.POLY_KINDS:
        ptrs.append(d_in.data_ptr() + 32 * n * at if inputs[kind] else None)
        at += len(inputs[kind])
    eng.quotient_device(vk, *ptrs, None, theta, beta, gamma, y, delta, d_h.data_ptr())   # the parent: H2AGG_ERR_INVALID
    eng.synchronize()
    assert bool(d_h[32 * n * (pieces - 1):].any()), "the top piece is zero: the high outputs of the cross-coset transform are not exercised"

    # polynomials stand for themselves as (slab, column) handles; Q.horner, which verifier_numerator and h_at call for every
    # evaluation, first records the points and then answers from the device's evaluations
    handles, at = {}, 0
    for kind in Q.POLY_KINDS:
        handles[kind] = [("in", at + j) for j in range(len(inputs[kind]))]
        at += len(inputs[kind])
    piece_handles = [("h", i) for i in range(pieces)]
    for _ in range(2):
        x = rng.randrange(R)
        asked = []
        monkeypatch.setattr(Q, "horner", lambda h, pt: asked.append((h, pt % R)) or 0)
        Q.verifier_numerator(cs, handles, sc, x)
        Q.h_at(piece_handles, n, x)
        points = sorted({pt for _h, pt in asked})
        values = {}
        for slab, tensor, count in (("in", d_in, len(flat)), ("h", d_h, pieces)):
            mine = [(h[1], pt) for h, pt in asked if h[0] == slab]
            got = eng.fr_poly_eval_device(tensor.data_ptr(), count, k, [(col, points.index(pt)) for col, pt in mine], enc(points))
            for i, (col, pt) in enumerate(mine):
                values[((slab, col), pt)] = int.from_bytes(got[32 * i:32 * i + 32], "little")
        monkeypatch.setattr(Q, "horner", lambda h, pt: values[(h, pt % R)])
        assert Q.verifier_numerator(cs, handles, sc, x) == Q.h_at(piece_handles, n, x)
        monkeypatch.undo()
    vk.close()


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_context_usable(pkg, eng, split, poly, verifier):
    rng = random.Random(0xE64)
    cs = Q.random_shape(rng, 5, 4, 1, 1, True, BF)
    polys, sc = Q.random_inputs(rng, cs), Q.random_scalars(rng)
    want, _H = Q.quotient_py(cs, *Q.quotient_args(polys, sc))
    _ch, theta, beta, gamma, y, delta = scalars(sc)
    one = enc([1])
    for e in (eng, split):
        vk = make_vk(e, verifier, cs)
        # k + e = 29: k = 23 with degree 66 (e = 6), and k = 24 with degree 34 (e = 5); k = 25: refused before anything is read
        for k, degree in ((23, 66), (24, 34), (25, 3)):
            big = make_vk(e, verifier, Q.make_cs(k, degree, 1, 0, 0, [(0, 0)], [], [], [[("advice", 0)]], [], [], BF))
            # (the host-buffer form keeps k + e <= 24 and says so; the resident form states the new bound)
            for call, args, why in (
                    (e._lib.h2agg_quotient, (one, None, None, None, None, None, None, None, None, theta, beta, gamma, y, delta, one),
                     r"2\^\(k \+ e\) must be <= 2\^28|host-buffer form takes extended domains 2\^\(k \+ e\) <= 2\^24"),
                    (e._lib.h2agg_quotient_device, (None,) * 9 + (theta, beta, gamma, y, delta, None), r"2\^\(k \+ e\) must be <= 2\^28")):
                with pytest.raises(pkg.H2AggError, match=why) as ei:
                    e._check(call(e._ctx, big._vk, *args))
                assert ei.value.code == pkg.ERR_INVALID
                assert quotient_host(e, poly, vk, polys, sc) == cols(want)
            big.close()
        # k + e = 26 (k = 23, degree 6): the host-buffer form keeps its bound; the resident form takes the key (what it refuses
        # here is the null slab)
        big = make_vk(e, verifier, Q.make_cs(23, 6, 1, 0, 0, [(0, 0)], [], [], [[("advice", 0)]], [], [], BF))
        for call, args, why in (
                (e._lib.h2agg_quotient, (one, None, None, None, None, None, None, None, None, theta, beta, gamma, y, delta, one),
                 "host-buffer form takes extended domains"),
                (e._lib.h2agg_quotient_device, (None,) * 9 + (theta, beta, gamma, y, delta, None), "null buffer")):
            with pytest.raises(pkg.H2AggError, match=why) as ei:
                e._check(call(e._ctx, big._vk, *args))
            assert ei.value.code == pkg.ERR_INVALID
            assert quotient_host(e, poly, vk, polys, sc) == cols(want)
        big.close()
        # the setting takes 0 and 1 only, and a refused value changes nothing
        before = 1 if e is split else 0
        for value in (2, -1):
            with pytest.raises(pkg.H2AggError, match="split must be 0 .by size. or 1 .always.") as ei:
                e.quotient_configure(value)
            assert ei.value.code == pkg.ERR_INVALID
            assert quotient_host(e, poly, vk, polys, sc) == cols(want)
        e.quotient_configure(before)
        vk.close()
