"""GPU: the quotient polynomial h(X) — h2agg_vk_expressions_eval, h2agg_quotient, their _device twins, and poly.py over them.

halo2_proofs is not vendored in the reference, so the yardstick is the definition in include/h2agg.h, restated with Python
integers in tests/quotient_ref.py, which tests/test_quotient_host.py ties to the identity the reference's verifier checks
(oracle/verifier.py:348-356, :393-398).  Everything is exact and compared byte for byte."""
import importlib
import random

import pytest

import __graft_entry__ as entry
from oracle import bn254 as O
from tests import quotient_ref as Q
from tests.fr_bytes import dec, enc, fe
from tests.toy_prover import make_constraint_system

pytestmark = pytest.mark.gpu

R = Q.R
BF = 5


@pytest.fixture(scope="module")
def poly(pkg):
    return importlib.import_module(entry.PKG_NAME + ".poly")


@pytest.fixture(scope="module")
def verifier(pkg):
    return importlib.import_module(entry.PKG_NAME + ".verifier")


@pytest.fixture(scope="module")
def satisfied():
    """satisfied_circuit at k = 5 (degree 4: four sets, the last ragged) and k = 8 (degree 6: two sets), with quotient_py's pieces"""
    out = {}
    for k, degree in ((5, 4), (8, 6)):
        cs, lag, polys, sc = Q.satisfied_circuit(random.Random(0xD00 + k), k, degree)
        pieces, H = Q.quotient_py(cs, *Q.quotient_args(polys, sc))
        assert not any(H[(degree - 1) << k:])
        out[k] = (cs, lag, polys, sc, pieces)
    return out


def make_vk(eng, verifier, cs):
    return verifier.VerifyingKey(eng, verifier.encode_vk(cs, O.aff_to_bytes))


def cols(columns):
    return [enc(c) for c in columns]


def scalars(sc):
    return [fe(c) for c in sc["challenges"]], fe(sc["theta"]), fe(sc["beta"]), fe(sc["gamma"]), fe(sc["y"]), fe(sc["delta"])


def device_slab(columns):
    """columns of integers -> (tensor or None, pointer or None)"""
    import torch
    if not columns:
        return None, None
    t = torch.frombuffer(bytearray(b"".join(enc(c) for c in columns)), dtype=torch.uint8).to(torch.device("cuda:0"))
    return t, t.data_ptr()


def quotient_host(eng, poly, vk, polys, sc):
    ch, theta, beta, gamma, y, delta = scalars(sc)
    return poly.quotient_pieces(eng, vk, *[cols(polys[kind]) for kind in Q.POLY_KINDS], ch, theta, beta, gamma, y, delta)


def quotient_device(eng, vk, ptrs, sc, d_out_ptr):
    ch, theta, beta, gamma, y, delta = scalars(sc)
    eng.quotient_device(vk, *ptrs, b"".join(ch) if ch else None, theta, beta, gamma, y, delta, d_out_ptr)


def random_columns(rng, cs):
    n = cs.n
    col = lambda: [rng.choice((0, R - 1)) if rng.randrange(16) == 0 else rng.randrange(R) for _ in range(n)]
    return ([col() for _ in range(cs.num_advice_columns)], [col() for _ in range(len(cs.fixed_commitments))],
            [col() for _ in range(cs.num_instance_columns)])


def check_expressions(eng, poly, vk, cs, advice, fixed, instance, challenges, theta):
    """all three lists, fold None and fold = theta, host form and _device twin, against expressions_rows_py"""
    import torch
    n = cs.n
    ch = [fe(c) for c in challenges]
    keep = [device_slab(x) for x in (advice, fixed, instance)]
    lists = [(0, 0)] + [(w, j) for j in range(len(cs.lookups)) for w in (1, 2)]
    for which, j in lists:
        want = Q.expressions_rows_py(cs, which, j, advice, fixed, instance, challenges)
        if not want:
            continue
        folded = Q.expressions_rows_py(cs, which, j, advice, fixed, instance, challenges, theta)
        got = poly.expressions_eval(eng, vk, which, j, cols(advice), cols(fixed), cols(instance), ch)
        assert got == cols(want), (which, j, "columns")
        assert poly.expressions_eval(eng, vk, which, j, cols(advice), cols(fixed), cols(instance), ch, fe(theta)) == enc(folded), \
            (which, j, "fold")
        d_out = torch.zeros(32 * n * (len(want) + 1), dtype=torch.uint8, device=torch.device("cuda:0"))
        torch.cuda.synchronize()
        chb = b"".join(ch) if ch else None
        eng.vk_expressions_eval_device(vk, which, j, cs.k, keep[0][1], keep[1][1], keep[2][1], chb, None, d_out.data_ptr())
        eng.vk_expressions_eval_device(vk, which, j, cs.k, keep[0][1], keep[1][1], keep[2][1], chb, fe(theta),
                                       d_out.data_ptr() + 32 * n * len(want))
        eng.synchronize()
        assert bytes(d_out.cpu().numpy()) == b"".join(cols(want)) + enc(folded), (which, j, "device")


# ---------------------------------------------------------------------------------------------- expressions
@pytest.mark.parametrize("n_challenges", [0, 2])
@pytest.mark.parametrize("k", [4, 6, 9])
def test_expressions_of_toy_keys(eng, poly, verifier, k, n_challenges):
    """k = 4: one partial workgroup; 6: exactly one; 9: several"""
    cs = make_constraint_system(O.SplitMix64(0xD10 + 16 * k + n_challenges), k=k, n_lookups=2, n_challenges=n_challenges)
    rng = random.Random(0xD11 + k)
    vk = make_vk(eng, verifier, cs)
    advice, fixed, instance = random_columns(rng, cs)
    check_expressions(eng, poly, vk, cs, advice, fixed, instance, [rng.randrange(R) for _ in range(n_challenges)], rng.randrange(R))
    vk.close()


def nested_sum(depth):
    """an expression whose postfix form holds `depth` values at once: a_0 + (a_1 + (... + a_{depth-1}))"""
    e = ("advice", (depth - 1) % 5)
    for i in range(depth - 2, -1, -1):
        e = ("sum", ("product", ("advice", i % 5), ("const", i + 2)) if i % 3 == 0 else ("advice", i % 5), e)
    return e


def handmade_cs(k, gates, lookups=()):
    n = 1 << k
    advice_queries = [(0, 1), (1, -1), (0, -(BF + 1)), (1, n - 1), (0, -n - 3)]
    return Q.make_cs(k, 4, 2, 1, 1, advice_queries, [(0, 0)], [(0, 2)], gates, list(lookups), [], BF, 1)


@pytest.mark.parametrize("k", [4, 6])
def test_expressions_handmade_rotations_constants_and_depth(eng, pkg, poly, verifier, k):
    rng = random.Random(0xD20 + k)
    A = [("advice", q) for q in range(5)]
    F, I, CH = ("fixed", 0), ("instance", 0), ("challenge", 0)
    deep = nested_sum(pkg.EXPR_MAX_DEPTH)
    gates = [[("sum", A[0], ("sum", A[1], ("sum", A[2], ("sum", A[3], A[4])))), ("product", ("const", 0), A[0])],
             [("sum", ("product", ("const", 1), A[1]), ("scaled", ("neg", ("product", A[2], ("const", R - 1))), R - 1)), A[4]],
             [deep, ("product", ("sum", F, ("neg", I)), ("sum", CH, ("const", R - 1)))]]
    lookups = [([A[3], ("neg", A[4])], [F])]
    cs = handmade_cs(k, gates, lookups)
    vk = make_vk(eng, verifier, cs)
    advice, fixed, instance = random_columns(rng, cs)
    challenges, theta = [rng.randrange(R)], rng.randrange(R)
    check_expressions(eng, poly, vk, cs, advice, fixed, instance, challenges, theta)
    # by hand: CONST 0 times anything; query 4 is column 0 at rotation -n - 3, row i - 3
    got = poly.expressions_eval(eng, vk, 0, 0, cols(advice), cols(fixed), cols(instance), [fe(challenges[0])])
    assert len(got) == 6 and dec(got[1]) == [0] * cs.n
    assert dec(got[3]) == [advice[0][(i - 3) % cs.n] for i in range(cs.n)]
    # one value more on the stack: refused by this call, not by the key, and the context goes on
    too_deep = handmade_cs(k, [[nested_sum(pkg.EXPR_MAX_DEPTH + 1)], [A[0]]], lookups)
    vk2 = make_vk(eng, verifier, too_deep)
    for fold in (None, fe(theta)):
        with pytest.raises(pkg.H2AggError) as ei:
            poly.expressions_eval(eng, vk2, 0, 0, cols(advice), cols(fixed), cols(instance), [fe(challenges[0])], fold)
        assert ei.value.code == pkg.ERR_INVALID, ei.value
    want = Q.expressions_rows_py(too_deep, 1, 0, advice, fixed, instance, challenges)
    assert poly.expressions_eval(eng, vk2, 1, 0, cols(advice), cols(fixed), cols(instance), [fe(challenges[0])]) == cols(want)
    # an empty gate list, an unknown list, a lookup that is not there, another k, a missing slab, scalars and elements >= r
    empty = make_vk(eng, verifier, handmade_cs(k, [], lookups))
    ch = fe(challenges[0])
    a_b, f_b, i_b = b"".join(cols(advice)), b"".join(cols(fixed)), b"".join(cols(instance))
    call = eng.vk_expressions_eval
    bad_a = enc([R]) + a_b[32:]
    for code, args in ((pkg.ERR_INVALID, (empty, 0, 0, k, a_b, f_b, i_b, ch, None)),
                       (pkg.ERR_INVALID, (empty, 0, 0, k, a_b, f_b, i_b, ch, fe(theta))),
                       (pkg.ERR_INVALID, (vk, 3, 0, k, a_b, f_b, i_b, ch, None)),
                       (pkg.ERR_INVALID, (vk, -1, 0, k, a_b, f_b, i_b, ch, None)),
                       (pkg.ERR_INVALID, (vk, 1, 1, k, a_b, f_b, i_b, ch, None)),
                       (pkg.ERR_INVALID, (vk, 0, 0, k + 1, a_b, f_b, i_b, ch, None)),
                       (pkg.ERR_INVALID, (vk, 0, 0, k, None, f_b, i_b, ch, None)),
                       (pkg.ERR_INVALID, (vk, 0, 0, k, a_b, None, i_b, ch, None)),
                       (pkg.ERR_INVALID, (vk, 0, 0, k, a_b, f_b, None, ch, None)),
                       (pkg.ERR_INVALID, (vk, 0, 0, k, a_b, f_b, i_b, None, None)),
                       (pkg.ERR_NONCANONICAL, (vk, 0, 0, k, a_b, f_b, i_b, enc([R]), None)),
                       (pkg.ERR_NONCANONICAL, (vk, 0, 0, k, a_b, f_b, i_b, ch, enc([R]))),
                       (pkg.ERR_NONCANONICAL, (vk, 0, 0, k, bad_a, f_b, i_b, ch, fe(theta)))):
        with pytest.raises(pkg.H2AggError) as ei:
            call(*args)
        assert ei.value.code == code, (args[1:4], ei.value)
        assert poly.expressions_eval(eng, vk, 1, 0, cols(advice), cols(fixed), cols(instance), [ch], fe(theta)) == \
            enc(Q.expressions_rows_py(cs, 1, 0, advice, fixed, instance, challenges, theta))
    with pytest.raises(pkg.H2AggError) as ei:
        eng.vk_expressions_eval_device(vk, 0, 0, k, None, None, None, ch, None, None)
    assert ei.value.code == pkg.ERR_INVALID
    for key in (vk, vk2, empty):
        key.close()


def test_gates_vanish_on_a_satisfied_witness(eng, poly, verifier, satisfied):
    cs, lag, _polys, sc, _pieces = satisfied[5]
    vk = make_vk(eng, verifier, cs)
    got = poly.expressions_eval(eng, vk, 0, 0, cols(lag["advice"]), cols(lag["fixed"]), cols(lag["instance"]), [], fe(sc["y"]))
    assert got == bytes(32 * cs.n)
    vk.close()


# ---------------------------------------------------------------------------------------------- the quotient
# k: 4 (u = 10 with five blinding rows), 6, 9; degree 3 / 4 / 6: e = 1 / 2 / 3, chunk_len c = 1 / 2 / 4; permutation columns 0, 1, c,
# c + 1, 2c + 1: no argument, one set, full sets, a ragged last set; lookups 0, 1, 2; gates none and several
SHAPES = [  # k, degree, permutation columns, lookups, gates, challenges
    (4, 3, 0, 0, False, 0), (4, 3, 0, 0, True, 2), (4, 3, 3, 1, False, 0), (4, 4, 1, 2, True, 0), (4, 6, 5, 1, True, 2),
    (6, 3, 2, 0, True, 0), (6, 4, 2, 0, True, 0), (6, 4, 5, 2, False, 2), (6, 6, 4, 1, True, 0), (6, 6, 0, 1, False, 0),
    (9, 3, 1, 1, True, 0), (9, 4, 3, 0, True, 2), (9, 6, 9, 2, True, 0)]


@pytest.mark.parametrize("k,degree,n_perm,n_lookups,with_gates,n_challenges", SHAPES)
def test_quotient_of_random_polynomials(eng, poly, verifier, k, degree, n_perm, n_lookups, with_gates, n_challenges):
    rng = random.Random(hash((0xD30, k, degree, n_perm, n_lookups, with_gates)) & 0xFFFFFFFF)
    cs = Q.random_shape(rng, k, degree, n_perm, n_lookups, with_gates, BF, n_challenges)
    assert Q.extended_k(k, degree) == {3: 1, 4: 2, 6: 3}[degree]
    polys, sc = Q.random_inputs(rng, cs), Q.random_scalars(rng, n_challenges)
    want, _H = Q.quotient_py(cs, *Q.quotient_args(polys, sc))
    vk = make_vk(eng, verifier, cs)
    assert quotient_host(eng, poly, vk, polys, sc) == cols(want)
    vk.close()


@pytest.mark.parametrize("k", [5, 8])
def test_quotient_of_a_satisfied_circuit(eng, poly, verifier, satisfied, k):
    cs, _lag, polys, sc, want = satisfied[k]
    vk = make_vk(eng, verifier, cs)
    got = quotient_host(eng, poly, vk, polys, sc)
    assert got == cols(want)
    pieces = [dec(p) for p in got]
    rng = random.Random(0xD40 + k)
    for _ in range(2):                                   # the verifier's identity (oracle/verifier.py:393-398)
        x = rng.randrange(R)
        assert Q.verifier_numerator(cs, polys, sc, x) == Q.h_at(pieces, cs.n, x)
    # commit_quotient: commit_coeff of each piece (a Jacobian point has many encodings: compared as affine points), which
    # with the trapdoor known is h_i(s) * G
    s = 0x5EC12E7 + k
    g, gl = eng.params_setup(k, fe(s))
    commits = poly.commit_quotient(eng, g, got)
    assert len(commits) == cs.degree - 1
    assert eng.g1_batch_to_affine(b"".join(commits)) == eng.g1_batch_to_affine(b"".join(poly.commit_coeff(eng, g, p) for p in got))
    assert eng.g1_batch_to_affine(b"".join(commits)) == b"".join(O.aff_to_bytes(O.scalar_mul(Q.horner(p, s), O.G1)) for p in pieces)
    eng.bases_free(g)
    eng.bases_free(gl)
    vk.close()


def test_quotient_queued_back_to_back(eng, verifier, satisfied):
    """two h2agg_quotient_device calls with different scalars, then the chain h2agg_fr_fft_device (Lagrange -> coefficients) ->
    h2agg_quotient_device, one synchronisation behind all of it"""
    import torch
    cs, lag, polys, sc, want = satisfied[5]
    k, n = cs.k, cs.n
    vk = make_vk(eng, verifier, cs)
    other = dict(sc, theta=(sc["theta"] + 1) % R, beta=(sc["beta"] + 2) % R, gamma=(sc["gamma"] + 4) % R, y=(sc["y"] + 8) % R)
    want_other, _H = Q.quotient_py(cs, *Q.quotient_args(polys, other))
    assert want_other != want
    coeff = [device_slab(polys[kind]) for kind in Q.POLY_KINDS]
    rows = [device_slab(lag[kind]) for kind in Q.POLY_KINDS]
    piece_bytes = 32 * n * (cs.degree - 1)
    d_out = torch.zeros(3 * piece_bytes, dtype=torch.uint8, device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    quotient_device(eng, vk, [p for _t, p in coeff], sc, d_out.data_ptr())
    quotient_device(eng, vk, [p for _t, p in coeff], other, d_out.data_ptr() + piece_bytes)
    for kind, (_t, ptr) in zip(Q.POLY_KINDS, rows):
        for c in range(len(lag[kind])):
            eng.fr_fft_device(ptr + 32 * n * c, k, True, None, ptr + 32 * n * c)
    quotient_device(eng, vk, [p for _t, p in rows], sc, d_out.data_ptr() + 2 * piece_bytes)
    eng.synchronize()
    got = bytes(d_out.cpu().numpy())
    assert got[:piece_bytes] == b"".join(cols(want)), "first call"
    assert got[piece_bytes:2 * piece_bytes] == b"".join(cols(want_other)), "second call"
    assert got[2 * piece_bytes:] == b"".join(cols(want)), "behind the transforms"
    for (t, _p), kind in zip(coeff, Q.POLY_KINDS):
        assert bytes(t.cpu().numpy()) == b"".join(cols(polys[kind])), "an input changed"
    vk.close()


def test_quotient_refusals_leave_the_context_usable(eng, pkg, poly, verifier, satisfied):
    cs, _lag, polys, sc, want = satisfied[5]
    vk = make_vk(eng, verifier, cs)
    k = cs.k
    slabs = [b"".join(cols(polys[kind])) for kind in Q.POLY_KINDS]
    ch, theta, beta, gamma, y, delta = scalars(sc)
    pieces = cs.degree - 1

    def still_works():
        assert quotient_host(eng, poly, vk, polys, sc) == cols(want)

    def refused(code, fn):
        with pytest.raises(pkg.H2AggError) as ei:
            fn()
        assert ei.value.code == code, ei.value
        still_works()

    # k + e > 24: a key with k = 23 and degree 6 (e = 3); refused before anything is read or allocated
    big = make_vk(eng, verifier, Q.make_cs(23, 6, 1, 0, 0, [(0, 0)], [], [], [[("advice", 0)]], [], [], BF))
    one = enc([1])
    refused(pkg.ERR_INVALID, lambda: eng._check(eng._lib.h2agg_quotient(eng._ctx, big._vk, one, None, None, None, None, None, None, None,
                                                                        None, theta, beta, gamma, y, delta, one)))
    refused(pkg.ERR_INVALID, lambda: eng._check(eng._lib.h2agg_quotient_device(eng._ctx, big._vk, None, None, None, None, None, None,
                                                                               None, None, None, theta, beta, gamma, y, delta, None)))
    big.close()
    for hole in range(8):                                # every slab of this key is required
        args = list(slabs)
        args[hole] = None
        refused(pkg.ERR_INVALID, lambda: eng.quotient(vk, *args, None, theta, beta, gamma, y, delta))
    for hole in range(5):                                # a scalar >= r
        sc5 = [theta, beta, gamma, y, delta]
        sc5[hole] = enc([R])
        refused(pkg.ERR_NONCANONICAL, lambda: eng.quotient(vk, *slabs, None, *sc5))
    for hole in (0, 3, 4, 6):                            # an element >= r: advice, sigma, a permutation Z, a lookup's a'
        args = list(slabs)
        args[hole] = args[hole][:64] + enc([R + 1]) + args[hole][96:]
        refused(pkg.ERR_NONCANONICAL, lambda: eng.quotient(vk, *args, None, theta, beta, gamma, y, delta))
    # the _device twin reports it at synchronize, once
    import torch
    bad = {kind: [list(c) for c in polys[kind]] for kind in Q.POLY_KINDS}
    bad["lookup_sp"][0][7] = (1 << 256) - 1
    dev = [device_slab(bad[kind]) for kind in Q.POLY_KINDS]
    d_out = torch.zeros(32 * cs.n * pieces, dtype=torch.uint8, device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    quotient_device(eng, vk, [p for _t, p in dev], sc, d_out.data_ptr())
    with pytest.raises(pkg.H2AggError) as ei:
        eng.synchronize()
    assert ei.value.code == pkg.ERR_NONCANONICAL
    eng.synchronize()
    still_works()
    vk.close()
