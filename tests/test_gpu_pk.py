"""GPU: the proving key as a device object — h2agg_pk_create / _create_resident / _info / _ptr / _quotient / _destroy, and
poly.ProvingKey over them.

The yardstick is tests/quotient_ref.py (the definitions of include/h2agg.h with Python integers): the forms of a key are
Q.ntt of its columns, the quotient through the key is Q.quotient_py, and both must also be, byte for byte, what the entry
points that existed before give (h2agg_fr_fft_batch's bytes through the same reference, h2agg_quotient_device directly).
Lagrange inputs are Q.ntt of the coefficient columns the references are made of, so a key's coefficient form is those columns
again.  Every comparison is exact."""
import functools
import importlib
import random

import pytest

import __graft_entry__ as entry
from oracle import bn254 as O
from tests import honest_prover as HP
from tests import quotient_ref as Q
from tests import stream_probe as SP
from tests.fr_bytes import dec, enc, fe
from tests.grand_product_ref import DELTA
from tests.test_gpu_quotient import cols, device_slab, make_vk, quotient_device, scalars

pytestmark = pytest.mark.gpu

R = Q.R
BF = 5
WITNESS_KINDS = ("advice", "instance", "perm_z", "lookup_z", "lookup_ap", "lookup_sp")
PHASE_NAMES = ["forward", "gates", "permutation", "lookups", "inverse"]


@pytest.fixture(scope="module")
def poly(pkg):
    return importlib.import_module(entry.PKG_NAME + ".poly")


@pytest.fixture(scope="module")
def verifier(pkg):
    return importlib.import_module(entry.PKG_NAME + ".verifier")


@pytest.fixture
def split_setting(eng):
    """h2agg_quotient_configure, back at 0 behind the test"""
    yield eng.quotient_configure
    eng.quotient_configure(0)


def lagrange(polys, kind, k):
    return [Q.ntt(c, k) for c in polys[kind]]


def key_of(eng, poly, vk, cs, polys, cosets=True):
    return poly.ProvingKey.from_lagrange(eng, vk, cols(lagrange(polys, "fixed", cs.k)), cols(lagrange(polys, "sigma", cs.k)), cosets)


def read_form(eng, ptr, columns, k):
    """`columns` columns of 2^k canonical elements at a device address -> bytes.  Column by column through
    h2agg_fr_columns_compress_device with m = 1: the fold of one column is the column."""
    import torch
    if not columns:
        assert ptr is None
        return b""
    t = torch.zeros(32 * columns << k, dtype=torch.uint8, device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    for c in range(columns):
        eng.fr_columns_compress_device(ptr + (32 << k) * c, 1, k, fe(1), t.data_ptr() + (32 << k) * c)
    eng.synchronize()
    return bytes(t.cpu().numpy())


def every_form(pkg, eng, key):
    k, out = key.info["k"], []
    for which in (pkg.PK_FIXED_LAGRANGE, pkg.PK_SIGMA_LAGRANGE, pkg.PK_FIXED_COEFF, pkg.PK_SIGMA_COEFF, pkg.PK_LAGRANGE_COEFF):
        out.append(read_form(eng, *key.ptr(which), k))
    if key.cosets:
        out += [read_form(eng, *key.ptr(pkg.PK_COSET, c), k) for c in range(1 << key.info["e"])]
    return out


def witness_ptrs(dev):
    """dev: {kind: (tensor, pointer)} -> the six witness pointers of h2agg_pk_quotient"""
    return [dev[kind][1] for kind in WITNESS_KINDS]


def pk_quotient(eng, key, ptrs, sc, d_out_ptr):
    ch, theta, beta, gamma, y, delta = scalars(sc)
    eng.pk_quotient(key.handle, *ptrs, b"".join(ch) if ch else None, theta, beta, gamma, y, delta, d_out_ptr)


def run_pk_quotient(eng, key, cs, polys, sc):
    """one call over device copies of the witness polynomials -> the pieces as bytes"""
    import torch
    dev = {kind: device_slab(polys[kind]) for kind in WITNESS_KINDS}
    d_out = torch.zeros(32 * cs.n * (cs.degree - 1), dtype=torch.uint8, device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    pk_quotient(eng, key, witness_ptrs(dev), sc, d_out.data_ptr())
    eng.synchronize()
    return bytes(d_out.cpu().numpy())


def run_quotient_device(eng, vk, cs, polys, sc):
    import torch
    dev = [device_slab(polys[kind]) for kind in Q.POLY_KINDS]
    d_out = torch.zeros(32 * cs.n * (cs.degree - 1), dtype=torch.uint8, device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    quotient_device(eng, vk, [p for _t, p in dev], sc, d_out.data_ptr())
    eng.synchronize()
    return bytes(d_out.cpu().numpy())


# ---------------------------------------------------------------------------------------------- 1. the forms
@pytest.mark.parametrize("k,degree,n_perm,e", [(4, 3, 3, 1), (6, 6, 4, 3)])
def test_forms_against_python_integers(pkg, eng, poly, verifier, k, degree, n_perm, e):
    rng = random.Random(0xF00 + k)
    cs = Q.random_shape(rng, k, degree, n_perm, 1, True, BF)
    assert Q.extended_k(k, degree) == e
    polys = Q.random_inputs(rng, cs)
    n, u = cs.n, cs.n - BF - 1
    fixed_lag, sigma_lag = lagrange(polys, "fixed", k), lagrange(polys, "sigma", k)
    rows = [[int(i == 0) for i in range(n)], [int(i == u) for i in range(n)], [int(i > u) for i in range(n)]]
    rows_coeff = [Q.ntt(r, k, inverse=True) for r in rows]
    vk = make_vk(eng, verifier, cs)
    with key_of(eng, poly, vk, cs, polys) as key, key_of(eng, poly, vk, cs, polys, cosets=False) as lean:
        assert key.info == {"k": k, "e": e, "num_fixed": 2, "num_permutation_columns": n_perm, "forms": pkg.PK_COSETS,
                            "bytes": poly.pk_bytes(eng, vk)}
        assert lean.info["forms"] == 0 and lean.info["bytes"] == poly.pk_bytes(eng, vk, cosets=False) < key.info["bytes"]
        for obj in (key, lean):
            assert read_form(eng, *obj.ptr(pkg.PK_FIXED_LAGRANGE), k) == b"".join(cols(fixed_lag))
            assert read_form(eng, *obj.ptr(pkg.PK_SIGMA_LAGRANGE), k) == b"".join(cols(sigma_lag))
            assert obj.ptr(pkg.PK_FIXED_COEFF)[1] == 2 and obj.ptr(pkg.PK_SIGMA_COEFF)[1] == n_perm
            assert read_form(eng, *obj.ptr(pkg.PK_FIXED_COEFF), k) == b"".join(cols(Q.ntt(c, k, inverse=True) for c in fixed_lag))
            assert read_form(eng, *obj.ptr(pkg.PK_SIGMA_COEFF), k) == b"".join(cols(Q.ntt(c, k, inverse=True) for c in sigma_lag))
            assert read_form(eng, *obj.ptr(pkg.PK_LAGRANGE_COEFF), k) == b"".join(cols(rows_coeff))
        w_ext = Q.omega(k + e)
        for c in range(1 << e):
            s = Q.ZETA * pow(w_ext, c, R) % R
            want = [Q.ntt(p, k, s) for p in polys["fixed"] + polys["sigma"] + rows_coeff]
            ptr, columns = key.ptr(pkg.PK_COSET, c)
            assert columns == 2 + n_perm + 3
            assert read_form(eng, ptr, columns, k) == b"".join(cols(want)), "coset %d" % c
            # ... and every column is what the transform entry point gives for it
            assert poly.columns_coeff_to_extended(eng, cols(polys["sigma"][:1]), k, k, fe(s)) == cols(want[2:3])
    vk.close()


def test_sigma_forms_of_a_key_made_by_permutation_key(pkg, eng, poly, verifier):
    k, m = 5, 4
    cs = Q.random_shape(random.Random(0xF10), k, 4, m, 0, True, BF)
    u = cs.n - BF - 1
    copies = [(0, 1, 2, 3), (1, 0, 3, u - 1), (2, 3, 2, 7), (0, 5, 1, 5)]
    g, gl = eng.params_setup(k, fe(0x5EC12E7))
    sig_lag, sig_coeff, _commit = poly.permutation_key(eng, gl, poly.permutation_mapping(m, k, u, copies), m, k, u, fe(DELTA))
    fixed = cols([[random.Random(0xF11 + c).randrange(R) for _ in range(cs.n)] for c in range(2)])
    vk = make_vk(eng, verifier, cs)
    with poly.ProvingKey.from_lagrange(eng, vk, fixed, sig_lag) as key:
        assert read_form(eng, *key.ptr(pkg.PK_SIGMA_COEFF), k) == b"".join(sig_coeff)
        assert read_form(eng, *key.ptr(pkg.PK_FIXED_COEFF), k) == b"".join(poly.columns_lagrange_to_coeff(eng, fixed, k))
    # the same key from columns that are on the device already: the stores are not written
    with poly.ColumnStore(eng, 2 + m, k) as store:
        store.write(0, fixed + sig_lag)
        with poly.ProvingKey.from_views(eng, vk, store.view(0, 2), store.view(2, m)) as key:
            assert read_form(eng, *key.ptr(pkg.PK_SIGMA_COEFF), k) == b"".join(sig_coeff)
            assert read_form(eng, *key.ptr(pkg.PK_SIGMA_LAGRANGE), k) == b"".join(sig_lag)
        assert store.read() == fixed + sig_lag
    eng.bases_free(g)
    eng.bases_free(gl)
    vk.close()


# ---------------------------------------------------------------------------------------------- 2. the quotient
# no permutation; sets full and ragged; fixed columns among the permutation columns (perm >= 2, and two of them at >= 6);
# n below and above one workgroup; degree 3 / 4 / 6: e = 1, 2, 3
SHAPES = [  # k, degree, permutation columns, lookups, gates, challenges
    (4, 3, 0, 0, True, 2), (4, 3, 3, 1, False, 0), (4, 6, 5, 1, True, 2), (6, 4, 5, 2, False, 2), (6, 6, 0, 1, False, 0),
    (9, 4, 3, 0, True, 2), (9, 6, 9, 2, True, 0)]


@functools.lru_cache(maxsize=None)
def shape_reference(shape):
    """-> (cs, polys, scalars, quotient_py's pieces as bytes): made once per shape, shared, left unchanged"""
    k, degree, n_perm, n_lookups, with_gates, n_challenges = shape
    rng = random.Random(hash((0xF20,) + shape) & 0xFFFFFFFF)
    cs = Q.random_shape(rng, k, degree, n_perm, n_lookups, with_gates, BF, n_challenges)
    polys, sc = Q.random_inputs(rng, cs), Q.random_scalars(rng, n_challenges)
    want, _H = Q.quotient_py(cs, *Q.quotient_args(polys, sc))
    return cs, polys, sc, b"".join(cols(want))


def check_both_keys_on_both_endings(eng, poly, verifier, split_setting, cs, polys, sc, want):
    vk = make_vk(eng, verifier, cs)
    assert run_quotient_device(eng, vk, cs, polys, sc) == want, "h2agg_quotient_device"
    for cosets in (True, False):
        with key_of(eng, poly, vk, cs, polys, cosets) as key:
            for split in (0, 1):
                split_setting(split)
                assert run_pk_quotient(eng, key, cs, polys, sc) == want, "cosets %s, split %d" % (cosets, split)
            split_setting(0)
    vk.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_quotient_through_the_key(eng, poly, verifier, split_setting, shape):
    cs, polys, sc, want = shape_reference(shape)
    assert Q.extended_k(cs.k, cs.degree) == {3: 1, 4: 2, 6: 3}[cs.degree]
    if shape[2] >= 2:
        assert ("fixed", 1) in cs.permutation_columns[:shape[2]]
    if shape[2] >= 6:
        assert ("fixed", 0) in cs.permutation_columns[:shape[2]]
    check_both_keys_on_both_endings(eng, poly, verifier, split_setting, cs, polys, sc, want)


@pytest.mark.parametrize("which", ["no key column", "no witness column"])
def test_quotient_of_handmade_keys(eng, poly, verifier, split_setting, which):
    """F = 0 and P = 0: the key's coset slab is the three Lagrange columns alone.  Gates over fixed columns only and no advice,
    instance, permutation or lookup: nothing is transformed per coset."""
    k = 5
    if which == "no key column":
        A0, A1 = ("advice", 0), ("advice", 1)
        cs = Q.make_cs(k, 4, 2, 0, 1, [(0, 0), (1, 1)], [], [(0, 0)], [[("product", A0, ("sum", A1, ("neg", ("instance", 0))))]],
                       [([A0], [A1])], [], BF)
    else:
        F0, F1, F2 = ("fixed", 0), ("fixed", 1), ("fixed", 2)
        cs = Q.make_cs(k, 4, 0, 2, 0, [], [(0, 0), (1, 0), (1, -1)], [], [[("product", F0, ("sum", F1, ("neg", F2)))], [("scaled", F2, 5)]],
                       [], [], BF)
    rng = random.Random(0xF30 + len(which))
    polys, sc = Q.random_inputs(rng, cs), Q.random_scalars(rng)
    want, _H = Q.quotient_py(cs, *Q.quotient_args(polys, sc))
    assert any(any(p) for p in want)
    check_both_keys_on_both_endings(eng, poly, verifier, split_setting, cs, polys, sc, b"".join(cols(want)))


# ---------------------------------------------------------------------------------------------- 3. a satisfied circuit
@functools.lru_cache(maxsize=None)
def satisfied(k, degree):
    cs, lag, polys, sc = Q.satisfied_circuit(random.Random(0xD00 + k), k, degree)
    pieces, H = Q.quotient_py(cs, *Q.quotient_args(polys, sc))
    assert not any(H[(degree - 1) << k:])
    return cs, lag, polys, sc, pieces


@pytest.mark.parametrize("k,degree", [(5, 4), (8, 6)])
def test_quotient_of_a_satisfied_circuit_through_the_key(eng, poly, verifier, k, degree):
    cs, lag, polys, sc, want = satisfied(k, degree)
    vk = make_vk(eng, verifier, cs)
    ch, theta, beta, gamma, y, delta = scalars(sc)
    with poly.ProvingKey.from_lagrange(eng, vk, cols(lag["fixed"]), cols(lag["sigma"])) as key:
        got = key.quotient_pieces(*[cols(polys[kind]) for kind in WITNESS_KINDS], ch, theta, beta, gamma, y, delta)
        assert got == cols(want)
        assert [dec(p) for p in got] == want
    vk.close()


# ---------------------------------------------------------------------------------------------- 4. read-only, queued
def test_two_queued_calls_leave_the_key_and_the_inputs_as_they_were(pkg, eng, poly, verifier):
    import torch
    cs, _lag, polys, sc, want = satisfied(5, 4)
    other = dict(sc, theta=(sc["theta"] + 1) % R, beta=(sc["beta"] + 2) % R, gamma=(sc["gamma"] + 4) % R, y=(sc["y"] + 8) % R)
    polys2 = dict(polys, advice=[[(v + 1) % R for v in c] for c in polys["advice"]])
    want_other, _H = Q.quotient_py(cs, *Q.quotient_args(polys2, other))
    assert want_other != want
    vk = make_vk(eng, verifier, cs)
    with key_of(eng, poly, vk, cs, polys) as key:
        before = every_form(pkg, eng, key)
        assert len(before) == 5 + 4
        dev = {kind: device_slab(polys[kind]) for kind in WITNESS_KINDS}
        advice2 = device_slab(polys2["advice"])
        piece_bytes = 32 * cs.n * (cs.degree - 1)
        d_out = torch.zeros(2 * piece_bytes, dtype=torch.uint8, device=torch.device("cuda:0"))
        torch.cuda.synchronize()
        pk_quotient(eng, key, witness_ptrs(dev), sc, d_out.data_ptr())
        pk_quotient(eng, key, [advice2[1]] + witness_ptrs(dev)[1:], other, d_out.data_ptr() + piece_bytes)
        eng.synchronize()
        got = bytes(d_out.cpu().numpy())
        assert got[:piece_bytes] == b"".join(cols(want)), "first call"
        assert got[piece_bytes:] == b"".join(cols(want_other)), "second call"
        for kind in WITNESS_KINDS:
            assert bytes(dev[kind][0].cpu().numpy()) == b"".join(cols(polys[kind])), "an input changed"
        assert bytes(advice2[0].cpu().numpy()) == b"".join(cols(polys2["advice"]))
        assert every_form(pkg, eng, key) == before, "a form of the key changed"
    vk.close()


def test_two_keys_of_different_shapes_alternate_on_one_context(eng, poly, verifier):
    """the context's work memory is one buffer: the larger key regrows it, the smaller one runs in it afterwards"""
    refs = [shape_reference(SHAPES[1]), shape_reference(SHAPES[5])]
    vks = [make_vk(eng, verifier, cs) for cs, _p, _s, _w in refs]
    keys = [key_of(eng, poly, vk, cs, polys) for vk, (cs, polys, _s, _w) in zip(vks, refs)]
    assert keys[0].work_bytes() < keys[1].work_bytes()
    for _round in range(2):
        for key, (cs, polys, sc, want) in zip(keys, refs):
            assert run_pk_quotient(eng, key, cs, polys, sc) == want
    for key in keys:
        key.close()
    for vk in vks:
        vk.close()


# ---------------------------------------------------------------------------------------------- 5. the caller's stream
def test_pk_quotient_runs_on_the_callers_stream_and_does_not_wait(pkg, poly, verifier):
    """tests/stream_probe.py's probe, as tests/test_gpu_caller_stream.py runs it for h2agg_quotient_device: the context is on
    a held torch stream, the witness slabs hold a decoy until the true input arrives behind the hold"""
    import torch
    from tests.test_gpu_caller_stream import quotient_key, slab
    cs = quotient_key()
    assert cs.k == 4
    sc = Q.random_scalars(random.Random(0xA0F1))
    a, d = Q.random_inputs(random.Random(0xA0F2), cs), Q.random_inputs(random.Random(0xA0F3), cs)
    d = dict(d, fixed=a["fixed"], sigma=a["sigma"])          # one key: the decoy is another witness
    ref = lambda p: slab(Q.quotient_py(cs, *Q.quotient_args(p, sc))[0])
    want, want_decoy = ref(a), ref(d)
    assert want != want_decoy, "the decoy would pass for the true input"
    as_bytes = lambda p: b"".join(slab(p[kind]) for kind in WITNESS_KINDS)
    ctx = pkg.H2Agg(0)
    s = torch.cuda.Stream()
    ctx.set_stream(s.cuda_stream)
    vk = make_vk(ctx, verifier, cs)
    key = key_of(ctx, poly, vk, cs, a)
    try:
        d_in = torch.zeros(len(as_bytes(a)), dtype=torch.uint8, device=SP.device())
        d_out = torch.zeros(len(want), dtype=torch.uint8, device=SP.device())
        torch.cuda.synchronize()
        counts = {"advice": cs.num_advice_columns, "instance": cs.num_instance_columns, "perm_z": cs.num_permutation_sets,
                  "lookup_z": len(cs.lookups), "lookup_ap": len(cs.lookups), "lookup_sp": len(cs.lookups)}
        ptrs, at = [], d_in.data_ptr()
        for kind in WITNESS_KINDS:
            ptrs.append(at if counts[kind] else None)
            at += 32 * cs.n * counts[kind]
        call = lambda: pk_quotient(ctx, key, ptrs, sc, d_out.data_ptr())
        assert SP.probe(ctx, s, call, as_bytes(a), as_bytes(d), d_in, d_out) == want
    finally:
        key.close()
        vk.close()
        ctx.close()


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_context_usable(pkg, eng, poly, verifier):
    import torch
    cs, polys, sc, want = shape_reference(SHAPES[1])
    k = cs.k
    vk = make_vk(eng, verifier, cs)
    fixed, sigma = b"".join(cols(lagrange(polys, "fixed", k))), b"".join(cols(lagrange(polys, "sigma", k)))
    ch, theta, beta, gamma, y, delta = scalars(sc)
    key = key_of(eng, poly, vk, cs, polys)
    lean = key_of(eng, poly, vk, cs, polys, cosets=False)
    dev = {kind: device_slab(polys[kind]) for kind in WITNESS_KINDS}
    ptrs = witness_ptrs(dev)
    d_out = torch.zeros(len(want), dtype=torch.uint8, device=torch.device("cuda:0"))
    torch.cuda.synchronize()

    def refused(code, fn):
        with pytest.raises(pkg.H2AggError) as ei:
            fn()
        assert ei.value.code == code, ei.value
        assert run_pk_quotient(eng, key, cs, polys, sc) == want      # one good call on the same context

    def create_leaves_null(code, *args):
        out = pkg.C.c_void_p(0xDEAD)
        rc = eng._lib.h2agg_pk_create(eng._ctx, *args, pkg.C.byref(out))
        assert rc == code and not out.value
        assert run_pk_quotient(eng, key, cs, polys, sc) == want

    # a shape the quotient refuses (k + e > 28), unknown bits in forms, a null required slab
    big = make_vk(eng, verifier, Q.make_cs(23, 66, 1, 0, 0, [(0, 0)], [], [], [[("advice", 0)]], [], [], BF))
    create_leaves_null(pkg.ERR_INVALID, big._vk, None, None, 0)
    with pytest.raises(pkg.H2AggError) as ei:
        eng.pk_bytes(big, 0)
    assert ei.value.code == pkg.ERR_INVALID
    big.close()
    create_leaves_null(pkg.ERR_INVALID, vk._vk, fixed, sigma, 2)
    create_leaves_null(pkg.ERR_INVALID, vk._vk, fixed, sigma, pkg.PK_COSETS | 4)
    create_leaves_null(pkg.ERR_INVALID, vk._vk, None, sigma, pkg.PK_COSETS)
    create_leaves_null(pkg.ERR_INVALID, vk._vk, fixed, None, pkg.PK_COSETS)
    create_leaves_null(pkg.ERR_INVALID, None, fixed, sigma, pkg.PK_COSETS)
    refused(pkg.ERR_INVALID, lambda: eng.pk_create_resident(vk, None, None))
    # a key used with another context
    other = pkg.H2Agg(0)
    try:
        with pytest.raises(pkg.H2AggError) as ei:
            pk_quotient(other, key, ptrs, sc, d_out.data_ptr())
        assert ei.value.code == pkg.ERR_INVALID
    finally:
        other.close()
    # an unknown form, a coset out of range, COSET of the low-memory key
    refused(pkg.ERR_INVALID, lambda: key.ptr(6))
    refused(pkg.ERR_INVALID, lambda: key.ptr(-1))
    refused(pkg.ERR_INVALID, lambda: key.ptr(pkg.PK_COSET, 1 << key.info["e"]))
    refused(pkg.ERR_INVALID, lambda: lean.ptr(pkg.PK_COSET, 0))
    assert key.ptr(pkg.PK_FIXED_COEFF, 99)[1] == 2           # (coset is ignored for the other forms)
    # a null required buffer of the call
    for hole in range(len(ptrs)):
        args = list(ptrs)
        args[hole] = None
        refused(pkg.ERR_INVALID, lambda: pk_quotient(eng, key, args, sc, d_out.data_ptr()))
    refused(pkg.ERR_INVALID, lambda: pk_quotient(eng, key, ptrs, sc, None))
    # a scalar >= r
    for hole in range(5):
        sc5 = [theta, beta, gamma, y, delta]
        sc5[hole] = enc([R])
        refused(pkg.ERR_NONCANONICAL, lambda: eng.pk_quotient(key.handle, *ptrs, None, *sc5, d_out.data_ptr()))
    # a witness element >= r: at h2agg_synchronize, once
    bad = dict(polys, lookup_sp=[[(1 << 256) - 1 if i == 7 else v for i, v in enumerate(polys["lookup_sp"][0])]])
    bad_dev = {kind: device_slab(bad[kind]) for kind in WITNESS_KINDS}
    torch.cuda.synchronize()
    for obj in (key, lean):
        pk_quotient(eng, obj, witness_ptrs(bad_dev), sc, d_out.data_ptr())
        with pytest.raises(pkg.H2AggError) as ei:
            eng.synchronize()
        assert ei.value.code == pkg.ERR_NONCANONICAL
        eng.synchronize()
        assert run_pk_quotient(eng, obj, cs, polys, sc) == want
    lean.close()
    key.close()
    vk.close()


def test_create_refuses_a_noncanonical_element_and_nothing_leaks(pkg, eng, poly, verifier):
    """k = 12: one key holds 5.6 MiB, so a key left behind by one of the 20 refusals or 50 destroys would show far above the
    2 MiB the device allocator hands memory out in"""
    import torch
    k = 12
    cs = Q.random_shape(random.Random(0xF60), k, 4, 3, 0, True, BF)
    rnd = random.Random(0xF61)
    good = [enc([rnd.randrange(R) for _ in range(cs.n)]) for _ in range(5)]
    fixed, sigma = b"".join(good[:2]), b"".join(good[2:])
    vk = make_vk(eng, verifier, cs)
    assert poly.pk_bytes(eng, vk) == 32 * cs.n * (2 * 5 + 3 + 4 * 8) > 5 << 20
    eng.pk_destroy(eng.pk_create(vk, fixed, sigma))              # (the context's transform work memory grows here)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    bad_fixed = fixed[:32 * 9] + enc([R]) + fixed[32 * 10:]
    bad_sigma = sigma[:-32] + enc([(1 << 256) - 1])
    for i in range(20):
        out = pkg.C.c_void_p(0xDEAD)
        args = (bad_fixed, sigma) if i % 2 else (fixed, bad_sigma)
        assert eng._lib.h2agg_pk_create(eng._ctx, vk._vk, *args, pkg.PK_COSETS if i % 4 < 2 else 0, pkg.C.byref(out)) == pkg.ERR_NONCANONICAL
        assert not out.value
    eng.synchronize()                                            # clean: the refusal reported the status itself
    assert abs(torch.cuda.mem_get_info()[0] - free0) <= 2 << 20
    for _ in range(50):
        h = eng.pk_create(vk, fixed, sigma)
        eng.pk_destroy(h)
        assert not h
    assert abs(torch.cuda.mem_get_info()[0] - free0) <= 2 << 20
    eng.pk_destroy(pkg.C.c_void_p())                             # NULL does nothing
    vk.close()


# ---------------------------------------------------------------------------------------------- 7. the phase line
@pytest.mark.parametrize("cosets", [True, False])
def test_phase_line_has_the_five_names(eng, poly, verifier, cosets):
    cs, polys, sc, want = shape_reference(SHAPES[3])
    vk = make_vk(eng, verifier, cs)
    with key_of(eng, poly, vk, cs, polys, cosets) as key:
        eng.debug_configure("phases", 1)
        try:
            assert run_pk_quotient(eng, key, cs, polys, sc) == want
            line = eng.last_phases()
        finally:
            eng.debug_configure("phases", 0)
        assert [kv.split("=")[0] for kv in line.split()] == PHASE_NAMES
        assert all(float(kv.split("=")[1]) >= 0 for kv in line.split())
    vk.close()


# ---------------------------------------------------------------------------------------------- 8. an honest proof
class KeyedStages(HP.DeviceStages):
    """DeviceStages whose quotient goes through one poly.ProvingKey, built from the Key's Lagrange forms when the first proof
    loads its verifying key and kept for the proofs after it"""

    def __init__(self, *args):
        super().__init__(*args)
        self.pk, self.built, self._lagrange = None, 0, None

    def keygen(self, circuit):
        key = super().keygen(circuit)
        self._lagrange = (circuit.lag["fixed"], key.sigma_lag)
        return key

    def load_key(self, cs):
        if self.vk is not None:
            assert cs.vk_scalar == self.cs.vk_scalar, "another key"
            return
        super().load_key(cs)
        self.cs = cs
        self.pk = self.poly.ProvingKey.from_lagrange(self.eng, self.vk, self._cols(self._lagrange[0]), self._cols(self._lagrange[1]))
        self.built += 1

    def quotient(self, polys, scalars):
        sc = scalars
        return self._ints(self.pk.quotient_pieces(*[self._cols(polys[kind]) for kind in WITNESS_KINDS], [], fe(sc["theta"]),
                                                  fe(sc["beta"]), fe(sc["gamma"]), fe(sc["y"]), fe(sc["delta"])))

    def close(self):
        if self.pk is not None:
            self.pk.close()
            self.pk = None
        super().close()


@pytest.mark.parametrize("k", [5, 7])
def test_two_honest_proofs_through_one_key(pkg, eng, poly, verifier, k):
    from tests.test_gpu_honest_proofs import TAU, verdicts
    setup = HP.Setup(k, TAU, HP.INSTANCE_ROWS)
    first = HP.make_circuit(random.Random(0xF80 + k), k, 4)
    # another witness of the same key: a cell of advice column c on the last row, which no gate, copy or lookup constrains
    second = first.with_cell("advice", 2, first.cs.n - 1, first.lag["advice"][2][first.cs.n - 1] + 1)
    memo = {}
    want = [HP.prove(c, setup, HP.PyStages(setup, memo), random.Random(seed)) for c, seed in ((first, 1), (second, 2))]
    assert want[0].data != want[1].data
    stages = KeyedStages(pkg, eng, poly, verifier, setup)
    try:
        got = [HP.prove(c, setup, stages, random.Random(seed)) for c, seed in ((first, 1), (second, 2))]
        assert stages.built == 1 and stages.pk.cosets
    finally:
        stages.close()
    for g, w in zip(got, want):
        assert HP.first_difference(g, w) is None, "first differing field: %s" % HP.first_difference(g, w)
        assert g.data == w.data
    each, agg = verdicts(eng, verifier, {k: setup}, [got])
    assert [(status, ok) for _pair, status, ok in each] == [(0, True), (0, True)] and agg is True
