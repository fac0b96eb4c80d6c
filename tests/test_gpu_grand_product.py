"""GPU: grand products — h2agg_fr_batch_invert, h2agg_fr_grand_product, h2agg_permutation_product, h2agg_lookup_product, their
_device twins, and poly.py over them.

halo2_proofs is not vendored in the reference, so the yardstick is the definition in include/h2agg.h, restated with Python
integers in tests/grand_product_ref.py (one pow(x, r - 2, r) per element), which tests/test_grand_product_host.py ties to
the identities the reference's verifier checks.  Everything is exact and compared byte for byte.  The Z column is then
committed, opened and put through the verifier path of tests/test_gpu_poly_open.py.

(H2AGG_ERR_NOMEM is the one refusal of the header's list that is not tried: every argument the entry points accept asks for
at most 16 GiB of work memory, which the device has; there is no call that reaches it.)"""
import ctypes as C
import importlib
import random

import pytest

import __graft_entry__ as entry
from oracle import bn254 as O
from oracle import pairing as E
from tests.fr_bytes import dec, enc, fe
from tests.grand_product_ref import (BIG, DELTA, R, batch_invert_py, grand_product_py, lookup_product_py, omega,
                                     permutation_chain_py, permutation_product_py, permuted_pair, satisfied_permutation)
from tests.poly_open_ref import BIG_Z, horner, quotient_py, random_input
from tests.test_gpu_fr_fft import ntt_py

pytestmark = pytest.mark.gpu

T = 1 << 11
BETA, GAMMA = 0x1234567 * 0x89ABCDEF0123 % R, (R - 0xFEDCBA987 * 0x13579BDF)
ONE = fe(1)


@pytest.fixture(scope="module")
def poly(pkg):
    return importlib.import_module(entry.PKG_NAME + ".poly")


class chunk:
    """the debug key fr_scan_chunk for the length of a with-block"""

    def __init__(self, eng, t):
        self.eng, self.t = eng, t

    def __enter__(self):
        self.eng.debug_configure("fr_scan_chunk", self.t)

    def __exit__(self, *exc):
        self.eng.debug_configure("fr_scan_chunk", 0)


# ---------------------------------------------------------------------------------------------- batch_invert
def invert_inputs(seed, n, t):
    rng = random.Random(seed)
    base = [rng.randrange(1, R) for _ in range(n)]
    out = [base, [1] * n, [R - 1] * n, [0] * n]
    for pos in sorted({0, n - 1, t - 1, t}):
        if 0 <= pos < n:
            a = list(base)
            a[pos] = 0
            out.append(a)
    if n > t:                                            # one whole chunk of zeros
        a = list(base)
        a[t:2 * t] = [0] * len(a[t:2 * t])
        out.append(a)
    return out


def check_invert(eng, seed, n, t):
    memo = {}                                             # the inputs share most elements: one pow per distinct value
    for xs in invert_inputs(seed, n, t):
        for x in set(xs) - set(memo):
            memo[x] = batch_invert_py([x])[0]
        want = [memo[x] for x in xs]
        assert all(x * y % R == (1 if x else 0) for x, y in zip(xs, want))     # for every non-zero element, in * out == 1
        got = eng.fr_batch_invert(enc(xs))
        assert got == enc(want), (n, t)
        buf = bytearray(enc(xs))                          # in place
        assert eng.fr_batch_invert(buf) is buf and bytes(buf) == got


@pytest.mark.parametrize("n", [0, 1, 2, 7, 8, 9, T - 1, T, T + 1, 3 * T + 5, 1 << 13])
def test_batch_invert_default_chunk(eng, pkg, n):
    assert pkg.FR_SCAN_CHUNK == 11
    check_invert(eng, 100 + n, n, T)


@pytest.mark.parametrize("t", [3, 4])
@pytest.mark.parametrize("n", [63, 64, 65, 513, 1000, 1024])
def test_batch_invert_small_chunks(eng, t, n):
    with chunk(eng, t):
        check_invert(eng, 200 + 16 * t + n, n, 1 << t)


def test_batch_invert_py(eng, poly):
    xs = [3, 0, R - 2, BIG]
    assert poly.batch_invert(eng, enc(xs)) == enc(batch_invert_py(xs))


# ---------------------------------------------------------------------------------------------- grand_product
def check_grand_product(eng, seed, k):
    rng = random.Random(seed)
    n = 1 << k
    num = [rng.randrange(1, R) for _ in range(n)]
    den = [rng.randrange(1, R) for _ in range(n)]
    us = sorted({u for u in (0, 1, n // 2, n - 6, n - 1) if 0 <= u < n})
    cases = [(num, None), (num, den)]
    if n >= 4:
        zn = list(num)
        zn[n // 2 - 1] = 0                               # a zero in num in the middle: everything after it is 0
        zd = list(den)
        zd[n // 2 - 1] = 0                               # a zero in den: inv(0) = 0, the same
        cases += [(zn, den), (num, zd)]
    for a, b in cases:
        for init in (1, BIG):
            full = grand_product_py(a, b, n - 1, init)   # a shorter u is a prefix of it
            if n >= 4 and 0 in a + (b or []):
                assert full[n // 2 - 1] != 0 and set(full[n // 2:]) == {0}
            for u in us:
                out, last = eng.fr_grand_product(enc(a[:u]), None if b is None else enc(b[:u]), k, u, fe(init))
                assert out == enc(full[:u + 1]) and last == fe(full[u]), (k, u, init, b is None)


@pytest.mark.parametrize("k", range(0, 14))
def test_grand_product_default_chunk(eng, k):
    check_grand_product(eng, 300 + k, k)


@pytest.mark.parametrize("t", [3, 4])
@pytest.mark.parametrize("k", [6, 9, 10])
def test_grand_product_small_chunks(eng, t, k):
    with chunk(eng, t):
        check_grand_product(eng, 400 + 16 * t + k, k)


@pytest.mark.parametrize("k,t,u", [(5, 0, 20), (12, 0, (1 << 12) - 6), (9, 3, 511)])
def test_grand_product_device_aliasing_and_untouched_rows(eng, k, t, u):
    """out aliasing num; elements of out beyond u + 1 left as the caller filled them; d_last; den NULL"""
    import torch
    dev = torch.device("cuda:0")
    rng = random.Random(500 + k)
    n = 1 << k
    num = [rng.randrange(R) for _ in range(n)]
    den = [rng.randrange(1, R) for _ in range(n)]
    want = grand_product_py(num, den, u, BIG)
    plain = grand_product_py(num, None, u, 1)
    fill = bytes([0xA5]) * 32
    d_num = torch.frombuffer(bytearray(enc(num)), dtype=torch.uint8).to(dev)
    d_den = torch.frombuffer(bytearray(enc(den)), dtype=torch.uint8).to(dev)
    d_io = d_num.clone()
    d_out = torch.frombuffer(bytearray(fill * n), dtype=torch.uint8).to(dev)
    d_out2 = torch.frombuffer(bytearray(fill * n), dtype=torch.uint8).to(dev)
    d_last = torch.zeros(32, dtype=torch.uint8, device=dev)
    d_last2 = torch.zeros(32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with chunk(eng, t):
        eng.fr_grand_product_device(d_num.data_ptr(), d_den.data_ptr(), k, u, fe(BIG), d_out.data_ptr(), d_last.data_ptr())
        eng.fr_grand_product_device(d_num.data_ptr(), None, k, u, ONE, d_out2.data_ptr(), d_last2.data_ptr())   # other constants, queued behind
        eng.fr_grand_product_device(d_io.data_ptr(), d_den.data_ptr(), k, u, fe(BIG), d_io.data_ptr(), None)     # out is num
        eng.synchronize()
    assert bytes(d_out.cpu().numpy()) == enc(want) + fill * (n - u - 1)
    assert bytes(d_out2.cpu().numpy()) == enc(plain) + fill * (n - u - 1)
    assert bytes(d_last.cpu().numpy()) == fe(want[u]) and bytes(d_last2.cpu().numpy()) == fe(plain[u])
    assert bytes(d_io.cpu().numpy()) == enc(want) + enc(num[u + 1:])
    assert bytes(d_num.cpu().numpy()) == enc(num) and bytes(d_den.cpu().numpy()) == enc(den), "an input changed"


def test_batch_invert_device_in_and_out_of_place(eng):
    import torch
    dev = torch.device("cuda:0")
    n = 3 * T + 5
    xs = invert_inputs(600, n, T)[-1]
    d_in = torch.frombuffer(bytearray(enc(xs)), dtype=torch.uint8).to(dev)
    d_io, d_out = d_in.clone(), torch.zeros_like(d_in)
    torch.cuda.synchronize()
    eng.fr_batch_invert_device(d_in.data_ptr(), n, d_out.data_ptr())
    eng.fr_batch_invert_device(d_io.data_ptr(), n, d_io.data_ptr())
    eng.fr_batch_invert_device(0, 0, 0)                   # n == 0: a no-op
    eng.synchronize()
    want = enc(batch_invert_py(xs))
    assert bytes(d_out.cpu().numpy()) == want and bytes(d_io.cpu().numpy()) == want
    assert bytes(d_in.cpu().numpy()) == enc(xs)


# ---------------------------------------------------------------------------------------------- three families, one queue
@pytest.mark.parametrize("k,t", [(7, 3), (12, 0)])
def test_fft_divide_invert_queued_back_to_back(eng, k, t):
    """fr_fft_device -> fr_poly_divide_device -> fr_batch_invert_device on one context, each output the next call's input,
    nothing synchronised in between.  The three families share the level plan and the staging of csrc/fr_host.inc but no
    level buffer: nothing of one call may show in the next.  t = 3 at k = 7 is the three-launch plan 128 -> 16 -> 2 -> 1 of
    both chunked sweeps; t = 0 is the default chunk.  z has 254 bits; the quotient's top coefficient is the inversion's zero."""
    import torch
    dev = torch.device("cuda:0")
    n = 1 << k
    a = random_input(700 + k, k)
    evals = ntt_py(a, k)
    quot, rem = quotient_py(evals, BIG_Z), horner(evals, BIG_Z)
    assert quot[n - 1] == 0 and BIG_Z.bit_length() == 254
    want = batch_invert_py(quot)
    d_a = torch.frombuffer(bytearray(enc(a)), dtype=torch.uint8).to(dev)
    d_evals, d_quot, d_inv = torch.zeros_like(d_a), torch.zeros_like(d_a), torch.zeros_like(d_a)
    d_rem = torch.zeros(32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eng.debug_configure("fr_poly_chunk", t)
    eng.debug_configure("fr_scan_chunk", t)
    try:
        eng.fr_fft_device(d_a.data_ptr(), k, False, None, d_evals.data_ptr())
        eng.fr_poly_divide_device(d_evals.data_ptr(), k, fe(BIG_Z), d_quot.data_ptr(), d_rem.data_ptr())
        eng.fr_batch_invert_device(d_quot.data_ptr(), n, d_inv.data_ptr())
        eng.synchronize()
    finally:
        eng.debug_configure("fr_poly_chunk", 0)
        eng.debug_configure("fr_scan_chunk", 0)
    assert bytes(d_evals.cpu().numpy()) == enc(evals)
    assert bytes(d_quot.cpu().numpy()) == enc(quot) and bytes(d_rem.cpu().numpy()) == fe(rem)
    assert bytes(d_inv.cpu().numpy()) == enc(want)
    assert bytes(d_a.cpu().numpy()) == enc(a), "the input changed"


# ---------------------------------------------------------------------------------------------- permutation / lookup
class Satisfied:
    """the construction of tests/test_grand_product_host.py (m = 5, chunk_len = 2, u = n - 6), computed once per k"""

    def __init__(self, k):
        self.k, self.m, self.c = k, 5, 2
        self.n, self.u = 1 << k, (1 << k) - 6
        self.values, self.sigmas = satisfied_permutation(0x700 + k, k, self.m, self.u)
        self.zs = permutation_chain_py(self.values, self.sigmas, k, self.u, BETA, GAMMA, DELTA, self.c)
        assert self.zs[-1][self.u] == 1
        self.pair = permuted_pair(0x710 + k, k, self.u)
        self.lz = lookup_product_py(*self.pair, self.u, BETA, GAMMA)
        assert self.lz[self.u] == 1


@pytest.fixture(scope="module", params=[(6, 0), (10, 3)], ids=["k6", "k10-chunk3"])
def sat(request):
    k, t = request.param
    s = Satisfied(k)
    s.t = t
    return s


def test_permutation_products_satisfied(eng, poly, sat):
    s = sat
    blind = [enc([0xB000 + 16 * q + i for i in range(s.n - s.u - 1)]) for q in range(3)]
    with chunk(eng, s.t):
        cols = poly.permutation_products(eng, [enc(v) for v in s.values], [enc(v) for v in s.sigmas], s.k, s.u, fe(BETA),
                                         fe(GAMMA), fe(DELTA), s.c, blinding=blind)
        bare = poly.permutation_products(eng, [enc(v) for v in s.values], [enc(v) for v in s.sigmas], s.k, s.u, fe(BETA),
                                         fe(GAMMA), fe(DELTA), s.c)
    assert len(cols) == 3
    for q in range(3):
        assert cols[q] == enc(s.zs[q]) + blind[q] and bare[q] == enc(s.zs[q]) + bytes(32 * (s.n - s.u - 1))
    assert cols[2][32 * s.u:32 * s.u + 32] == ONE                           # the final z[u] == 1


def test_permutation_product_unsatisfied_and_column_counts(eng, sat):
    s = sat
    rng = random.Random(0x720 + s.k)
    for m in (1, 16):
        values = [[rng.randrange(R) for _ in range(s.n)] for _ in range(m)]
        sigmas = [[rng.randrange(R) for _ in range(s.n)] for _ in range(m)]
        df = pow(DELTA, 7, R)
        want = permutation_product_py(values, sigmas, s.k, s.u, BETA, GAMMA, DELTA, df, BIG)
        with chunk(eng, s.t):
            z, last = eng.permutation_product(b"".join(enc(v) for v in values), b"".join(enc(v) for v in sigmas), m, s.k, s.u,
                                              fe(BETA), fe(GAMMA), fe(DELTA), fe(df), fe(BIG))
        assert z == enc(want) and last == fe(want[s.u]), m


def test_lookup_product_satisfied_and_random(eng, poly, sat):
    s = sat
    a, t, ap, sp = s.pair
    blind = enc([0xC000 + i for i in range(s.n - s.u - 1)])
    rng = random.Random(0x730 + s.k)
    rnd = [[rng.randrange(R) for _ in range(s.n)] for _ in range(4)]
    want = lookup_product_py(*rnd, s.u, BETA, GAMMA)
    with chunk(eng, s.t):
        col = poly.lookup_product(eng, enc(a), enc(t), enc(ap), enc(sp), s.k, s.u, fe(BETA), fe(GAMMA), blinding=blind)
        z, last = eng.lookup_product(*[enc(c) for c in rnd], s.k, s.u, fe(BETA), fe(GAMMA))
    assert col == enc(s.lz) + blind and col[32 * s.u:32 * s.u + 32] == ONE
    assert z == enc(want) and last == fe(want[s.u]) and want[s.u] != 1


def test_device_calls_queued_back_to_back(eng, sat):
    """two calls with different constants and no synchronisation between them: both right (constants go by value)"""
    import torch
    dev = torch.device("cuda:0")
    s = sat
    up = lambda cols: torch.frombuffer(bytearray(b"".join(enc(c) for c in cols)), dtype=torch.uint8).to(dev)
    d_v, d_s = up(s.values[:2]), up(s.sigmas[:2])
    d_l = [up([c]) for c in s.pair]
    outs = [torch.zeros(32 * s.n, dtype=torch.uint8, device=dev) for _ in range(4)]
    lasts = [torch.zeros(32, dtype=torch.uint8, device=dev) for _ in range(4)]
    beta2, gamma2, df2 = (BETA * 3 + 1) % R, (GAMMA * 5 + 2) % R, pow(DELTA, 4, R)
    torch.cuda.synchronize()
    with chunk(eng, s.t):
        eng.permutation_product_device(d_v.data_ptr(), d_s.data_ptr(), 2, s.k, s.u, fe(BETA), fe(GAMMA), fe(DELTA), ONE, ONE,
                                       outs[0].data_ptr(), lasts[0].data_ptr())
        eng.permutation_product_device(d_v.data_ptr(), d_s.data_ptr(), 2, s.k, s.u, fe(beta2), fe(gamma2), fe(DELTA), fe(df2),
                                       fe(BIG), outs[1].data_ptr(), lasts[1].data_ptr())
        eng.lookup_product_device(*[d.data_ptr() for d in d_l], s.k, s.u, fe(BETA), fe(GAMMA), outs[2].data_ptr(), lasts[2].data_ptr())
        eng.lookup_product_device(*[d.data_ptr() for d in d_l], s.k, s.u, fe(beta2), fe(gamma2), outs[3].data_ptr(), lasts[3].data_ptr())
        eng.synchronize()
    want = [s.zs[0],
            permutation_product_py(s.values[:2], s.sigmas[:2], s.k, s.u, beta2, gamma2, DELTA, df2, BIG),
            s.lz, lookup_product_py(*s.pair, s.u, beta2, gamma2)]
    for q in range(4):
        assert bytes(outs[q].cpu().numpy()) == enc(want[q]) + bytes(32 * (s.n - s.u - 1)), q
        assert bytes(lasts[q].cpu().numpy()) == fe(want[q][s.u]), q


# ---------------------------------------------------------------------------------------------- closing the loop
def test_z_column_commits_opens_and_verifies(eng, pkg, poly):
    """the permutation Z of the k = 6 construction: lagrange_to_coeff, commit_coeff, multiopen_prove at x and w x; the opened
    values are z(x) and z(w x) by Python evaluation; the pair passes batch_multi_open / evaluate_multiopen_proof / the pairing"""
    s = Satisfied(6)
    rng = random.Random(0x740)
    tau = rng.randrange(2, R)
    g, gl = eng.params_setup(s.k, fe(tau))
    try:
        z_col = poly.permutation_products(eng, [enc(v) for v in s.values], [enc(v) for v in s.sigmas], s.k, s.u, fe(BETA),
                                          fe(GAMMA), fe(DELTA), s.c)[0]
        assert z_col == enc(s.zs[0]) + bytes(32 * (s.n - s.u - 1))
        coeffs = poly.lagrange_to_coeff(eng, z_col, s.k)
        commit = eng.g1_batch_to_affine(poly.commit_coeff(eng, g, coeffs))
        assert commit == eng.g1_batch_to_affine(poly.commit_lagrange(eng, gl, z_col))
        x = rng.randrange(R)
        wx = omega(s.k) * x % R
        queries, points, v, u = [(0, 0), (0, 1)], fe(x) + fe(wx), fe(rng.randrange(R)), fe(rng.randrange(R))
        evals, _groups, ws = poly.multiopen_prove(eng, g, coeffs, s.k, queries, points, v)
        assert evals == [fe(horner(dec(coeffs), x)), fe(horner(dec(coeffs), wx))]
        # z(w^i) is row i of the column: the evaluations are those of the polynomial that interpolates the device's Z
        assert horner(dec(coeffs), pow(omega(s.k), 3, R)) == s.zs[0][3]
        g2 = b"".join(O.fe_to_bytes(c) for c in (E.G2[0][0], E.G2[0][1], E.G2[1][0], E.G2[1][1]))
        s_g2 = pkg.g2_scalar_mul(g2, fe(tau))

        def verify(evals):
            b = pkg.SchemaBuilder(eng)
            try:
                nodes = b.evaluation_queries(["z", "z"], commit + commit, b"".join(evals))
                w_x, w_g = b.batch_multi_open("zloop", [0, 1], points, nodes, b"".join(ws), v, u)
                left, right, _names = b.evaluate_multiopen_proof(w_x, w_g)
                return eng.final_pair_check(left, right, s_g2, g2)
            finally:
                b.close()

        assert verify(evals)
        assert not verify([evals[0], fe(int.from_bytes(evals[1], "little") + 1)])
    finally:
        eng.bases_free(g)
        eng.bases_free(gl)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_context_usable(eng, pkg):
    import torch
    lib, ctx = eng._lib, eng._ctx
    k, u = 4, 10
    rng = random.Random(0x750)
    col = lambda: [rng.randrange(1, R) for _ in range(1 << k)]
    num, den = col(), col()
    good = enc(grand_product_py(num, den, u, 1))
    vals, sigs = [col(), col()], [col(), col()]
    pz = enc(permutation_product_py(vals, sigs, k, u, BETA, GAMMA, DELTA, 1, 1))
    lcols = [col() for _ in range(4)]
    lz = enc(lookup_product_py(*lcols, u, BETA, GAMMA))
    slab = lambda cols: b"".join(enc(c) for c in cols)

    def still_works():
        assert eng.fr_batch_invert(enc(num)) == enc(batch_invert_py(num))
        assert eng.fr_grand_product(enc(num[:u]), enc(den[:u]), k, u, ONE)[0] == good
        assert eng.permutation_product(slab(vals), slab(sigs), 2, k, u, fe(BETA), fe(GAMMA), fe(DELTA), ONE, ONE)[0] == pz
        assert eng.lookup_product(*[enc(c) for c in lcols], k, u, fe(BETA), fe(GAMMA))[0] == lz

    def refused(code, fn, *args):
        with pytest.raises(pkg.H2AggError) as ei:
            fn(*args)
        assert ei.value.code == code, ei.value
        still_works()

    big = R.to_bytes(32, "little")
    buf, last = C.create_string_buffer(32 * 2 * (1 << k)), C.create_string_buffer(32)
    p = C.cast(buf, C.c_void_p)
    perm = lambda **kw: eng.permutation_product(kw.get("values", slab(vals)), kw.get("sigmas", slab(sigs)), kw.get("m", 2),
                                                kw.get("k", k), kw.get("u", u), kw.get("beta", fe(BETA)), kw.get("gamma", fe(GAMMA)),
                                                kw.get("delta", fe(DELTA)), kw.get("delta_first", ONE), kw.get("init", ONE))
    look = lambda **kw: eng.lookup_product(*kw.get("cols", [enc(c) for c in lcols]), kw.get("k", k), kw.get("u", u),
                                           kw.get("beta", fe(BETA)), kw.get("gamma", fe(GAMMA)))
    # k > 24, n > 2^24, u >= 2^k
    refused(pkg.ERR_INVALID, eng.fr_grand_product, enc(num[:u]), None, 25, u, ONE)
    refused(pkg.ERR_INVALID, lambda: perm(k=25))
    refused(pkg.ERR_INVALID, lambda: look(k=25))
    refused(pkg.ERR_INVALID, lambda: eng._check(lib.h2agg_fr_batch_invert(ctx, p, (1 << 24) + 1, p)))
    refused(pkg.ERR_INVALID, lambda: eng._check(lib.h2agg_fr_batch_invert_device(ctx, p, (1 << 24) + 1, p)))
    refused(pkg.ERR_INVALID, eng.fr_grand_product, enc(num), None, k, 1 << k, ONE)
    refused(pkg.ERR_INVALID, lambda: perm(u=1 << k))
    refused(pkg.ERR_INVALID, lambda: look(u=1 << k))
    # m == 0, m > 16
    refused(pkg.ERR_INVALID, lambda: perm(m=0))
    refused(pkg.ERR_INVALID, lambda: perm(m=17))
    # a null required buffer
    refused(pkg.ERR_INVALID, lambda: eng._check(lib.h2agg_fr_batch_invert(ctx, None, 4, p)))
    refused(pkg.ERR_INVALID, lambda: eng._check(lib.h2agg_fr_batch_invert(ctx, p, 4, None)))
    refused(pkg.ERR_INVALID, lambda: eng._check(lib.h2agg_fr_batch_invert_device(ctx, None, 4, None)))
    refused(pkg.ERR_INVALID, lambda: eng._check(lib.h2agg_fr_grand_product(ctx, None, None, k, u, ONE, p, last)))
    refused(pkg.ERR_INVALID, lambda: eng._check(lib.h2agg_fr_grand_product(ctx, p, None, k, u, None, p, last)))
    refused(pkg.ERR_INVALID, lambda: eng._check(lib.h2agg_fr_grand_product(ctx, p, None, k, u, ONE, None, last)))
    refused(pkg.ERR_INVALID, lambda: eng._check(lib.h2agg_fr_grand_product_device(ctx, None, None, k, u, ONE, None, None)))
    refused(pkg.ERR_INVALID, lambda: eng._check(lib.h2agg_permutation_product(ctx, p, None, 2, k, u, ONE, ONE, ONE, ONE, ONE, p, last)))
    refused(pkg.ERR_INVALID, lambda: eng._check(lib.h2agg_permutation_product(ctx, p, p, 2, k, u, ONE, None, ONE, ONE, ONE, p, last)))
    refused(pkg.ERR_INVALID, lambda: eng._check(lib.h2agg_permutation_product_device(ctx, None, None, 2, k, u, ONE, ONE, ONE, ONE, ONE, None, None)))
    refused(pkg.ERR_INVALID, lambda: eng._check(lib.h2agg_lookup_product(ctx, p, p, None, p, k, u, ONE, ONE, p, last)))
    refused(pkg.ERR_INVALID, lambda: eng._check(lib.h2agg_lookup_product(ctx, p, p, p, p, k, u, None, ONE, p, last)))
    refused(pkg.ERR_INVALID, lambda: eng._check(lib.h2agg_lookup_product_device(ctx, None, None, None, None, k, u, ONE, ONE, None, None)))
    # a constant >= r: from the call
    refused(pkg.ERR_NONCANONICAL, eng.fr_grand_product, enc(num[:u]), None, k, u, big)
    for name in ("beta", "gamma", "delta", "delta_first", "init"):
        refused(pkg.ERR_NONCANONICAL, lambda: perm(**{name: big}))
    for name in ("beta", "gamma"):
        refused(pkg.ERR_NONCANONICAL, lambda: look(**{name: big}))
    # a column element >= r: from the call for the synchronous entry points
    bad = enc(num[:3]) + big + enc(num[4:])
    refused(pkg.ERR_NONCANONICAL, eng.fr_batch_invert, bad)
    refused(pkg.ERR_NONCANONICAL, eng.fr_grand_product, bad[:32 * u], enc(den[:u]), k, u, ONE)
    refused(pkg.ERR_NONCANONICAL, eng.fr_grand_product, enc(num[:u]), bad[:32 * u], k, u, ONE)
    refused(pkg.ERR_NONCANONICAL, lambda: perm(values=bad + enc(vals[1])))
    refused(pkg.ERR_NONCANONICAL, lambda: perm(sigmas=enc(sigs[0]) + bad))
    for q in range(4):
        cols = [enc(c) for c in lcols]
        cols[q] = bad
        refused(pkg.ERR_NONCANONICAL, lambda: look(cols=cols))
    # ... and at h2agg_synchronize for a queued one, once
    d = torch.frombuffer(bytearray(bad), dtype=torch.uint8).to(torch.device("cuda:0"))
    d_out = torch.zeros_like(d)
    torch.cuda.synchronize()
    with pytest.raises(pkg.H2AggError) as ei:
        eng.fr_grand_product_device(d.data_ptr(), None, k, u, big, d_out.data_ptr(), None)
    assert ei.value.code == pkg.ERR_NONCANONICAL
    eng.synchronize()                                                               # nothing was queued, nothing to report
    for queue in (lambda: eng.fr_batch_invert_device(d.data_ptr(), 1 << k, d_out.data_ptr()),
                  lambda: eng.fr_grand_product_device(d.data_ptr(), None, k, u, ONE, d_out.data_ptr(), None),
                  lambda: eng.lookup_product_device(d.data_ptr(), d.data_ptr(), d.data_ptr(), d.data_ptr(), k, u, ONE, ONE, d_out.data_ptr(), None)):
        queue()
        with pytest.raises(pkg.H2AggError) as ei:
            eng.synchronize()
        assert ei.value.code == pkg.ERR_NONCANONICAL
        eng.synchronize()                                                           # reported once
    still_works()
