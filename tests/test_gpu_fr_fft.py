"""GPU: the Fourier transform over Fr — h2agg_fr_fft / h2agg_fr_fft_device (best_fft, coset domains) and poly.py over them.

halo2_proofs is not vendored in the reference, so the yardstick is the definition in include/h2agg.h, evaluated here with
Python integers:  forward out[i] = sum_j (shift^j in[j]) w^(ij);  inverse out[j] = shift^-j / n * sum_i in[i] w^(-ij);
n = 2^k, w = FR_ROOT_OF_UNITY^(2^(28-k)), natural order.  dft_definition is that sum as written (O(n^2)); ntt_py is an
iterative radix-2 transform which the first test ties to dft_definition and the later tests trust.  Results are exact and
compared byte for byte."""
import importlib
import random

import pytest

import __graft_entry__ as entry
from oracle import bn254 as O
from oracle import verifier as V
from tests.fr_bytes import dec, enc

pytestmark = pytest.mark.gpu

R = O.R


@pytest.fixture(scope="module")
def poly(pkg):
    return importlib.import_module(entry.PKG_NAME + ".poly")


def dft_definition(a, k, inverse, shift):
    n = 1 << k
    w = V.omega_for_k(k) if k else 1
    if not inverse:
        return [sum(pow(shift, j, R) * a[j] * pow(w, i * j, R) for j in range(n)) % R for i in range(n)]
    wi, si, ni = O.inv(w, R), O.inv(shift, R), O.inv(n, R)
    return [pow(si, j, R) * ni * sum(a[i] * pow(wi, i * j, R) for i in range(n)) % R for j in range(n)]


def ntt_py(a, k, inverse=False, shift=1):
    n = 1 << k
    w = V.omega_for_k(k) if k else 1
    a = list(a)
    if inverse:
        w = O.inv(w, R)
    elif shift != 1:
        f = 1
        for j in range(n):
            a[j] = a[j] * f % R
            f = f * shift % R
    for i in range(n):                                   # bit reversal, then decimation in time
        j = int(format(i, "0%db" % k)[::-1], 2) if k else 0
        if i < j:
            a[i], a[j] = a[j], a[i]
    for s in range(1, k + 1):
        half = 1 << (s - 1)
        ws = pow(w, 1 << (k - s), R)
        tw = [1] * half
        for t in range(1, half):
            tw[t] = tw[t - 1] * ws % R
        for base in range(0, n, 2 * half):
            for t in range(half):
                x, y = a[base + t], a[base + t + half] * tw[t] % R
                a[base + t], a[base + t + half] = (x + y) % R, (x - y) % R
    if inverse:
        f, si = O.inv(n, R), O.inv(shift, R)
        for j in range(n):
            a[j] = a[j] * f % R
            f = f * si % R
    return a


def random_input(seed, k):
    """random canonical elements; 0, 1 and r - 1 among them where there is room"""
    rng = random.Random(seed)
    a = [rng.randrange(R) for _ in range(1 << k)]
    for pos, v in zip(rng.sample(range(1 << k), min(3, 1 << k)), (R - 1, 0, 1)):
        a[pos] = v
    return a


BIG_SHIFT = random.Random(0xF47).randrange(1 << 253, R)   # a 254-bit value


def shifts(poly):
    return [None, poly.ZETA_INT, BIG_SHIFT]


def run(eng, a, k, inverse, shift):
    return dec(eng.fr_fft(enc(a), k, inverse, None if shift is None else shift.to_bytes(32, "little")))


def test_ntt_py_is_the_definition(poly):
    for k in range(0, 7):
        a = random_input(100 + k, k)
        for inverse in (False, True):
            for sh in (1, poly.ZETA_INT, BIG_SHIFT):
                assert ntt_py(a, k, inverse, sh) == dft_definition(a, k, inverse, sh), (k, inverse, sh)


def test_zeta_is_the_glv_eigenvalue(poly):
    assert pow(poly.ZETA_INT, 3, R) == 1 and poly.ZETA_INT != 1
    assert dec(poly.ZETA) == [poly.ZETA_INT]


@pytest.mark.parametrize("k", range(0, 13))
def test_against_the_definition_default_plan(eng, poly, k):
    a = random_input(200 + k, k)
    for inverse in (False, True):
        for sh in shifts(poly):
            assert run(eng, a, k, inverse, sh) == ntt_py(a, k, inverse, 1 if sh is None else sh), (k, inverse, sh)


@pytest.mark.parametrize("local,k", [(1, 1), (1, 2), (1, 3), (1, 4),
                                     (2, 1), (2, 2), (2, 3), (2, 4), (2, 5), (2, 7),
                                     (3, 3), (3, 4), (3, 6), (3, 7), (3, 9), (3, 10)])
def test_every_pass_boundary_at_the_smallest_size(eng, local, k):
    a = random_input(300 + 16 * local + k, k)
    try:
        eng.debug_configure("fr_fft_local", local)
        for inverse in (False, True):
            assert run(eng, a, k, inverse, BIG_SHIFT) == ntt_py(a, k, inverse, BIG_SHIFT), (local, k, inverse)
    finally:
        eng.debug_configure("fr_fft_local", 0)


def default_plan_ks(pkg):
    D = pkg.FR_FFT_LOCAL
    return sorted({min(x, 21) for x in (D - 1, D, D + 1, 2 * D, 2 * D + 1)})


def test_default_fused_stage_count_is_exported(pkg):
    assert pkg.FR_FFT_LOCAL == 10 and default_plan_ks(pkg) == [9, 10, 11, 20, 21]


@pytest.mark.parametrize("k", [9, 10, 11, 20, 21])
def test_default_plan_boundaries_geometric_input(eng, pkg, k):
    """in[j] = c^j  ->  out[i] = sum_j (c w^i)^j = (c^n - 1) / (c w^i - 1), every i; one batch inversion"""
    assert k in default_plan_ks(pkg)
    n = 1 << k
    c = 0x1234567890ABCDEF0FEDCBA987654321 + k
    cn = pow(c, n, R)
    assert cn != 1
    a, den, x, cw, w = [0] * n, [0] * n, 1, c, V.omega_for_k(k)
    for j in range(n):
        a[j] = x
        x = x * c % R
        den[j] = (cw - 1) % R
        cw = cw * w % R
    pre, acc = [0] * n, 1
    for i in range(n):
        pre[i] = acc
        acc = acc * den[i] % R
    inv = O.inv(acc, R) * (cn - 1) % R
    want = [0] * n
    for i in range(n - 1, -1, -1):
        want[i] = inv * pre[i] % R
        inv = inv * den[i] % R
    got = eng.fr_fft(enc(a), k)
    assert got == enc(want)


@pytest.mark.parametrize("k", [9, 10, 11, 20, 21])
def test_default_plan_boundaries_round_trip(eng, pkg, poly, k):
    assert k in default_plan_ks(pkg)
    n = 1 << k
    buf = bytearray(random.Random(400 + k).randbytes(32 * n))
    buf[31::32] = bytes(b & 0x1F for b in buf[31::32])      # every element < 2^253 < r
    for pos, v in ((0, 0), (n // 2 + 1, 1), (n - 1, R - 1)):
        buf[32 * pos:32 * pos + 32] = v.to_bytes(32, "little")
    data = bytes(buf)
    for sh in (None, poly.ZETA, BIG_SHIFT.to_bytes(32, "little")):
        mid = eng.fr_fft(data, k, False, sh)
        assert mid != data
        assert eng.fr_fft(mid, k, True, sh) == data, (k, sh)


@pytest.mark.parametrize("k", [3, 7])
def test_structured_inputs(eng, poly, k):
    n = 1 << k
    w = V.omega_for_k(k)
    for sh in shifts(poly):
        s = 1 if sh is None else sh
        assert run(eng, [0] * n, k, False, sh) == [0] * n
        assert run(eng, [0] * n, k, True, sh) == [0] * n
        for p in (0, 1, n - 1):
            delta = [0] * n
            delta[p] = 1
            assert run(eng, delta, k, False, sh) == [pow(s, p, R) * pow(w, i * p, R) % R for i in range(n)], (k, p, sh)
            assert run(eng, delta, k, True, sh) == ntt_py(delta, k, True, s)
        for a in ([5] * n, [1 if j % 2 == 0 else R - 1 for j in range(n)]):
            for inverse in (False, True):
                assert run(eng, a, k, inverse, sh) == ntt_py(a, k, inverse, s), (k, inverse, sh)
    assert run(eng, [5] * n, k, False, None) == [5 * n % R] + [0] * (n - 1)
    assert run(eng, [1 if j % 2 == 0 else R - 1 for j in range(n)], k, False, None) == [n if i == n // 2 else 0 for i in range(n)]


def test_in_place_and_device_resident(eng, poly):
    import torch
    k, dev = 9, torch.device("cuda:0")
    data = enc(random_input(500, k))
    sh = BIG_SHIFT.to_bytes(32, "little")
    want = eng.fr_fft(data, k, False, sh)
    assert want == enc(ntt_py(dec(data), k, False, BIG_SHIFT))
    buf = bytearray(data)
    assert eng.fr_fft(buf, k, False, sh) is buf and bytes(buf) == want          # host, out is in
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    d_io = d_in.clone()
    d_out = torch.zeros_like(d_in)
    d_back = torch.zeros_like(d_in)
    torch.cuda.synchronize()
    eng.fr_fft_device(d_in.data_ptr(), k, False, sh, d_out.data_ptr())          # distinct buffers
    eng.fr_fft_device(d_io.data_ptr(), k, False, sh, d_io.data_ptr())           # in place, queued behind it
    eng.fr_fft_device(d_out.data_ptr(), k, True, sh, d_back.data_ptr())         # and the way back, another shift table
    eng.synchronize()
    assert bytes(d_out.cpu().numpy()) == want
    assert bytes(d_io.cpu().numpy()) == want
    assert bytes(d_back.cpu().numpy()) == data
    assert bytes(d_in.cpu().numpy()) == data, "the device variant changed its input"


def test_refusals_leave_the_context_usable(eng, pkg):
    import torch
    good = random_input(600, 4)
    good_out = ntt_py(good, 4, False, BIG_SHIFT)

    def still_works():
        assert run(eng, good, 4, False, BIG_SHIFT) == good_out

    with pytest.raises(pkg.H2AggError) as ei:
        eng.fr_fft(bytes(32), 25)
    assert ei.value.code == pkg.ERR_INVALID
    still_works()
    with pytest.raises(pkg.H2AggError) as ei:
        eng.fr_fft(enc(good), 4, False, bytes(32))
    assert ei.value.code == pkg.ERR_INVALID
    still_works()
    with pytest.raises(pkg.H2AggError) as ei:
        eng.fr_fft(enc(good), 4, True, R.to_bytes(32, "little"))
    assert ei.value.code == pkg.ERR_NONCANONICAL
    still_works()
    bad = random_input(601, 5)
    bad[13] = R
    with pytest.raises(pkg.H2AggError) as ei:
        eng.fr_fft(enc(bad), 5)
    assert ei.value.code == pkg.ERR_NONCANONICAL
    still_works()
    d = torch.frombuffer(bytearray(enc(bad)), dtype=torch.uint8).to(torch.device("cuda:0"))
    d_out = torch.zeros_like(d)
    torch.cuda.synchronize()
    for args in ((25, False, None), (5, False, bytes(32)), (5, True, R.to_bytes(32, "little"))):
        with pytest.raises(pkg.H2AggError):
            eng.fr_fft_device(d.data_ptr(), args[0], args[1], args[2], d_out.data_ptr())
    eng.synchronize()                                                           # nothing was queued, nothing to report
    eng.fr_fft_device(d.data_ptr(), 5, False, None, d_out.data_ptr())           # queues; the element >= r is seen on the device
    with pytest.raises(pkg.H2AggError) as ei:
        eng.synchronize()
    assert ei.value.code == pkg.ERR_NONCANONICAL
    eng.synchronize()                                                           # reported once
    still_works()


@pytest.mark.parametrize("k", [4, 8])
def test_commitments_agree_through_the_transform(eng, poly, k):
    """commit(g, coeffs) == commit(g_lagrange, evals) == p(s) * G"""
    n = 1 << k
    s = random.Random(700 + k).randrange(2, R)
    a = random_input(710 + k, k)
    g, gl = eng.params_setup(k, s.to_bytes(32, "little"))
    try:
        evals = poly.coeff_to_lagrange(eng, enc(a), k)
        assert evals == enc(ntt_py(a, k))
        assert poly.lagrange_to_coeff(eng, evals, k) == enc(a)
        c1 = eng.g1_batch_to_affine(poly.commit_coeff(eng, g, enc(a)))
        c2 = eng.g1_batch_to_affine(poly.commit_lagrange(eng, gl, evals))
    finally:
        eng.bases_free(g)
        eng.bases_free(gl)
    ps = 0
    for c in reversed(a):
        ps = (ps * s + c) % R
    assert c1 == c2 == O.aff_to_bytes(O.scalar_mul(ps, O.G1))


def test_poly_extended_domain(eng, poly):
    k, ek = 5, 7
    a = random_input(800, k)
    ext = poly.coeff_to_extended(eng, enc(a), k, ek)
    assert poly.extended_to_coeff(eng, ext, ek) == enc(a + [0] * ((1 << ek) - (1 << k)))
    w = V.omega_for_k(ek)
    got = dec(ext)
    for i in (0, 1, 2, 31, 32, 77, 126, 127):
        x, v = poly.ZETA_INT * pow(w, i, R) % R, 0
        for c in reversed(a):
            v = (v * x + c) % R
        assert got[i] == v, i
