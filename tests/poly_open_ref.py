"""The yardstick of the KZG opening tests in Python integers (no device, no library): the definitions of include/h2agg.h,
a(z) = sum_i a[i] z^i and q[j] = sum_{i>j} a[i] z^(i-j-1), rem = a(z).  tests/test_poly_open_host.py ties the recurrence to
the sum as written; tests/test_gpu_poly_open.py compares the device with it byte for byte."""
import random

from oracle import bn254 as O

R = O.R
BIG_Z = random.Random(0x0BE2).randrange(1 << 253, R)   # a 254-bit value


def horner(a, z):
    v = 0
    for c in reversed(a):
        v = (v * z + c) % R
    return v


def quotient_definition(a, z):
    n = len(a)
    return [sum(a[i] * pow(z, i - j - 1, R) for i in range(j + 1, n)) % R for j in range(n)]


def quotient_py(a, z):
    n = len(a)
    q = [0] * n
    for j in range(n - 1, 0, -1):
        q[j - 1] = (a[j] + z * q[j]) % R
    return q


def assert_division(a, z, q, rem):
    """q(X) (X - z) + rem == a(X) on integers mod r, the zero on top, rem = a(z)"""
    n = len(a)
    assert len(q) == n and q[n - 1] == 0
    assert rem == horner(a, z)
    assert (rem - z * q[0]) % R == a[0]
    for j in range(1, n):
        assert (q[j - 1] - z * q[j]) % R == a[j], j


def random_input(seed, k):
    """random canonical elements; 0, 1 and r - 1 among them where there is room"""
    rng = random.Random(seed)
    a = [rng.randrange(R) for _ in range(1 << k)]
    for pos, v in zip(rng.sample(range(1 << k), min(3, 1 << k)), (R - 1, 0, 1)):
        a[pos] = v
    return a
