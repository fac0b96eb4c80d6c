"""Fr elements as the C ABI takes them: canonical 32-byte little-endian.  Shared by the GPU tests of the Fr prover steps."""
from oracle import bn254 as O

R = O.R


def enc(xs):
    """integers in [0, 2^256) as they are: a value >= R stays non-canonical, nothing is reduced behind the test's back"""
    return b"".join(x.to_bytes(32, "little") for x in xs)


def dec(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def fe(x):
    return (x % R).to_bytes(32, "little")
