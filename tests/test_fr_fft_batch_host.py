"""CPU: poly.columns_* — the slab forms of the four domain conversions — against a stand-in engine that records what it is
handed: one fr_fft_batch call each, the padding of coeff_to_extended, the lengths, and the rejection of a ragged slab."""
import importlib

import pytest

import __graft_entry__ as entry


@pytest.fixture(scope="module")
def poly(pkg):
    return importlib.import_module(entry.PKG_NAME + ".poly")


class Recorder:
    """fr_fft_batch that returns its input with every byte incremented, and keeps its arguments"""

    def __init__(self):
        self.calls = []

    def fr_fft_batch(self, data, k, inverse=False, shift=None):
        self.calls.append((bytes(data), k, bool(inverse), shift))
        return bytes((b + 1) & 0xFF for b in data)

    def fr_fft(self, *a, **kw):
        raise AssertionError("a slab form went through the single transform")


def column(k, tag):
    return bytes((tag + i) & 0xFF for i in range(32 << k))


def bumped(b):
    return bytes((x + 1) & 0xFF for x in b)


def test_one_call_per_conversion_with_the_right_direction_and_shift(poly):
    k, m = 3, 4
    cols = [column(k, 16 * j) for j in range(m)]
    for fn, inverse in ((poly.columns_lagrange_to_coeff, True), (poly.columns_coeff_to_lagrange, False)):
        eng = Recorder()
        out = fn(eng, cols, k)
        assert eng.calls == [(b"".join(cols), k, inverse, None)]
        assert out == [bumped(c) for c in cols]
    eng = Recorder()
    out = poly.columns_extended_to_coeff(eng, cols, k)
    assert eng.calls == [(b"".join(cols), k, True, poly.ZETA)] and out == [bumped(c) for c in cols]
    eng = Recorder()
    poly.columns_extended_to_coeff(eng, cols, k, shift=b"\x05" + bytes(31))
    assert eng.calls[0][3] == b"\x05" + bytes(31)


def test_coeff_to_extended_pads_every_column(poly):
    k, ek, m = 2, 4, 3
    cols = [column(k, 16 * j + 1) for j in range(m)]
    pad = bytes((32 << ek) - (32 << k))
    eng = Recorder()
    out = poly.columns_coeff_to_extended(eng, cols, k, ek)
    assert eng.calls == [(b"".join(c + pad for c in cols), ek, False, poly.ZETA)]
    assert [len(o) for o in out] == [32 << ek] * m
    assert out == [bumped(c + pad) for c in cols]
    eng = Recorder()
    assert poly.columns_coeff_to_extended(eng, cols, k, k) == [bumped(c) for c in cols]     # extended_k == k: no padding
    assert eng.calls[0][0] == b"".join(cols)
    with pytest.raises(ValueError):
        poly.columns_coeff_to_extended(Recorder(), cols, k, k - 1)


def test_what_slab_accepts_is_accepted(poly):
    k = 2
    cols = [column(k, 3), column(k, 40)]
    for given in (cols, tuple(cols), iter(cols), [bytearray(c) for c in cols]):
        eng = Recorder()
        assert poly.columns_coeff_to_lagrange(eng, given, k) == [bumped(c) for c in cols]
        assert eng.calls[0][0] == b"".join(cols)


def test_ragged_and_empty_slabs_are_refused_before_the_engine(poly):
    k = 3
    good = column(k, 0)
    fns = (lambda e, c: poly.columns_lagrange_to_coeff(e, c, k), lambda e, c: poly.columns_coeff_to_lagrange(e, c, k),
           lambda e, c: poly.columns_coeff_to_extended(e, c, k, k + 1), lambda e, c: poly.columns_extended_to_coeff(e, c, k))
    for fn in fns:
        for bad in ([good, good[:-32]], [good + bytes(32), good], [good, None], [], None):
            eng = Recorder()
            with pytest.raises(ValueError):
                fn(eng, bad)
            assert eng.calls == []
