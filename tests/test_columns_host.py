"""CPU: the Fr column stores' binding — every h2agg_columns_* declaration of include/h2agg.h has a ctypes signature and a method
on the engine class, none of the names claims the _device / _async suffixes (those mean caller-owned device buffers:
tests/test_stream_probe_host.py holds their set fixed), and the range and overlap arithmetic of poly.ColumnStore.view is
what it is worked out to be by hand."""
import importlib
import re

import pytest

import __graft_entry__ as entry

EXPECTED = ["create", "destroy", "info", "write", "read", "ptr", "move", "fft", "commit", "sigmas", "witness_check", "shplonk_begin"]


def declared(pkg):
    text = re.sub(r"/\*.*?\*/", " ", open(pkg.HEADER_PATH).read(), flags=re.S)
    return re.findall(r"\bint\s+(h2agg_columns_\w+)\s*\(", text)


@pytest.fixture(scope="module")
def poly(pkg):
    return importlib.import_module(entry.PKG_NAME + ".poly")


def test_the_header_declares_the_store_calls_and_the_resident_forms(pkg):
    assert sorted(declared(pkg)) == sorted("h2agg_columns_" + n for n in EXPECTED)


def test_every_declaration_has_a_signature_and_a_method(pkg):
    names = declared(pkg)
    assert names
    symbols = set(pkg.exported_symbols())
    lib = pkg.load_library()
    for name in names:
        assert name in symbols, name
        fn = getattr(lib, name)
        assert fn.argtypes and fn.restype is not None, name
        assert callable(getattr(pkg.H2Agg, name[len("h2agg_"):], None)), name


def test_no_new_name_claims_the_device_buffer_suffixes(pkg):
    names = declared(pkg)
    assert names
    for name in names:
        assert not re.search(r"_device|_async", name), name


class _Store:
    """what ColumnView reads of a store"""

    def __init__(self, handle, m, k):
        self.handle, self.m, self.k = handle, m, k


def test_view_ranges(poly):
    st = poly.ColumnStore(None, 6, 3, handle=9)          # wraps a handle: no engine call
    assert (st.m, st.k, st.handle, st.owned) == (6, 3, 9, False)
    whole = st.view()
    assert (whole.first, whole.count, whole.k, whole.handle) == (0, 6, 3, 9)
    assert (st.view(2).first, st.view(2).count) == (2, 4)
    v = st.view(1, 4)                                    # columns 1 2 3 4
    assert (v.first, v.count) == (1, 4)
    w = v.view(1, 2)                                     # columns 2 3 of the store
    assert (w.first, w.count) == (2, 2)
    assert (v.view(3, 1).first, st.view(5, 1).first) == (4, 5)
    for first, count in ((0, 7), (6, 1), (5, 2), (-1, 2), (0, 0), (3, -1)):
        with pytest.raises(ValueError):
            st.view(first, count)
    for first, count in ((0, 5), (4, 1), (3, 2), (-1, 1), (1, 0)):
        with pytest.raises(ValueError):
            v.view(first, count)
    st.close()                                           # not owned: nothing to call
    assert st.handle == 0


def test_view_overlaps(poly):
    a, b = _Store(4, 8, 2), _Store(5, 8, 2)
    V = poly.ColumnView
    assert V(a, 0, 3).overlaps(V(a, 2, 2))               # column 2 in common
    assert not V(a, 0, 2).overlaps(V(a, 2, 2))           # 0 1 | 2 3: adjacent
    assert not V(a, 2, 2).overlaps(V(a, 0, 2))
    assert V(a, 1, 5).overlaps(V(a, 3, 1)) and V(a, 3, 1).overlaps(V(a, 1, 5))   # inside
    assert V(a, 7, 1).overlaps(V(a, 0, 8))
    assert not V(a, 0, 8).overlaps(V(b, 0, 8))           # another store
    assert V(a, 2, 3).same(V(a, 2, 3)) and not V(a, 2, 3).same(V(a, 2, 2)) and not V(a, 2, 3).same(V(b, 2, 3))
    with pytest.raises(ValueError):
        V(a, 6, 3)
