"""The proving key as a device object (include/h2agg.h "Proving key on the device"), without a device: the names of every
layer, the two memory sums restated with Python integers, and that the C++ class compiles.  A verifying key needs a context, so
— as in tests/test_quotient_split_host.py — the one test that holds the sums against the binding is marked gpu."""
import importlib
import os
import random
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as entry
from tests import quotient_ref as Q

MAX_K = 24                 # FFT_MAX_K: the largest single transform
BATCH_WORK_LOG = 23        # FR_FFT_BATCH_WORK_LOG: the most elements a batched transform's work array is sized for


@pytest.fixture(scope="module")
def poly(pkg):
    return importlib.import_module(entry.PKG_NAME + ".poly")


def declared(header_path):
    src = re.sub(r"/\*.*?\*/", "", open(header_path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(h2agg_pk_[a-z0-9_]+)\s*\(", src)))


def test_every_layer_names_the_entry_points(pkg, poly):
    names = declared(pkg.HEADER_PATH)
    assert names == sorted("h2agg_pk_" + s for s in ("create", "create_resident", "bytes", "info", "ptr", "quotient",
                                                      "quotient_work_bytes", "destroy"))
    assert not [n for n in names if re.fullmatch(r"h2agg_\w*(_device|_async)\w*", n)]
    protos = set(pkg.exported_symbols())
    for n in names:
        assert n in protos, n
        assert callable(getattr(pkg.H2Agg, n[len("h2agg_"):])), n
    for method in ("from_lagrange", "from_views", "close", "ptr", "quotient_pieces", "resident_quotient"):
        assert callable(getattr(poly.ProvingKey, method)), method
    assert callable(poly.pk_bytes)
    assert (pkg.PK_FIXED_LAGRANGE, pkg.PK_SIGMA_LAGRANGE, pkg.PK_FIXED_COEFF, pkg.PK_SIGMA_COEFF, pkg.PK_LAGRANGE_COEFF,
            pkg.PK_COSET, pkg.PK_COSETS) == (0, 1, 2, 3, 4, 5, 1)
    header = open(pkg.HEADER_PATH).read()
    for name, value in (("COSETS", "1u"), ("FIXED_LAGRANGE", "0"), ("SIGMA_LAGRANGE", "1"), ("FIXED_COEFF", "2"),
                        ("SIGMA_COEFF", "3"), ("LAGRANGE_COEFF", "4"), ("COSET", "5")):
        assert re.search(r"#define H2AGG_PK_%s %s\b" % (name, value), header), name


# ---------------------------------------------------------------------------------------------- the two sums
def pk_bytes(k, e, F, P, cosets):
    """32 (2 (F + P) n + 3 n + [COSETS] (F + P + 3) n 2^e)"""
    n = 1 << k
    return 32 * (2 * (F + P) * n + 3 * n + ((F + P + 3) * n << e if cosets else 0))


def batch_work(m, k):
    """h2agg_fr_fft_batch's work array for m columns of 2^k, in elements: the whole batch up to 2^23, one column at least"""
    return max(1 << k, min(m << k, 1 << BATCH_WORK_LOG))


def pk_quotient_work_bytes(k, degree, A, F, I, P, L, cosets):
    n, e = 1 << k, Q.extended_k(k, degree)
    sets = -(-P // (degree - 2))
    witness = A + I + sets + 3 * L
    largest = n if k + e > MAX_K else n << e
    if cosets:      # the witness slab, the fold column, a lookup's two theta-folds, ext / u; the witness transforms' work
        return 32 * ((witness + 3) * n + (n << e) + max(largest, batch_work(witness, k)))
    inputs = witness + F + P   # today's layout less the three coefficient columns: (inputs + 6) n, transforms of inputs + 3
    return 32 * ((inputs + 6) * n + (n << e) + max(largest, batch_work(inputs + 3, k)))


def quotient_work_bytes(k, degree, A, F, I, P, L):
    """h2agg_quotient_work_bytes (tests/test_quotient_split_host.py)"""
    n, e = 1 << k, Q.extended_k(k, degree)
    inputs = A + F + I + P + -(-P // (degree - 2)) + 3 * L
    largest = n if k + e > MAX_K else n << e
    return 32 * ((inputs + 9) * n + (n << e) + max(largest, batch_work(inputs + 3, k)))


def test_the_sums_at_the_sizes_the_documents_name():
    gib = 1 << 30
    assert pk_bytes(24, 2, 4, 8, False) == 12 * gib + 3 * gib // 2
    assert pk_bytes(24, 2, 4, 8, True) - pk_bytes(24, 2, 4, 8, False) == 30 * gib
    # the measured shape (tools/pk_time.py): 8 advice, 4 fixed, 1 instance, 8 permutation columns, 2 lookups, degree 4
    for k in (16, 18, 20):
        with_key = pk_quotient_work_bytes(k, 4, 8, 4, 1, 8, 2, True)
        assert with_key < pk_quotient_work_bytes(k, 4, 8, 4, 1, 8, 2, False) < quotient_work_bytes(k, 4, 8, 4, 1, 8, 2)
        assert with_key == 32 * ((19 + 3 + 4) << k) + 32 * max(4 << k, min(19 << k, 1 << 23))


def test_cpp_proving_key_compiles(tmp_path):
    src = tmp_path / "pk.cpp"
    src.write_text('#include "h2agg_chips.hpp"\n'
                   "static_assert(sizeof(h2agg_chips::ProvingKey) > 0, \"the class\");\n"
                   "void (h2agg_chips::ProvingKey::*quotient_of_the_key)(const void*, const void*, const void*, const void*, const void*, "
                   "const void*, const uint8_t*, const h2agg_chips::Scalar&, const h2agg_chips::Scalar&, const h2agg_chips::Scalar&, "
                   "const h2agg_chips::Scalar&, const h2agg_chips::Scalar&, void*) const = &h2agg_chips::ProvingKey::quotient;\n")
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(entry.ROOT, "include"), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---------------------------------------------------------------------------------------------- the binding
@pytest.mark.gpu
@pytest.mark.parametrize("k,degree", [(4, 3), (6, 4), (9, 6)])
def test_the_sums_through_the_binding(pkg, eng, poly, k, degree):
    verifier = importlib.import_module(entry.PKG_NAME + ".verifier")
    from oracle import bn254 as O
    from tests.fr_bytes import enc
    rng = random.Random(0xF90 + k)
    n_perm, n_lookups = 5, 2
    cs = Q.random_shape(rng, k, degree, n_perm, n_lookups, True)
    vk = verifier.VerifyingKey(eng, verifier.encode_vk(cs, O.aff_to_bytes))
    e = Q.extended_k(k, degree)
    column = lambda: enc([rng.randrange(Q.R) for _ in range(cs.n)])
    for cosets in (True, False):
        assert poly.pk_bytes(eng, vk, cosets) == pk_bytes(k, e, 2, n_perm, cosets)
        with poly.ProvingKey.from_lagrange(eng, vk, [column() for _ in range(2)], [column() for _ in range(n_perm)], cosets) as key:
            assert key.info["bytes"] == pk_bytes(k, e, 2, n_perm, cosets) and key.info["e"] == e
            assert key.work_bytes() == pk_quotient_work_bytes(k, degree, 3, 2, 1, n_perm, n_lookups, cosets)
            assert key.work_bytes() < eng.quotient_work_bytes(vk) == quotient_work_bytes(k, degree, 3, 2, 1, n_perm, n_lookups)
    vk.close()


@pytest.mark.gpu
def test_pk_bytes_refuses_what_quotient_work_bytes_refuses(pkg, eng):
    verifier = importlib.import_module(entry.PKG_NAME + ".verifier")
    from oracle import bn254 as O
    rng = random.Random(0xF91)
    for k, degree, refused in ((24, 34, True), (23, 66, True), (25, 3, True), (24, 9, False), (10, 3, False)):
        vk = verifier.VerifyingKey(eng, verifier.encode_vk(Q.random_shape(rng, k, degree, 0, 0, True), O.aff_to_bytes))
        for fn in (eng.quotient_work_bytes, lambda v: eng.pk_bytes(v, 0), lambda v: eng.pk_bytes(v, pkg.PK_COSETS)):
            if refused:
                with pytest.raises(pkg.H2AggError) as ei:
                    fn(vk)
                assert ei.value.code == pkg.ERR_INVALID
            else:
                assert fn(vk) > 0
        with pytest.raises(pkg.H2AggError) as ei:
            eng.pk_bytes(vk, 2)
        assert ei.value.code == pkg.ERR_INVALID
        vk.close()
