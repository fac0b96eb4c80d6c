"""The batched lookup entry points of include/h2agg.h restated with Python integers: lookup j of a batch is lookup_permute_py
(tests/lookup_permute_ref.py) / lookup_product_py (tests/grand_product_ref.py) on column j, with a status word per lookup, and
the rule that cuts a batch into chunks (csrc/lookup.inc lk_batch_chunk).  tests/test_lookup_batch_host.py ties the
restatement to the verifier's conditions; tests/test_gpu_lookup_batch.py compares the library with it byte for byte."""
from tests.grand_product_ref import R, lookup_product_py
from tests.lookup_permute_ref import NotInTable, lookup_permute_py

FLAG_NONCANONICAL, FLAG_NOT_IN_TABLE = 1, 8               # the library's status bits (batch_kernels.hpp, lookup_kernels.hpp)
BATCH_ROWS, BATCH_MAX, MAX_LOOKUPS = 1 << 24, 1024, 65535


def batch_chunk(u, forced=0):
    """lookups per set of launches: clamp(2^24 / max(u, 1), 1, 1024), fewer where lookup_configure asks for fewer"""
    b = min(max(BATCH_ROWS // max(u, 1), 1), BATCH_MAX)
    return forced if forced and forced < b else b


def chunk_split(count, u, forced=0):
    """-> [(first lookup, lookups)] of the chunks of a batch"""
    b = batch_chunk(u, forced)
    return [(j, min(b, count - j)) for j in range(0, count, b)]


def status_py(a, s, u):
    """the status word of one lookup: an element >= r among the usable rows, a head value absent from the usable table rows"""
    word = FLAG_NONCANONICAL if any(x >= R for x in a[:u] + s[:u]) else 0
    if set(a[:u]) - set(s[:u]):
        word |= FLAG_NOT_IN_TABLE
    return word


def batch_permute_py(a_cols, s_cols, u):
    """-> (ap columns, sp columns, status words); the pair of a failed lookup is None (unspecified)"""
    aps, sps, status = [], [], []
    for a, s in zip(a_cols, s_cols):
        word = status_py(a, s, u)
        status.append(word)
        if word:
            aps.append(None)
            sps.append(None)
            continue
        ap, sp = lookup_permute_py(a, s, u)
        aps.append(ap)
        sps.append(sp)
    return aps, sps, status


def first_failure(status):
    """the status word the call's return code comes from: the lowest-numbered failing lookup's (0: none failed)"""
    return next((w for w in status if w), 0)


def batch_product_py(a_cols, s_cols, ap_cols, sp_cols, u, beta, gamma):
    """-> (z[j][0 .. u], last[j])"""
    zs = [lookup_product_py(a, s, ap, sp, u, beta, gamma) for a, s, ap, sp in zip(a_cols, s_cols, ap_cols, sp_cols)]
    return zs, [z[u] for z in zs]


__all__ = ["NotInTable", "batch_chunk", "chunk_split", "status_py", "batch_permute_py", "first_failure", "batch_product_py"]
