"""h2agg_destroy frees everything a context owns: its grow-only buffers free themselves with the context (no list names them),
its base tables through Table::release.  Three cycles of create / use / close in one process; "use" touches a buffer of each
owner at the smallest shape that allocates it.  Every result equals what the same call gave in the first cycle, and the
device's free memory after the third close is not below what it was after the second (the first cycle absorbs what the runtime
allocates once per process).

Measured at the commit before the buffers freed themselves (a written-out list in h2agg_destroy): the figures after the second
and third close were equal, so no allowance is made."""
import pytest

from oracle import bn254 as O

pytestmark = pytest.mark.gpu

ALLOWANCE = 0   # bytes the free memory may fall between the second and third close


def inputs():
    rng = O.SplitMix64(0x4C494645)
    fr = lambda n: b"".join(O.fe_to_bytes(rng.fr() or 1) for _ in range(n))
    pts = [O.scalar_mul(k, O.G1) for k in range(1, 17)]
    return {
        "a4": fr(4), "b4": fr(4), "s4": fr(4), "s16": fr(16), "f8": fr(8), "v8": fr(8),
        "bases": b"".join(O.aff_to_bytes(p) for p in pts),
        "jac2": b"".join(O.jac_to_bytes(p) for p in pts[:2]),
        "jac2b": b"".join(O.jac_to_bytes(p) for p in pts[2:4]),
    }


def use(pkg, x):
    """one context's life; returns what its calls gave"""
    e = pkg.H2Agg(0)
    try:
        got = [e.fr_batch_op(pkg.OP_MUL, x["a4"], x["b4"])]
        jac = [e.g1_batch_add(x["jac2"], x["jac2b"])]
        h = e.bases_upload(x["bases"])
        e.bases_precompute(h, 8)
        jac.append(e.g1_msm_preloaded(h, x["s4"]))      # the table's comb
        e.debug_configure("comb_msm", 0)
        jac.append(e.g1_msm_preloaded(h, x["s16"]))     # the bucket path and its tail slot
        e.bases_free(h)
        e.bases_upload(x["bases"])                      # one table left for destroy to free
        got.append(e.fr_fft(x["f8"], 3))
        got.append(e.fr_batch_invert(x["v8"]))
        # (a point has many Jacobian forms, and which one the bucket path gives is not fixed: the values compared are affine)
        got.append(e.g1_batch_to_affine(b"".join(bytes(j) for j in jac)))
        return [bytes(g) for g in got]
    finally:
        e.close()


def test_three_contexts_in_a_row_leave_no_memory_behind(pkg):
    import torch
    x = inputs()
    torch.cuda.mem_get_info()
    free, first = [], None
    for cycle in range(3):
        got = use(pkg, x)
        free.append(torch.cuda.mem_get_info()[0])
        if first is None:
            first = got
        assert got == first, "cycle %d" % (cycle + 1)
    print("free device memory after each close:", free)
    assert free[2] >= free[1] - ALLOWANCE, free
