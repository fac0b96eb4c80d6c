"""h2agg_destroy frees everything a context owns, and no list names any of it: every resource has an owner that releases it
with the context (csrc/hip_owners.hpp).  The figures cover the grow-only device buffers (DevBuf), the base tables' columns,
beta * x columns, fixed-base levels and combs and the work memory of the G1 transform and the setup (DevMem); the streams,
the events and the pinned blocks (Stream, Event, PinnedBuf) hold no device memory the figures could show and are covered by the
calls succeeding cycle after cycle.  Three cycles of create / use / close in one process; "use" touches a buffer of each owner
at the smallest shape that allocates it, and a table from each of the five creating paths, some freed by hand and some left
for destroy.  Every result equals what the same call gave in the first cycle, and the device's free memory after the third
close is not below what it was after the second (the first cycle absorbs what the runtime allocates once per process).

Measured at the commit before the owners (written-out lists in h2agg_destroy and Table::release, the refusal paths freeing by
hand), on an MI355X: free memory after the three closes 308017102848, 308017102848, 308017102848 bytes; before and after the
64 refusals 308000325632 and 308000325632 bytes.  Equal figures, so neither test makes an allowance."""
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


def device_bytes(data):
    import torch
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(torch.device("cuda:0"))
    torch.cuda.synchronize()
    return t


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
        # a table from every other creating path; hg and gl are left for destroy, hf and g are freed here
        hg = e.bases_generate(x["d_s16"].data_ptr(), 16)
        hf = e.bases_fft(hg, 3)
        g, gl = e.params_setup(3, x["s4"][:32])
        got += [e.bases_download(hg, 0, 16), e.bases_download(hf, 0, 8), e.bases_download(g, 0, 8), e.bases_download(gl, 0, 8)]
        e.msm_configure_glv(1)
        jac.append(e.g1_msm_preloaded(hg, x["s16"]))    # the table's beta * x column
        e.msm_configure_glv(0)
        e.bases_free(hf)
        e.bases_free(g)
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
    x["d_s16"] = device_bytes(x["s16"])   # (made once: torch keeps its block for all three cycles)
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


REFUSAL_ALLOWANCE = 0   # bytes the free memory may fall over the 64 refused calls
LOG_N = 14              # 2^14 points: 1 MiB per table, so tables left behind by the refusals would be 64 MiB


def test_refusals_after_the_allocation_leave_nothing_behind(pkg):
    """a table is allocated before the device can say that its input is bad: 32 uploads whose last point is no point of the
    curve and 32 generations whose last scalar is r, each followed by a good small call.  (h2agg_bases_upload tests the
    coordinates' range and not the curve equation: the point it refuses is (1, p), H2AGG_ERR_NONCANONICAL; (1, 3) it takes.)"""
    import torch
    x = inputs()
    n = 1 << LOG_N
    g = O.aff_to_bytes(O.G1)
    off_curve = g[:32] + O.P.to_bytes(32, "little")
    good_points, bad_points = g * n, g * (n - 1) + off_curve
    one = O.fe_to_bytes(1)
    d_good, d_bad = device_bytes(one * n), device_bytes(one * (n - 1) + O.R.to_bytes(32, "little"))
    e = pkg.H2Agg(0)
    try:
        small = e.fr_batch_op(pkg.OP_MUL, x["a4"], x["b4"])
        # what a good call of either kind grows in the context (staging, the generator's comb) is there before the first figure
        h = e.bases_upload(good_points)
        want = e.bases_download(h, n - 2, 2)
        e.bases_free(h)
        h = e.bases_generate(d_good.data_ptr(), n)
        assert e.bases_download(h, n - 2, 2) == want == g * 2
        e.bases_free(h)
        before = torch.cuda.mem_get_info()[0]
        for call, code in ((lambda: e.bases_upload(bad_points), pkg.ERR_NONCANONICAL),
                           (lambda: e.bases_generate(d_bad.data_ptr(), n), pkg.ERR_NONCANONICAL)):
            for _ in range(32):
                with pytest.raises(pkg.H2AggError) as ei:
                    call()
                assert ei.value.code == code, ei.value
                assert e.fr_batch_op(pkg.OP_MUL, x["a4"], x["b4"]) == small
        after = torch.cuda.mem_get_info()[0]
        print("free device memory before and after the refusals:", before, after)
        assert after >= before - REFUSAL_ALLOWANCE, (before, after)
    finally:
        e.close()


def test_stream_roles_are_handed_out_twice_and_the_pool_is_released(pkg):
    """create, a caller's stream, a bucket-path MSM, the context's own stream again, close: place_streams permutes the roles
    twice per context before the streams' owners release them; three cycles give the same point and no error"""
    import torch
    x = inputs()
    stream = torch.cuda.Stream()
    first = None
    for cycle in range(3):
        e = pkg.H2Agg(0)
        try:
            e.set_stream(stream.cuda_stream)
            e.debug_configure("comb_msm", 0)
            h = e.bases_upload(x["bases"])
            jac = e.g1_msm_preloaded(h, x["s16"])
            e.set_stream(None)
            got = bytes(e.g1_batch_to_affine(jac))
        finally:
            e.close()
        if first is None:
            first = got
        assert got == first and any(got), "cycle %d" % (cycle + 1)
