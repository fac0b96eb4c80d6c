"""GPU: MSMs with DIFFERENT plans in flight on the context's tail slots (round-1 advisor finding: the slots' bucket /
segment / window-sum regions were cut out of one allocation at par * (this MSM's size), so a small MSM's accumulation
could write into the region a large MSM's tail was still reading), plus the sticky status word of asynchronous calls.

Every expected value is (sum_{i<n} k_i s_i) * G from the Python oracle."""
import functools

import numpy as np
import pytest
import torch

from oracle import bn254 as O

pytestmark = pytest.mark.gpu


def _workload(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    raw = rng.bytes(64 * n)
    vals = [int.from_bytes(raw[64 * i:64 * i + 64], "little") % O.R for i in range(n)]
    arr = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(n, 32)
    return vals, arr


def _expected(prefix_total):
    return O.aff_to_bytes(O.scalar_mul(prefix_total % O.R, O.G1))


def _rotate(eng, table, d_s, scratch, k):
    """advance the context's tail-slot parity by k (one small MSM each)"""
    for _ in range(k):
        eng.g1_msm_device_async(table, d_s.data_ptr(), 64, scratch.data_ptr())


def test_sliced_device_msm_ragged_last_slice_every_parity(eng):
    """n = 2^22 + r: h2agg_g1_msm_device_async cuts the MSM into 2^22-point slices plus a ragged one; the slices share ONE
    bucket set (msm_run chain modes: c = 16, no GLV, every slice adds to the sums its buckets hold; bucket reduction and Horner
    tail once, behind the last slice), at every parity of the context's tail slots."""
    rs = [1000, 1 << 15, 1 << 19]
    n_max = (1 << 22) + max(rs)
    ks, k_np = _workload(n_max, 101)
    ss, s_np = _workload(n_max, 102)
    dev = torch.device("cuda", 0)
    d_k = torch.from_numpy(k_np.copy()).to(dev)
    d_s = torch.from_numpy(s_np.copy()).to(dev)
    scratch = torch.zeros(96, dtype=torch.uint8, device=dev)
    table = eng.bases_generate(d_k.data_ptr(), n_max)
    del d_k
    try:
        acc, marks = 0, {}
        want_at = sorted((1 << 22) + r for r in rs)
        j = 0
        for i in range(n_max):
            acc += ks[i] * ss[i]
            if i + 1 == want_at[j]:
                marks[want_at[j]] = acc
                j += 1
                if j == len(want_at):
                    break
        for r in rs:
            n = (1 << 22) + r
            want = _expected(marks[n])
            for start in range(3):
                _rotate(eng, table, d_s, scratch, start)
                got = eng.g1_batch_to_affine(eng.g1_msm_device(table, d_s.data_ptr(), n))
                assert got == want, (r, start)
    finally:
        eng.bases_free(table)


@pytest.mark.parametrize("level", [1, 2, 3])
def test_overlap_mode_alternating_sizes(eng, level):
    """public overlap mode, back-to-back asynchronous MSMs of very different sizes (2^20 / 2^10 / 2^14 / 3 points):
    every result must be right, whatever tails were in flight around it."""
    n_max = 1 << 20
    ks, k_np = _workload(n_max, 111)
    ss, s_np = _workload(n_max, 112)
    dev = torch.device("cuda", 0)
    d_k = torch.from_numpy(k_np.copy()).to(dev)
    d_s = torch.from_numpy(s_np.copy()).to(dev)
    table = eng.bases_generate(d_k.data_ptr(), n_max)
    sizes = [1 << 20, 1 << 10, 1 << 20, 1 << 10, 1 << 14, 1 << 20, 3, 1 << 10, 1 << 20, 1 << 14, 1 << 10, 1 << 20, 1 << 10]
    offsets = [0, 5, 0, 77, 1000, 0, 9, 0, 0, 12345, 999, 0, 31]
    d_out = torch.zeros((len(sizes), 96), dtype=torch.uint8, device=dev)
    pre = [0]
    for k, s in zip(ks, ss):
        pre.append(pre[-1] + k * s)
    eng.msm_set_tail_overlap(level)
    try:
        for rep in range(2):
            d_out.zero_()
            torch.cuda.synchronize()
            for i, (n, off) in enumerate(zip(sizes, offsets)):
                # scalars start at `off`: the MSM pairs base j with scalar off + j, so re-derive the expectation below
                eng.g1_msm_device_async(table, d_s.data_ptr() + 32 * off, n, d_out[i].data_ptr())
            eng.synchronize()
            out = bytes(d_out.cpu().numpy().tobytes())
            aff = eng.g1_batch_to_affine(out)
            for i, (n, off) in enumerate(zip(sizes, offsets)):
                if off == 0:
                    tot = pre[n]
                else:
                    tot = sum(ks[j] * ss[off + j] for j in range(n))
                assert aff[64 * i:64 * i + 64] == _expected(tot), (rep, i, n, off)
    finally:
        eng.msm_set_tail_overlap(0)
        eng.bases_free(table)


@functools.lru_cache(maxsize=None)
def _growth_workload():
    """computed once for both levels: (base scalars, MSM scalars, expected points of the first 2^20 and of all the pairs)"""
    n0, n1 = 1 << 20, (1 << 20) + (1 << 18)
    ks, k_np = _workload(n1, 141)
    ss, s_np = _workload(n1, 142)
    t0 = sum(k * s for k, s in zip(ks[:n0], ss[:n0]))
    t1 = t0 + sum(k * s for k, s in zip(ks[n0:], ss[n0:]))
    return k_np, s_np, _expected(t0), _expected(t1)


@pytest.mark.parametrize("level", [2, 3])
def test_deferred_tail_forced_out_by_workspace_growth(pkg, level):
    """A tail that waits for the next MSM (overlap level >= 2, 2^20 points) is launched from INSIDE that MSM's call when the call
    has to replace a workspace buffer: on a fresh context the second MSM (2^20 + 2^18 points) needs more than the first one's
    buffers with their 12.5 % head-room hold, and a grow-only buffer is only replaced behind everything queued or still to be
    queued that may refer to it.  Both results must be right."""
    n0, n1 = 1 << 20, (1 << 20) + (1 << 18)
    k_np, s_np, want0, want1 = _growth_workload()
    dev = torch.device("cuda", 0)
    d_k = torch.from_numpy(k_np.copy()).to(dev)
    d_s = torch.from_numpy(s_np.copy()).to(dev)
    d_out = torch.zeros((2, 96), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    e = pkg.H2Agg(0)
    try:
        table = e.bases_generate(d_k.data_ptr(), n1)
        e.msm_set_tail_overlap(level)
        e.g1_msm_device_async(table, d_s.data_ptr(), n0, d_out[0].data_ptr())
        e.g1_msm_device_async(table, d_s.data_ptr(), n1, d_out[1].data_ptr())
        e.synchronize()
        aff = e.g1_batch_to_affine(bytes(d_out.cpu().numpy().tobytes()))
        assert aff[:64] == want0
        assert aff[64:128] == want1
        e.bases_free(table)
    finally:
        e.close()


def test_host_sliced_msm_with_short_last_slice(eng):
    """h2agg_g1_msm host slicing (>= 2^19-point slices crossing PCIe under the previous slice's compute): a ragged
    total so that the slices differ in size."""
    n = (1 << 20) + (1 << 19) + 12345
    ks, k_np = _workload(n, 121)
    ss, s_np = _workload(n, 122)
    dev = torch.device("cuda", 0)
    d_k = torch.from_numpy(k_np.copy()).to(dev)
    table = eng.bases_generate(d_k.data_ptr(), n)
    try:
        bases = eng.bases_download(table, 0, n)
    finally:
        eng.bases_free(table)
    want = _expected(sum(k * s for k, s in zip(ks, ss)))
    for start in range(3):
        if start:
            eng.g1_msm(bases[:64 * 7], bytes(s_np[:7].tobytes()))     # rotates the slot parity
        assert eng.g1_batch_to_affine(eng.g1_msm(bases, bytes(s_np.tobytes()))) == want, start


def test_async_noncanonical_scalar_is_reported(eng, pkg):
    """A scalar >= r handed to an ASYNCHRONOUS MSM raises FLAG_NONCANONICAL on the device; it must surface from
    h2agg_synchronize (or the next synchronous call) instead of being wiped by that call's own flag reset."""
    n = 256
    ks, k_np = _workload(n, 131)
    ss, s_np = _workload(n, 132)
    bad = s_np.copy()
    bad[17] = np.frombuffer(O.R.to_bytes(32, "little"), dtype=np.uint8)          # == r: not canonical
    dev = torch.device("cuda", 0)
    d_k = torch.from_numpy(k_np.copy()).to(dev)
    d_bad = torch.from_numpy(bad).to(dev)
    d_good = torch.from_numpy(s_np.copy()).to(dev)
    d_out = torch.zeros(96, dtype=torch.uint8, device=dev)
    table = eng.bases_generate(d_k.data_ptr(), n)
    try:
        eng.g1_msm_device_async(table, d_bad.data_ptr(), n, d_out.data_ptr())
        with pytest.raises(pkg.H2AggError) as ei:
            eng.synchronize()
        assert ei.value.code == pkg.ERR_NONCANONICAL
        eng.synchronize()                                                         # reported once, then clean
        # ... and through the NEXT synchronous call when nobody synchronises in between
        eng.g1_msm_device_async(table, d_bad.data_ptr(), n, d_out.data_ptr())
        with pytest.raises(pkg.H2AggError) as ei:
            eng.g1_batch_to_affine_device(d_out.data_ptr(), 1)
        assert ei.value.code == pkg.ERR_NONCANONICAL
        # a clean asynchronous MSM afterwards is clean
        eng.g1_msm_device_async(table, d_good.data_ptr(), n, d_out.data_ptr())
        eng.synchronize()
        got = eng.g1_batch_to_affine_device(d_out.data_ptr(), 1)
        assert got == _expected(sum(k * s for k, s in zip(ks, ss)))
    finally:
        eng.bases_free(table)


def test_mul_with_bare_commitment_on_the_scalar_side(eng, pkg):
    """evaluation.rs:284-288: the commitment-free side of a Mul must evaluate to ONE entry WITH a scalar; a bare
    Commitment there makes the reference `unwrap()` a None.  With another scalar-carrying commitment present the
    multi_exp is not empty, so this must be H2AGG_ERR_INVALID — not a silently wrong point."""
    b = pkg.SchemaBuilder(eng)
    P, Q, Rr = O.scalar_mul(5, O.G1), O.scalar_mul(9, O.G1), O.scalar_mul(11, O.G1)
    cp = pkg.CommitQuery("p", O.aff_to_bytes(P), None)
    cq = pkg.CommitQuery("q", O.aff_to_bytes(Q), None)
    cr = pkg.CommitQuery("r", O.aff_to_bytes(Rr), None)
    three = b.scalar(O.fe_to_bytes(3))
    for s in ((b.commit(cp) * b.commit(cq)) + b.commit(cr) * three,
              three * (b.commit(cp) * b.commit(cq)) + b.commit(cr) * three):
        with pytest.raises(pkg.H2AggError) as ei:
            s.eval()
        assert ei.value.code == pkg.ERR_INVALID
    b.close()


def test_wrapper_length_checks(eng):
    """the ctypes wrappers refuse mismatched buffer lengths instead of letting the C side read past a short buffer"""
    one = O.fe_to_bytes(1)
    with pytest.raises(ValueError):
        eng.fr_batch_op(0, one * 4, one * 3)
    with pytest.raises(ValueError):
        eng.g1_batch_scalar_mul(O.aff_to_bytes(O.G1), one * 2)
    with pytest.raises(ValueError):
        eng.eval_flat(O.aff_to_bytes(O.G1), one, b"\x01\x01")
    with pytest.raises(ValueError):
        eng.fr_sum_with_coeff_and_constant(one * 2, one, one)
