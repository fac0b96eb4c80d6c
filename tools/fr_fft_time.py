#!/usr/bin/env python3
"""Timing of the Fr Fourier transform, device variant (h2agg_fr_fft_device), beside the two bounds it could sit at.

    python tools/fr_fft_time.py [--ks 12,16,20,22,24] > profiles/fr_fft.txt
    python tools/fr_fft_time.py --batch --ks 12,16,20 >> profiles/fr_fft.txt
    rocprofv3 --kernel-trace --stats -- python tools/fr_fft_time.py --only 20      (k_fr_fft_pass's own line; on its own,
                                                                                   no counters in the run)

Method (that of tools/params_time.py, with events instead of the wall clock because the call is asynchronous): the data is
resident, the context runs on a stream of the caller, two events on that stream bracket REPS transforms queued back to back
after two warm-up transforms (which also build the twiddle tables and grow the work array); the figure is the median of
five such brackets divided by REPS.  In place (d_out == d_in): a transform of random data is random data, so repeating
it needs no reset.

--batch: h2agg_fr_fft_batch against the same columns through h2agg_fr_fft, m in {1, 8, 34} columns at k in {12, 16, 20},
forward with shift zeta (a coset's transforms).  The batch has no device-buffer twin yet, so these rows go through the host
entry points, in place on one host buffer, and the two events bracket the staging copies as well as the launches — equally in
every column of the table:
  singles   m calls of h2agg_fr_fft, one column each (m copies in, m sets of launches, m copies out, m synchronisations)
  chunk 1   one h2agg_fr_fft_batch call with the debug key fr_fft_batch_chunk = 1: the slab staged whole, one column per set of
            launches — what of the gain over `singles` is the staging
  batch     one h2agg_fr_fft_batch call: every pass one launch over all columns the work array holds
The resident comparison is the quotient's `forward` phase (tools/quotient_time.py), which runs 34 columns per coset.

Bounds printed beside each time:
  mem    passes x 64 n bytes (every pass reads and writes 32 B per element) at the rate of a device-to-device copy of the
         same 32 n bytes measured in the same run — i.e. passes x the copy's time, not the data sheet's bandwidth;
  valu   Montgomery products x 882 cycles per wave64 product (162 v_mad_u64_u32 + 25 v_lshl_add_u64 +
         16 v_lshrrev_b64 + 9 v_mul_lo_u32 at 4 cycles, 17 v_and at 2) / 64 lanes / 1024 SIMDs at 2.08 GHz (the clock
         section 9 measured under a multiply-add load).  The product count is the kernel's own: conversion in and out,
         shift, every butterfly and inter-pass twiddle whose factor is not 1, one table product per inter-pass twiddle and
         per shifted element (an upper bound: a factor with a zero half needs none).  The additions, the reductions to < 2r
         and the LDS traffic are NOT in it, so the kernel cannot reach this bound; the column says how far the products
         alone would carry.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry

CYCLES_PER_PRODUCT = 882
SIMDS, CLOCK_HZ = 1024, 2.08e9
REPS = 10


def plan(k, local):
    if k == 0:
        return [0]
    p = (k + local - 1) // local
    return [local] * (p - 1) + [k - (p - 1) * local]


def products(k, local, shift):
    n = 1 << k
    widths = plan(k, local)
    total = 2 * n                                    # conversion in, conversion out
    if shift:
        total += 2 * (n - 1)                         # shift^j and its table product
    for q, w in enumerate(widths):
        hb, lb = sum(widths[:q]), sum(widths[q + 1:])
        per_transform = sum((1 << (w - 1)) - (1 << (w - s)) for s in range(1, w + 1))
        total += (n >> w) * per_transform
        if lb:
            total += 2 * (1 << hb) * ((1 << lb) - 1) * ((1 << w) - 1)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="12,16,20,22,24")
    ap.add_argument("--batch", action="store_true", help="h2agg_fr_fft_batch against m single calls (see the header)")
    ap.add_argument("--only", type=int, default=0, help="two warm-up transforms and one bracket at this k, forward, no shift")
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    poly = __import__("importlib").import_module(entry.PKG_NAME + ".poly")
    eng = pkg.H2Agg(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    eng.set_stream(stream.cuda_stream)
    local = pkg.FR_FFT_LOCAL

    def bracket(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            for _ in range(REPS):
                f()
            e1.record(stream)
        eng.synchronize()
        e1.synchronize()
        return e0.elapsed_time(e1) / REPS

    def measure(f):
        f()
        f()
        eng.synchronize()
        return statistics.median(bracket(f) for _ in range(5))

    def resident(k):
        g = torch.Generator(device="cpu").manual_seed(k)
        d = torch.randint(0, 256, ((1 << k), 32), dtype=torch.uint8, generator=g)
        d[:, 31] &= 0x1F                              # every element < 2^253 < r
        d = d.to(dev)
        torch.cuda.synchronize()
        return d

    if a.batch:
        reps = 3
        print("# %s" % eng.describe())
        print("# forward, shift zeta, host entry points in place; %d repetitions per bracket, median of 5 brackets; times in ms" % reps)
        print("#  k    m    singles    chunk 1      batch   singles / batch   chunk 1 / batch")

        def timed(f):
            def one():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(reps):
                    f()
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1) / reps
            f()
            f()
            return statistics.median(one() for _ in range(5))

        for k in [int(x) for x in a.ks.split(",") if x]:
            col = 32 << k
            for m in (1, 8, 34):
                buf = bytearray(resident(k).cpu().numpy().tobytes() * m)
                views = [(C.c_char * col).from_buffer(buf, j * col) for j in range(m)]

                def singles():
                    for v in views:
                        eng._check(eng._lib.h2agg_fr_fft(eng._ctx, C.addressof(v), k, 0, poly.ZETA, C.addressof(v)))

                def batch():
                    eng.fr_fft_batch(buf, k, False, poly.ZETA)

                t_single = timed(singles)
                eng.debug_configure("fr_fft_batch_chunk", 1)
                t_chunk1 = timed(batch)
                eng.debug_configure("fr_fft_batch_chunk", 0)
                t_batch = timed(batch)
                print("%4d  %3d  %9.4f  %9.4f  %9.4f   %15.2f   %15.2f" % (k, m, t_single, t_chunk1, t_batch, t_single / t_batch,
                                                                          t_chunk1 / t_batch))
                sys.stdout.flush()
                del views, buf
        return
    if a.only:
        d = resident(a.only)
        measure(lambda: eng.fr_fft_device(d.data_ptr(), a.only, False, None, d.data_ptr()))
        return
    print("# %s" % eng.describe())
    print("# stages fused per pass: %d; %d transforms per bracket, median of 5 brackets; times in ms" % (local, REPS))
    print("#  k  dir      shift  passes        ms    copy ms    mem bound   products   valu bound")
    for k in [int(x) for x in a.ks.split(",") if x]:
        d = resident(k)
        e = torch.empty_like(d)

        def copy():
            with torch.cuda.stream(stream):
                e.copy_(d)
        t_copy = measure(copy)
        for inverse in (False, True):
            for shift in (None, poly.ZETA):
                t = measure(lambda: eng.fr_fft_device(d.data_ptr(), k, inverse, shift, d.data_ptr()))
                np_ = products(k, local, shift is not None)
                valu = np_ / 64.0 * CYCLES_PER_PRODUCT / SIMDS / CLOCK_HZ * 1e3
                passes = len(plan(k, local))
                print("%4d  %-7s  %-5s  %6d  %8.4f   %8.4f     %8.4f  %9d     %8.4f" % (
                    k, "inverse" if inverse else "forward", "zeta" if shift else "none", passes, t, t_copy, passes * t_copy, np_, valu))
                sys.stdout.flush()
        del d, e
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
