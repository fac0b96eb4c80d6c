#!/usr/bin/env python3
"""Timing of h2agg_lookup_permute_device beside the bounds it could sit at and the only route that existed before it.

    python tools/lookup_permute_time.py [--ks 16,20,22,24] [--host-ks 16,20,22,24] > profiles/lookup_permute.txt

Method (that of tools/grand_product_time.py).  The columns are resident and the context runs on a stream of the caller;
every call is the asynchronous device variant: two events on the stream bracket REPS calls queued back to back after two
warm-up calls (which also grow the work memory); median of five brackets / REPS.  u = 2^k - 6.  Two inputs, the input
column drawn from the table's usable rows in both:
  random   254-bit table values (top byte 0x20 .. 0x2f): all 32 byte passes of both sorts move
  16-bit   table values below 2^16: two passes of each sort move, thirty are skipped on the device

Beside each time:
  copy     a device-to-device copy of 32 u bytes measured in the same run (64 u bytes of traffic)
  B/row    the bytes the plan moves per row for that input: per sort 32 (byte histograms) + 102 per moving
           pass (32 tile histogram, 32 + 32 scatter, 6 count matrix); 250 for heads, prefix sums, leftovers and fill
  host     for k in --host-ks: what a caller had to do before — both columns to the host, one single-threaded sort of each
           (numpy lexsort over the eight 32-bit words, most significant last: the order of halo2's sort()), both permuted
           columns back.  The copies are timed over page-locked memory, each way, in the same run; the sort by the wall
           clock (best of three up to k = 20, one run above: a sort of 2^24 keys takes the better part of a minute).  The
           rebuilding of the table column on the host is NOT included: the host figure is a lower bound of that route.
           ratio = host / device.
  check    where the host sort runs its result also checks the device's: ap is the sorted input, sp a permutation of the
           table, ap[0] = sp[0], and every row has ap[i] = sp[i] or ap[i] = ap[i-1].  A mismatch ends the run with an error.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry

REPS = 10
PLAN_BYTES = {"random": 2 * (32 + 32 * 102) + 250, "16-bit": 2 * (32 + 2 * 102) + 250}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="16,20,22,24")
    ap.add_argument("--host-ks", default="16,20,22,24")
    args = ap.parse_args()
    import numpy as np
    import torch
    pkg = entry.load_package()
    eng = pkg.H2Agg(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    eng.set_stream(stream.cuda_stream)
    torch.set_num_threads(1)

    def bracket(f, reps=REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            for _ in range(reps):
                f()
            e1.record(stream)
        eng.synchronize()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def measure(f):
        f()
        f()
        eng.synchronize()
        return statistics.median(bracket(f) for _ in range(5))

    def table(kind, n, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        d = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g)
        if kind == "random":
            d[:, 31] = (d[:, 31] & 0x0F) | 0x20        # 254 bits, below r
        else:
            d[:, 2:] = 0
        rows = torch.randint(0, n - 6, (n,), generator=g)
        return d[rows].contiguous(), d

    def host_sort(col, runs):
        words = np.ascontiguousarray(col.numpy()).view("<u4").reshape(-1, 8)
        best = None
        for _ in range(runs):
            t0 = time.perf_counter()
            order = np.lexsort([words[:, j] for j in range(8)])
            ordered = words[order]
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None else min(best, dt)
        return best, ordered

    def check(a_sorted, s_sorted, ap, sp, what):
        ap = np.ascontiguousarray(ap.cpu().numpy()).view("<u4").reshape(-1, 8)
        sp = np.ascontiguousarray(sp.cpu().numpy()).view("<u4").reshape(-1, 8)
        if not np.array_equal(ap, a_sorted):
            sys.exit("%s: ap is not the sorted input" % what)
        if not np.array_equal(sp[np.lexsort([sp[:, j] for j in range(8)])], s_sorted):
            sys.exit("%s: sp is not a permutation of the table" % what)
        same = (ap == sp).all(axis=1)
        rep = np.concatenate(([False], (ap[1:] == ap[:-1]).all(axis=1)))
        if not same[0] or not (same | rep).all():
            sys.exit("%s: a row has neither ap = sp nor ap = the row above" % what)

    host_ks = {int(x) for x in args.host_ks.split(",") if x}
    print("# %s" % eng.describe())
    print("# tile: 2^%d keys per workgroup; %d calls per bracket, median of 5 brackets; u = 2^k - 6; times in ms" % (pkg.FR_SORT_TILE, REPS))
    print("# plan bytes per row: " + ", ".join("%s %d" % kv for kv in PLAN_BYTES.items()))
    print("#  k  input    copy ms  permute ms  x copy  B/row | host: 2 sorts   4 copies    total   ratio")
    for k in [int(x) for x in args.ks.split(",") if x]:
        n, u = 1 << k, (1 << k) - 6
        for kind in ("random", "16-bit"):
            a_h, s_h = table(kind, n, 31 * k + len(kind))
            d_a, d_s = a_h.to(dev), s_h.to(dev)
            d_ap, d_sp = torch.empty_like(d_a), torch.empty_like(d_s)
            torch.cuda.synchronize()

            def copy():
                with torch.cuda.stream(stream):
                    d_ap[:u].copy_(d_a[:u])

            t_copy = measure(copy)
            t_perm = measure(lambda: eng.lookup_permute_device(d_a.data_ptr(), d_s.data_ptr(), k, u, d_ap.data_ptr(), d_sp.data_ptr()))
            tail = "       -          -        -       -"
            if k in host_ks:
                runs = 3 if k <= 20 else 1
                (t_a, a_sorted), (t_s, s_sorted) = host_sort(a_h[:u], runs), host_sort(s_h[:u], runs)
                check(a_sorted, s_sorted, d_ap[:u], d_sp[:u], "k = %d, %s" % (k, kind))
                del a_sorted, s_sorted
                pin = torch.empty((u, 32), dtype=torch.uint8).pin_memory()

                def down():
                    with torch.cuda.stream(stream):
                        pin.copy_(d_a[:u], non_blocking=True)

                def upl():
                    with torch.cuda.stream(stream):
                        d_ap[:u].copy_(pin, non_blocking=True)

                t_copies = 2 * measure(down) + 2 * measure(upl)
                t_sorts = t_a + t_s
                total = t_sorts + t_copies
                tail = "%8.2f  %9.3f  %7.2f  %6.1f" % (t_sorts, t_copies, total, total / t_perm)
                del pin
            print("%4d  %-7s %8.4f  %10.4f  %6.1f  %5d | %s" % (k, kind, t_copy, t_perm, t_perm / t_copy, PLAN_BYTES[kind], tail))
            sys.stdout.flush()
            del d_a, d_s, d_ap, d_sp
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
