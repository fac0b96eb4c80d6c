#!/usr/bin/env python3
"""Timing of the grand-product path (h2agg_fr_batch_invert_device, h2agg_fr_grand_product_device,
h2agg_permutation_product_device, h2agg_lookup_product_device) beside the bounds it could sit at.

    python tools/grand_product_time.py [--ks 16,20,22,24] > profiles/grand_product.txt

Method (that of tools/poly_open_time.py).  The data is resident and the context runs on a stream of the caller; every call
is the asynchronous device variant: two events on the stream bracket REPS calls queued back to back after two warm-up
calls (which also grow the work buffers); median of five brackets / REPS.  The inversion runs in place on random non-zero
data (the inverse of random data is random data); the products write to a buffer of their own.  u = n - 6.

Beside each time:
  copy     a device-to-device copy of 32 n bytes measured in the same run (reads and writes 32 n: 64 n bytes of traffic),
           and the bytes the call moves per row in units of that copy's 64 B per row
  products the field products per row the call issues.  The issue cost of one product has no measured
           figure in this project, so the column is the count, not a time.
  parent   at n = 2^16 and 2^20: h2agg_fr_batch_op(INV) on the same non-zero input, the only route to the same inverses
           before this path existed — a synchronous host-buffer call, so it is timed by the wall clock (median of five
           after two warm-up calls) and includes the upload and download of 32 n bytes each way, which
           h2agg_fr_batch_invert (the synchronous host-buffer form of the new path, timed the same way beside it) includes too.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry

REPS = 10
M = 4
# per row: (products, bytes) of the version that ships
COST = {"invert": (4, 96), "product": (5, 96), "ratio": (9, 256), "perm": (9 + 4 * M + 1, 256 + 64 * M + 64), "lookup": (9 + 4, 256 + 128 + 64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="16,20,22,24")
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    eng = pkg.H2Agg(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    eng.set_stream(stream.cuda_stream)
    R = int.from_bytes(bytes.fromhex("010000f093f5e1439170b97948e833285d588181b64550b829a031e1724e6430"), "little")

    def fe(x):
        return (x % R).to_bytes(32, "little")

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

    def wall(f):
        f()
        f()
        out = []
        for _ in range(5):
            t0 = time.perf_counter()
            f()
            out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out)

    def resident(rows, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        d = torch.randint(0, 256, (rows, 32), dtype=torch.uint8, generator=g)
        d[:, 31] &= 0x1F                              # every element < 2^253 < r
        d[:, 0] |= 1                                  # and non-zero
        return d

    beta, gamma, delta = fe(0x1234567890ABCDEF0FEDCBA987654321 ** 3), fe(0xFEDCBA9876543210123456789ABCDEF ** 5), fe(7 ** 90)
    one = fe(1)

    print("# %s" % eng.describe())
    print("# chunk: 2^%d elements per workgroup; %d calls per bracket, median of 5 brackets; u = n - 6; permutation: m = %d; times in ms"
          % (pkg.FR_SCAN_CHUNK, REPS, M))
    print("# per row (products, bytes): " + ", ".join("%s %d / %d" % (name, p, b) for name, (p, b) in COST.items()))
    print("#  k   copy ms    invert   product     ratio  permutation    lookup | host: batch_invert  batch_op(INV)  ratio")
    for k in [int(x) for x in a.ks.split(",") if x]:
        n, u = 1 << k, (1 << k) - 6
        host = resident(n, k)
        x = host.to(dev)
        cols = resident(2 * M * n, k + 32).to(dev)
        out = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        p = lambda t, row=0: t.data_ptr() + 32 * row

        def copy():
            with torch.cuda.stream(stream):
                out.copy_(x)

        t_copy = measure(copy)
        t_inv = measure(lambda: eng.fr_batch_invert_device(p(x), n, p(x)))
        t_prod = measure(lambda: eng.fr_grand_product_device(p(cols), None, k, u, one, p(out)))
        t_ratio = measure(lambda: eng.fr_grand_product_device(p(cols), p(cols, n), k, u, one, p(out)))
        t_perm = measure(lambda: eng.permutation_product_device(p(cols), p(cols, M * n), M, k, u, beta, gamma, delta, one, one, p(out)))
        t_look = measure(lambda: eng.lookup_product_device(p(cols), p(cols, n), p(cols, 2 * n), p(cols, 3 * n), k, u, beta, gamma, p(out)))
        tail = "                 -              -      -"
        if k in (16, 20):
            data = bytes(host.numpy().tobytes())
            t_new = wall(lambda: eng.fr_batch_invert(data))
            t_old = wall(lambda: eng.fr_batch_op(pkg.OP_INV, data))
            assert eng.fr_batch_invert(data) == eng.fr_batch_op(pkg.OP_INV, data)
            tail = "%18.4f  %13.4f  %5.1f" % (t_new, t_old, t_old / t_new)
        print("%4d  %8.4f  %8.4f  %8.4f  %8.4f  %11.4f  %8.4f | %s" % (k, t_copy, t_inv, t_prod, t_ratio, t_perm, t_look, tail))
        sys.stdout.flush()
        del x, cols, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
