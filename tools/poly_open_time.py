#!/usr/bin/env python3
"""Timing of the KZG opening path (h2agg_fr_poly_eval_device, h2agg_fr_poly_divide_device, h2agg_kzg_multiopen_device)
beside the bounds it could sit at.

    python tools/poly_open_time.py [--ks 16,20,22,24] > profiles/poly_open.txt
    rocprofv3 --kernel-trace --stats -- python tools/poly_open_time.py --only 20     (the three kernels' own lines: one eval,
                                                                                     one divide, one multiopen; on its own,
                                                                                     no counters in the run)

Method (that of tools/fr_fft_time.py).  The data is resident and the context runs on a stream of the caller.
  divide   asynchronous: two events on the stream bracket REPS calls queued back to back after two warm-up calls (which also
           grow the work buffer); median of five brackets / REPS.  In place: a quotient of random data is random data (its top
           coefficient, zero, is canonical too), so repeating it needs no reset.
  eval, multiopen   synchronous calls that end with a download, so events cannot bracket them back to back: the wall clock
           around one call, after two warm-up calls; median of five.  These figures include one stream synchronisation and the
           download of the results (32 B per query / 64 B per group).
  the multiopen is 8 polynomials at 3 points, 8 queries per point (24 queries, 3 groups).  Its split is the library's own
           (debug key `phases`, h2agg_last_phases): events on the context's stream around the call's linear combination
           (`combine`), its up- and down-sweep over the three groups in one set of launches (`divide`) and the batch MSM with
           the conversion to affine (`commit`, which includes the host's wait in front of the MSM); each column is the median
           over the five timed calls.  The three do not add up to the wall clock: that also has the host's grouping, the power
           tables, the upload of the lists and the download.

Bounds printed beside each time:
  copy     a device-to-device copy of the polynomial's 32 n bytes measured in the same run (reads and writes 32 n: 64 n bytes of
           traffic).  eval reads 32 n (half a copy); divide reads 32 n twice (up-sweep and down-sweep) and writes it once (1.5
           copies); the combination reads 8 x 32 n per group and writes 32 n.
  msm      h2agg_g1_msm_device of the same k over the same table (wall clock, synchronous): what one commitment costs.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry

REPS = 10
NPOLY, NPOINTS = 8, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="16,20,22,24")
    ap.add_argument("--only", type=int, default=0, help="one eval, one divide and one multiopen at this k after a warm-up of each")
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    eng = pkg.H2Agg(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    eng.set_stream(stream.cuda_stream)
    eng.debug_configure("phases", 1)
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

    def resident(k, npoly, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        d = torch.randint(0, 256, (npoly << k, 32), dtype=torch.uint8, generator=g)
        d[:, 31] &= 0x1F                              # every element < 2^253 < r
        d = d.to(dev)
        torch.cuda.synchronize()
        return d

    zs = b"".join(fe(0x1234567890ABCDEF0FEDCBA987654321 ** (3 + p)) for p in range(NPOINTS))
    v = fe(0xFEDCBA9876543210123456789ABCDEF ** 5)
    queries = [(m, p) for p in range(NPOINTS) for m in range(NPOLY)]

    def one(k, report):
        n = 1 << k
        g, gl = eng.params_setup(k, fe(0x5EC2E7 ** 9))
        eng.bases_free(gl)
        d = resident(k, NPOLY, k)
        w = resident(k, 1, k + 8)
        e = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def copy():
            with torch.cuda.stream(stream):
                e.copy_(d[:n])

        split = []

        def mo():
            eng.kzg_multiopen_device(g, d.data_ptr(), NPOLY, k, queries, zs, v)
            split.append([float(f.split("=")[1]) for f in eng.last_phases().split()])

        ev1 = lambda: eng.fr_poly_eval_device(d.data_ptr(), NPOLY, k, [(0, 0)], zs)
        div1 = lambda: eng.fr_poly_divide_device(w.data_ptr(), k, zs[:32], w.data_ptr(), None)
        if not report:
            for f in (ev1, div1, mo):
                f()
                eng.synchronize()
                f()
                eng.synchronize()
            eng.bases_free(g)
            return
        t_copy = measure(copy)
        t_eval = wall(ev1)
        t_div = measure(div1)
        t_mo = wall(mo)
        t_comb, t_div3, t_commit = (statistics.median(col) for col in zip(*split[-5:]))
        t_msm = wall(lambda: eng.g1_msm_device(g, w.data_ptr(), n))
        print("%4d  %8.4f  %8.4f  %8.4f  %8.4f  %9.4f  %8.4f  %8.4f  %9.4f  %9.4f" % (
            k, t_copy, t_eval, t_div, 1.5 * t_copy, t_mo, t_comb, t_div3, t_commit, t_msm))
        sys.stdout.flush()
        eng.bases_free(g)
        del d, w, e
        torch.cuda.empty_cache()

    if a.only:
        one(a.only, False)
        return
    print("# %s" % eng.describe())
    print("# chunk: 2^%d coefficients per workgroup; divide: %d calls per bracket, median of 5 brackets; eval, multiopen, commit, msm:"
          " wall clock of one synchronous call, median of 5; times in ms" % (pkg.FR_POLY_CHUNK, REPS))
    print("# multiopen: %d polynomials, %d points, %d queries, 3 groups; combine / divide3 / commit3: that call's own split by"
          " events (h2agg_last_phases), median of the same 5 calls" % (NPOLY, NPOINTS, len(queries)))
    print("#  k   copy ms      eval    divide  1.5 copy  multiopen   combine   divide3    commit3   msm(one)")
    for k in [int(x) for x in a.ks.split(",") if x]:
        one(k, True)


if __name__ == "__main__":
    main()
