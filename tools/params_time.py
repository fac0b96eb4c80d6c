#!/usr/bin/env python3
"""Timing of the KZG-parameter entry points: h2agg_params_setup and h2agg_bases_fft (inverse: g_to_lagrange).

    python tools/params_time.py [--ks 12,16,20,22] [--oracle-ks 12,14] > profiles/params.txt
    rocprofv3 --kernel-trace --stats -- python tools/params_time.py --only-fft 20      (the stage kernel's own line;
                                                                                        on its own, no counters in the run)

Method: both calls are synchronous and move nothing across PCIe (handles in, handles out), so the wall clock around a call
is the device time of its kernels plus the call's own hipMalloc / hipFree of the work arrays; p50 of 5 calls after one
warm-up call (which also builds the context's comb table and twiddle records).  The oracle figure is the C restatement's
Pippenger multi_exp (oracle/cref.py msm_pippenger, 16 threads) over a sample of output rows, scaled to all 2^k rows: the
definition evaluated row by row, which is what the tests compare against."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
S = (0x1234567890ABCDEF << 128 | 0xFEDCBA0987654321).to_bytes(32, "little")


def p50(f, reps=5):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="12,16,20,22")
    ap.add_argument("--oracle-ks", default="12,14")
    ap.add_argument("--oracle-rows", type=int, default=16)
    ap.add_argument("--only-fft", type=int, default=0, help="one setup and one inverse transform at this k, nothing else")
    a = ap.parse_args()
    pkg = entry.load_package()
    eng = pkg.H2Agg(0)
    if a.only_fft:
        hg, hl = eng.params_setup(a.only_fft, S)
        eng.bases_free(eng.bases_fft(hg, a.only_fft, True))
        return
    print("# %s" % eng.describe())
    print("# k  params_setup ms (p50 min max)   bases_fft inverse ms (p50 min max)   scalar multiplications of the transform")
    for k in [int(x) for x in a.ks.split(",") if x]:
        def setup():
            hs = eng.params_setup(k, S)
            for h in hs:
                eng.bases_free(h)
        try:
            ts = p50(setup)
            hg, hl = eng.params_setup(k, S)
        except pkg.H2AggError as e:
            print("%2d  not run: %s" % (k, e))
            continue
        try:
            tf = p50(lambda: eng.bases_free(eng.bases_fft(hg, k, True)))
            muls = (1 << k) + (1 << (k - 1)) * (k - 1) - ((1 << (k - 1)) - 1)   # 1/n per point; per stage s >= 2 all but position 0
            print("%2d  %10.3f %10.3f %10.3f   %10.3f %10.3f %10.3f   %d" % ((k,) + ts + tf + (muls,)))
        except pkg.H2AggError as e:
            print("%2d  %10.3f %10.3f %10.3f   not run: %s" % ((k,) + ts + (e,)))
        finally:
            eng.bases_free(hg)
            eng.bases_free(hl)
        sys.stdout.flush()
    from oracle import cref
    from oracle import verifier as V
    print("# oracle (C, msm_pippenger with 16 threads, %d sampled rows scaled to 2^k rows)" % a.oracle_rows)
    for k in [int(x) for x in a.oracle_ks.split(",") if x]:
        n = 1 << k
        hg, hl = eng.params_setup(k, S)
        g = eng.bases_download(hg, 0, n)
        eng.bases_free(hg)
        eng.bases_free(hl)
        winv, ninv = pow(V.omega_for_k(k), R - 2, R), pow(n, R - 2, R)
        total = 0.0
        for r in range(a.oracle_rows):
            i = (r * 2654435761 + 1) % n
            wi, cur, sc = pow(winv, i, R), ninv, []
            for _ in range(n):
                sc.append(cur.to_bytes(32, "little"))
                cur = cur * wi % R
            sc = b"".join(sc)
            t0 = time.perf_counter()
            cref.msm_pippenger(g, sc, n, nthreads=16)
            total += time.perf_counter() - t0
        print("%2d  %.1f ms per row, %.1f s for the transform" % (k, total / a.oracle_rows * 1e3, total / a.oracle_rows * n))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
