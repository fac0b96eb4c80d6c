#!/usr/bin/env python3
"""Timing of the keys block: h2agg_permutation_sigmas split into its phases, and h2agg_commit_columns against the loop of
single MSMs it replaces.

    python tools/keygen_time.py > profiles/keygen.txt

Method.  Both entry points are synchronous over host buffers, so every figure includes what a caller pays.

Sigma columns (m = 8 columns, k = 16 and 20; a random permutation of the usable cells, the rows from `usable` up fixed):
the library is called directly over buffers allocated once (no Python copies inside the bracket).  With the debug key
"phases" the call brackets its own phases with events on the context's stream and h2agg_last_phases returns them:
  stage    the mapping's copy to the device (8 B per cell) and the roll of the status flags
  sigma    the bitmap's clear, the delta table (k_fr_powers) and k_perm_sigma
  inverse  the batched inverse transform of the m columns (h2agg_fr_fft_batch's launches)
  copy     both slabs back to the host (64 B per cell)
Two warm-up calls (they grow the buffers and build the twiddle tables), then the median of five calls per phase; `wall` is
the median wall-clock time of the same five calls, which adds the host's range scan and the synchronisations.
  copy bound   k_perm_sigma reads 8 B and writes 32 B per cell: 40 B of traffic.  A device-to-device copy of the 32 B-per-cell
               slab, measured in the same run on the same stream (median of five brackets of ten copies), moves 64 B per cell,
               so the bound is 40 / 64 of that copy's time — the copy's rate, not the data sheet's bandwidth.  The bitmap's
               atomics and the table reads are not in it.
  valu bound   two Montgomery products per cell (the twiddle tables' halves, then delta^c with the conversion out) x 882
               cycles per wave64 product / 64 lanes / 1024 SIMDs at 2.08 GHz (the figures of tools/fr_fft_time.py and
               DESIGN.md sections 4 and 9).  An upper bound on the product count (a zero half of an exponent needs no
               twiddle product); the range and identity tests, the atomic and the reduction to canonical form are not in it.

Commitments (m = 8 and 34 columns of random canonical scalars, k = 12 and 16, against g_lagrange of h2agg_params_setup):
  loop     m calls of h2agg_g1_msm_preloaded, one column each — what there was before the slab call (Jacobian results)
  slab     one h2agg_commit_columns call (affine results: it also pays one batched inversion)
Two warm-up rounds, then the median wall-clock time of five rounds.
"""
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
DELTA = 7   # any canonical value: the time does not depend on it
CYCLES_PER_PRODUCT = 882
SIMDS, CLOCK_HZ = 1024, 2.08e9


def random_mapping(np, m, k, usable, seed):
    """a valid mapping: a random permutation of the usable cells, the identity on the rows from `usable` up"""
    n = 1 << k
    rng = np.random.default_rng(seed)
    cols, rows = np.meshgrid(np.arange(m, dtype=np.uint32), np.arange(n, dtype=np.uint32), indexing="ij")
    mp = np.stack([cols, rows], axis=-1)                       # [m][n][2]
    usable_cells = mp[:, :usable, :].reshape(-1, 2)
    mp[:, :usable, :] = usable_cells[rng.permutation(len(usable_cells))].reshape(m, usable, 2)
    return np.ascontiguousarray(mp.reshape(-1))


def phases_of(line):
    return {k: float(v) for k, v in (item.split("=") for item in line.split())}


def main():
    import numpy as np
    import torch
    pkg = entry.load_package()
    eng = pkg.H2Agg(0)
    lib = eng._lib
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    eng.set_stream(stream.cuda_stream)
    print("# %s" % eng.describe())
    delta = DELTA.to_bytes(32, "little")

    print("# h2agg_permutation_sigmas, m = 8, both outputs; two warm-up calls, median of 5 calls; times in ms")
    print("#  k     cells      stage      sigma    inverse       copy       wall   slab copy   copy bound   valu bound   sigma / copy bound")
    eng.debug_configure("phases", 1)
    for k in (16, 20):
        m, n = 8, 1 << k
        usable = n - 6
        words = random_mapping(np, m, k, usable, k)
        lag = np.empty(32 * m * n, dtype=np.uint8)
        co = np.empty(32 * m * n, dtype=np.uint8)

        def call():
            eng._check(lib.h2agg_permutation_sigmas(eng._ctx, words.ctypes.data, m, k, usable, delta, lag.ctypes.data, co.ctypes.data))
        call()
        call()
        rows, walls = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            call()
            walls.append((time.perf_counter() - t0) * 1e3)
            rows.append(phases_of(eng.last_phases()))
        med = {name: statistics.median(r[name] for r in rows) for name in ("stage", "sigma", "inverse", "copy")}
        a = torch.empty(32 * m * n, dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)

        def bracket():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record(stream)
                for _ in range(10):
                    b.copy_(a)
                e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / 10
        bracket()
        t_copy = statistics.median(bracket() for _ in range(5))
        bound = t_copy * 40.0 / 64.0
        valu = 2.0 * m * n / 64.0 * CYCLES_PER_PRODUCT / SIMDS / CLOCK_HZ * 1e3
        print("%4d  %8d  %9.4f  %9.4f  %9.4f  %9.4f  %9.3f   %9.4f    %9.4f    %9.4f   %18.2f" % (
            k, m * n, med["stage"], med["sigma"], med["inverse"], med["copy"], statistics.median(walls), t_copy, bound, valu,
            med["sigma"] / bound))
        sys.stdout.flush()
        del a, b, lag, co, words
        torch.cuda.empty_cache()
    eng.debug_configure("phases", 0)

    print("# h2agg_commit_columns against m calls of h2agg_g1_msm_preloaded; two warm-up rounds, median wall clock of 5; times in ms")
    print("#  k    m       loop       slab   loop / slab")
    rng = np.random.default_rng(1)
    for k in (12, 16):
        n = 1 << k
        _g, gl = eng.params_setup(k, (0x5EED + k).to_bytes(32, "little"))
        for m in (8, 34):
            d = rng.integers(0, 256, size=(m * n, 32), dtype=np.uint8)
            d[:, 31] &= 0x1F                                   # every scalar < 2^253 < r
            slab = d.tobytes()
            columns = [slab[j * 32 * n:(j + 1) * 32 * n] for j in range(m)]
            out1 = C.create_string_buffer(96)
            outm = C.create_string_buffer(64 * m)

            def loop():
                for c in columns:
                    eng._check(lib.h2agg_g1_msm_preloaded(eng._ctx, gl, c, n, out1))

            def one():
                eng._check(lib.h2agg_commit_columns(eng._ctx, gl, slab, m, k, outm))

            def timed(f):
                f()
                f()
                ts = []
                for _ in range(5):
                    t0 = time.perf_counter()
                    f()
                    ts.append((time.perf_counter() - t0) * 1e3)
                return statistics.median(ts)
            t_loop, t_slab = timed(loop), timed(one)
            print("%4d  %3d  %9.3f  %9.3f   %11.2f" % (k, m, t_loop, t_slab, t_loop / t_slab))
            sys.stdout.flush()
        eng.bases_free(_g)
        eng.bases_free(gl)
    eng.close()


if __name__ == "__main__":
    main()
