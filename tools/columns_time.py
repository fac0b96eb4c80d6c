#!/usr/bin/env python3
"""Timing of the Fr column stores: the five slab families through their host-buffer entry points and through a store, and the
stores' two kernels beside the copy that bounds them.

    python tools/columns_time.py [--ks 16,20] [--out profiles/columns.txt]

Shape: the honest prover's circuit (tools/witness_check_time.py builds it: 3 advice, 3 fixed and 1 instance column, 2 gate
polynomials, 7 permutation columns, 1 lookup) and, for the Shplonk opening, tools/shplonk_time.py's 34 polynomials in sets of
1, 2 and 3 points.

  families  h2agg_fr_fft_batch (the 7 columns, inverse), h2agg_commit_columns (the 7 columns against g_lagrange),
            h2agg_permutation_sigmas (both outputs), h2agg_witness_check (everything, max_rows = 16), h2agg_kzg_shplonk_begin —
            each beside its resident form over stores written once, outside the clock.  The two legs ALTERNATE in one process:
            host call, resident call, ROUNDS times behind one warm-up round.  `wall` is the wall clock around the call (the
            queued h2agg_columns_fft: around the call and h2agg_synchronize).  Where the family has a phase clock (debug key
            phases, h2agg_last_phases) its columns follow, each the median of the same calls.  The yardstick is the host leg of
            the same run; the resident leg is expected at about the host leg minus what its `stage` / `copy` phases shrink by
            (the mapping of the sigma columns and of the witness check still crosses; for the families without those phases
            `host - resident` is the measure of the slab's crossing).
  kernels   k_columns_move (rotation 1) over 34 columns between two stores, bracketed by two events on the context's stream;
            k_columns_canonical over the same 34 columns as the `check` phase of an h2agg_columns_write; a device-to-device
            copy of the same bytes in the same run (one read plus one write of the slab: the move's bound; the check only
            reads, so half of it is the check's).
Median [min .. max] over the rounds: the spread a difference has to exceed."""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry
import witness_check_time as WT
from shplonk_time import SETS, fe

ROUNDS = 5
KERNEL_COLUMNS = 34


def spread(xs):
    return "%9.4f [%9.4f .. %9.4f]" % (statistics.median(xs), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="16,20")
    ap.add_argument("--out", default=os.path.join(entry.ROOT, "profiles", "columns.txt"))
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    verifier = importlib.import_module(entry.PKG_NAME + ".verifier")
    eng = pkg.H2Agg(0)
    lib, ctx, check = eng._lib, eng._ctx, eng._check
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    eng.set_stream(stream.cuda_stream)
    eng.debug_configure("phases", 1)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def phases():
        return WT.phases_of(eng.last_phases())

    def legs(name, host, resident, has_phases):
        """alternate the two legs; -> nothing, says the family's lines"""
        t = {"host": [], "resident": []}
        ph = {"host": [], "resident": []}
        for r in range(ROUNDS + 1):                   # the first round warms up
            for leg, f in (("host", host), ("resident", resident)):
                t0 = time.perf_counter()
                f()
                dt = (time.perf_counter() - t0) * 1e3
                if r:
                    t[leg].append(dt)
                    if has_phases:
                        ph[leg].append(phases())
        say("  %s" % name)
        saved = 0.0                                   # what the resident leg's stage / copy phases are shorter by
        for leg in ("host", "resident"):
            say("    %-9s wall %s" % (leg, spread(t[leg])))
            if has_phases:
                for key in ph[leg][0]:
                    col = [p[key] for p in ph[leg]]
                    say("      %-11s %s" % (key, spread(col)))
                    if key in ("stage", "copy"):
                        saved += statistics.median(col) * (1 if leg == "host" else -1)
        mh, mr = statistics.median(t["host"]), statistics.median(t["resident"])
        if has_phases and saved:
            say("    host - (its stage + copy less the resident leg's) = %.4f; resident = %.4f; host / resident = %.2f" % (mh - saved, mr, mh / mr))
        else:
            say("    host - resident = %.4f; host / resident = %.2f" % (mh - mr, mh / mr))

    def bracket(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            f()
            e1.record(stream)
        eng.synchronize()
        e1.synchronize()
        return e0.elapsed_time(e1)

    queries, at = [], 0
    for count, pts in SETS:
        queries += [(m, p) for m in range(at, at + count) for p in pts]
        at += count
    npoly = at
    assert npoly == KERNEL_COLUMNS
    zs = b"".join(fe(0x1234567890ABCDEF0FEDCBA987654321 ** (3 + p)) for p in range(6))
    y, v = fe(0xFEDCBA9876543210123456789ABCDEF ** 5), fe(0x0F1E2D3C4B5A69788796A5B4C3D2E1F ** 7)
    delta = fe(7)

    say("# %s" % eng.describe())
    say("# host-buffer entry point against its resident form over column stores, alternating; %d rounds behind one warm-up;" % ROUNDS)
    say("# times in ms, median [min .. max]")
    for k in [int(x) for x in a.ks.split(",") if x]:
        n = 1 << k
        col = 32 * n
        say("k = %d" % k)
        g, gl = eng.params_setup(k, fe(0x5EC2E7 ** 9))
        chk = WT.Check(pkg, eng, verifier, k, k)
        slab = b"".join(chk.slabs)                                       # advice, fixed, instance: 7 columns
        words = (C.c_uint32 * (len(chk.mapping) // 4)).from_buffer_copy(chk.mapping)
        u = n - WT.BF - 1
        host_in, host_out, host_out2 = C.create_string_buffer(slab, len(slab)), C.create_string_buffer(7 * col), C.create_string_buffer(7 * col)
        points = C.create_string_buffer(64 * 7)
        A, B, Cc = eng.columns_create(7, k), eng.columns_create(7, k), eng.columns_create(7, k)
        eng.columns_write(A, 0, slab)

        def fft_resident():
            eng.columns_fft(A, 0, B, 0, 7, True)
            eng.synchronize()
        legs("fr_fft_batch, 7 columns, inverse", lambda: check(lib.h2agg_fr_fft_batch(ctx, host_in, 7, k, 1, None, host_out)),
             fft_resident, False)
        legs("commit_columns, 7 columns", lambda: check(lib.h2agg_commit_columns(ctx, gl, host_in, 7, k, points)),
             lambda: check(lib.h2agg_columns_commit(ctx, gl, A, 0, 7, points)), False)
        legs("permutation_sigmas, 7 columns, both outputs",
             lambda: check(lib.h2agg_permutation_sigmas(ctx, words, 7, k, u, delta, host_out, host_out2)),
             lambda: check(lib.h2agg_columns_sigmas(ctx, words, 7, k, u, delta, B, 0, Cc, 0)), True)

        def wc_resident():
            check(lib.h2agg_columns_witness_check(ctx, chk.vk._vk, 7, A, 0, A, 3, A, 6, None, chk.theta, words, chk.max_rows, chk.counts,
                                                  chk.first, chk.rows, C.byref(chk.total)))
        legs("witness_check", chk.call, wc_resident, True)
        assert chk.total.value == 0
        for h in (A, B, Cc):
            eng.columns_destroy(h)
        eng.bases_free(gl)
        chk.vk.close()
        del host_in, host_out, host_out2, slab, chk

        gen = torch.Generator(device="cpu").manual_seed(k)
        slab_t = torch.randint(0, 256, (npoly << k, 32), dtype=torch.uint8, generator=gen)
        slab_t[:, 31] &= 0x1F                                            # every element < 2^253 < r
        slab = slab_t.numpy().tobytes()
        S, S2 = eng.columns_create(npoly, k), eng.columns_create(npoly, k)
        eng.columns_write(S, 0, slab_t.data_ptr(), npoly)
        evals = eng.fr_poly_eval(slab, k, queries, zs)

        def sh_host():
            _h1, obj = eng.kzg_shplonk_begin(g, slab, k, queries, zs, evals, y, v)
            eng.kzg_shplonk_destroy(obj)

        def sh_resident():
            _h1, obj = eng.columns_shplonk_begin(g, S, 0, npoly, queries, zs, evals, y, v)
            eng.kzg_shplonk_destroy(obj)
        legs("shplonk_begin, %d polynomials, %d queries (wall with the object's destruction)" % (npoly, len(queries)), sh_host, sh_resident, True)

        # ---- the two kernels beside the copy of the same bytes
        d_a = slab_t.to(dev)
        d_b = torch.empty_like(d_a)
        torch.cuda.synchronize()
        t_move, t_copy, t_check = [], [], []
        for r in range(ROUNDS + 1):
            mv = bracket(lambda: eng.columns_move(S, 0, S2, 0, npoly, 1))
            cp = bracket(lambda: d_b.copy_(d_a))
            eng.columns_write(S, 0, slab_t.data_ptr(), npoly)
            ck = phases()["check"]
            if r:
                t_move.append(mv)
                t_copy.append(cp)
                t_check.append(ck)
        mc = statistics.median(t_copy)
        say("  kernels over %d columns of 2^%d (%.1f MiB)" % (npoly, k, npoly * col / 2.0 ** 20))
        say("    copy                 %s   (device to device: one read + one write)" % spread(t_copy))
        say("    k_columns_move       %s   %.2f x the copy" % (spread(t_move), statistics.median(t_move) / mc))
        say("    k_columns_canonical  %s   %.2f x the copy, %.2f x half of it (the check only reads)"
            % (spread(t_check), statistics.median(t_check) / mc, 2 * statistics.median(t_check) / mc))
        eng.columns_destroy(S)
        eng.columns_destroy(S2)
        eng.bases_free(g)
        del d_a, d_b, slab_t, slab
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
