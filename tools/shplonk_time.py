#!/usr/bin/env python3
"""Timing of the Shplonk prover (h2agg_kzg_shplonk_begin / _finish) and of its set division beside the baseline it replaces.

    python tools/shplonk_time.py [--ks 16,20] [--out profiles/shplonk.txt]

Shape: 34 polynomials in three sets of 1, 2 and 3 points (16, 12 and 6 polynomials: a small circuit with a permutation and a
lookup), 58 queries.  The slab is host memory, as the entry points take it.

  begin / finish   the wall clock around one synchronous call after one warm-up call, median of ROUNDS, and the call's own split
           by events on the context's stream (debug key phases, h2agg_last_phases), each column the median of the same calls.
           `stage` is the slab's copy to the device from pageable memory.
  set division at |S| = 3, the two routes computing the same N / Z_S for one array N, ALTERNATING, ROUNDS times each:
      fused     the `divide` phase of a begin call over one polynomial opened at three points: one up-sweep launch per level
                over the three queries (N, z), the upper down-sweep levels per point, then k_fr_shplonk_leaf, which reads N once,
                carries the three chains and writes the weighted sum once.  (The call's first set writes h; a later set also
                reads h to add to it: one more pass, counted below.)
      baseline  three successive h2agg_fr_poly_divide_device calls in place on a resident array, bracketed by two events: per
                call an up-sweep and a down-sweep.
      Array passes of 32 n bytes: baseline 3 x (read, read, write) = 9; fused 3 reads (up-sweep) + 1 read + 1 write (leaf) = 5,
      6 when it accumulates.  The leaf alone is 2 or 3 passes against the 6 of the baseline's three down-sweeps.
  copy     a device-to-device copy of 32 n bytes in the same run: one read plus one write of the array.
The minimum and maximum over the rounds stand beside each median: the run-to-run spread that a difference has to exceed."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry

ROUNDS = 5
SETS = [(16, [0]), (12, [1, 2]), (6, [3, 4, 5])]   # (polynomials, points)
R = int.from_bytes(bytes.fromhex("010000f093f5e1439170b97948e833285d588181b64550b829a031e1724e6430"), "little")


def fe(x):
    return (x % R).to_bytes(32, "little")


def spread(xs):
    return "%9.4f [%9.4f .. %9.4f]" % (statistics.median(xs), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="16,20")
    ap.add_argument("--out", default=os.path.join(entry.ROOT, "profiles", "shplonk.txt"))
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    eng = pkg.H2Agg(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    eng.set_stream(stream.cuda_stream)
    eng.debug_configure("phases", 1)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def host_slab(k, npoly, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        d = torch.randint(0, 256, (npoly << k, 32), dtype=torch.uint8, generator=g)
        d[:, 31] &= 0x1F                              # every element < 2^253 < r
        return d

    def phases():
        return [float(f.split("=")[1]) for f in eng.last_phases().split()]

    queries, at = [], 0
    for count, pts in SETS:
        queries += [(m, p) for m in range(at, at + count) for p in pts]
        at += count
    npoly = at
    zs = b"".join(fe(0x1234567890ABCDEF0FEDCBA987654321 ** (3 + p)) for p in range(6))
    y, v, u = fe(0xFEDCBA9876543210123456789ABCDEF ** 5), fe(0x0F1E2D3C4B5A69788796A5B4C3D2E1F ** 7), fe(0x13579BDF02468ACE ** 11)

    say("# %s" % eng.describe())
    say("# %d polynomials, sets of 1 / 2 / 3 points with 16 / 12 / 6 polynomials, %d queries; %d rounds; times in ms, median [min .. max]"
        % (npoly, len(queries), ROUNDS))
    for k in [int(x) for x in a.ks.split(",") if x]:
        n = 1 << k
        g, gl = eng.params_setup(k, fe(0x5EC2E7 ** 9))
        eng.bases_free(gl)
        slab_t = host_slab(k, npoly, k)
        slab = slab_t.numpy().tobytes()
        evals = eng.fr_poly_eval(slab, k, queries, zs)
        t_begin, t_finish, s_begin, s_finish = [], [], [], []
        for r in range(ROUNDS + 1):                   # the first round warms up
            t0 = time.perf_counter()
            _h1, obj = eng.kzg_shplonk_begin(g, slab, k, queries, zs, evals, y, v)
            t1 = time.perf_counter()
            sb = phases()
            try:
                t2 = time.perf_counter()
                eng.kzg_shplonk_finish(obj, u)
                t3 = time.perf_counter()
                sf = phases()
            finally:
                eng.kzg_shplonk_destroy(obj)
            if r:
                t_begin.append((t1 - t0) * 1e3)
                t_finish.append((t3 - t2) * 1e3)
                s_begin.append(sb)
                s_finish.append(sf)
        say("k = %d" % k)
        say("  begin   wall %s" % spread(t_begin))
        for name, col in zip(("stage", "numerators", "divide", "commit"), zip(*s_begin)):
            say("    %-11s %s" % (name, spread(col)))
        say("  finish  wall %s" % spread(t_finish))
        for name, col in zip(("combine", "divide", "commit"), zip(*s_finish)):
            say("    %-11s %s" % (name, spread(col)))
        # the set division at |S| = 3: fused against three successive divisions, alternating
        one = slab[:32 * n]
        q3 = [(0, 3), (0, 4), (0, 5)]
        ev3 = eng.fr_poly_eval(one, k, q3, zs)
        d_num = slab_t[:n].to(dev)
        d_copy = torch.empty_like(d_num)
        torch.cuda.synchronize()

        def fused():
            _h1, obj = eng.kzg_shplonk_begin(g, one, k, q3, zs, ev3, y, v)
            eng.kzg_shplonk_destroy(obj)
            return phases()[2]

        def bracket(f):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record(stream)
                f()
                e1.record(stream)
            eng.synchronize()
            e1.synchronize()
            return e0.elapsed_time(e1)

        def baseline():
            for p in (3, 4, 5):
                eng.fr_poly_divide_device(d_num.data_ptr(), k, zs[32 * p:32 * p + 32], d_num.data_ptr(), None)

        def copy():
            d_copy.copy_(d_num)

        t_fused, t_base, t_copy = [], [], []
        for r in range(ROUNDS + 1):
            f, b, c = fused(), bracket(baseline), bracket(copy)
            if r:
                t_fused.append(f)
                t_base.append(b)
                t_copy.append(c)
        say("  division by Z_S, |S| = 3, one array of 2^%d" % k)
        say("    fused       %s" % spread(t_fused))
        say("    baseline    %s   (three h2agg_fr_poly_divide_device)" % spread(t_base))
        say("    copy        %s   (one read + one write)" % spread(t_copy))
        say("    fused / baseline = %.3f (medians)" % (statistics.median(t_fused) / statistics.median(t_base)))
        eng.bases_free(g)
        del d_num, d_copy, slab_t, slab
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
