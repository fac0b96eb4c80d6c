#!/usr/bin/env python3
"""Timing of h2agg_quotient_device: the call, its split by events, and the same transforms issued alone.

    python tools/quotient_time.py [--ks 16,18,20] > profiles/quotient.txt
    python tools/quotient_time.py --routes [--ks 16,18,20] >> profiles/quotient.txt     the two endings of the call, see below

One shape: 8 advice, 4 fixed and 1 instance column, 6 gate polynomials of degree <= 4 over rotations 0, +1 and -1, 8
permutation columns (four sets of chunk_len = 2), 2 lookups (2 + 2 and 1 + 1 expressions), degree 4: e = 2, four cosets, 34
polynomials with the three Lagrange columns, 3 pieces.  The inputs are random canonical elements (the circuit is not
satisfied: the work does not depend on the values).

Method (that of tools/grand_product_time.py).  Everything is resident and the context runs on a stream of the caller; two
events on the stream bracket one asynchronous call after two warm-up calls (which also grow the work memory); median of five
brackets.
  call        h2agg_quotient_device, debug key "phases" off
  split       one more call with the key on: the library's own events at the stage boundaries, summed over the four cosets
              (forward: the 34 transforms per coset and the three inverse transforms of the Lagrange rows; gates: the
              interpreter over the six gate polynomials; permutation; lookups: four interpreter launches and two fixed-form
              kernels per coset; inverse: the store to the extended domain is counted with the stage in front of it, the
              2^(k+2) inverse transform and the copy of the pieces here)
  transforms  the same 4 x 34 shifted forward transforms of size 2^k, 3 plain inverse ones and one shifted inverse of size
              2^(k+2), queued through h2agg_fr_fft_device alone (that entry point exists in the parent commit): what of the
              call is not new.  Each of these calls builds its own shift table and is its own set of launches; inside the
              quotient a coset is one batched transform (fr_fft_queue_batch): one table, one launch per pass for all 34.

--routes: the two endings of the call where both are legal (k + 2 <= 24), in one process on one context, alternating: the
h2agg_quotient_configure at 0 (the values of the four cosets interleaved, one inverse transform of size 2^(k+2)) and at 1
(per coset one inverse transform of size 2^k at the coset's shift, then k_qe_cross_cosets over the four results: twelve
products and 224 B per row).  Three rounds; per round and route the call (median of five brackets, key "phases" off) and the
`inverse` phase of one more call with the key on.  The pieces of the two routes are compared byte for byte first.
"""
import argparse
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry

G1 = (1).to_bytes(32, "little") + (2).to_bytes(32, "little")


def shape(k):
    A = lambda q: ("advice", q)
    F = lambda q: ("fixed", q)
    advice_queries = [(c, 0) for c in range(8)] + [(4, 1), (0, -1)]
    fixed_queries = [(c, 0) for c in range(4)]
    sub = lambda a, b: ("sum", a, ("neg", b))
    mul = lambda a, b: ("product", a, b)
    gates = [[mul(F(0), sub(mul(A(0), A(1)), A(2))), mul(F(0), sub(("sum", A(3), A(8)), A(5)))],
             [mul(F(1), mul(mul(A(6), A(7)), sub(A(0), ("const", 1))))],
             [mul(F(1), sub(mul(A(2), A(9)), ("scaled", A(4), 3))), mul(F(0), mul(A(5), sub(A(5), ("const", 1)))),
              mul(mul(F(0), F(1)), sub(A(1), A(7)))]]
    lookups = [([A(0), A(1)], [F(2), F(3)]), ([mul(F(0), A(2))], [F(3)])]
    perm = [("advice", c) for c in range(6)] + [("fixed", 2), ("instance", 0)]
    return types.SimpleNamespace(
        k=k, num_advice_columns=8, num_instance_columns=1, num_challenges=0, degree=4, blinding_factors=5,
        advice_column_phase=[0] * 8, challenge_phase=[], advice_queries=advice_queries, instance_queries=[(0, 0)],
        fixed_queries=fixed_queries, permutation_columns=perm, fixed_commitments=[G1] * 4, permutation_commitments=[G1] * 8,
        vk_scalar=1, gates=gates, lookups=lookups)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="16,18,20")
    ap.add_argument("--routes", action="store_true", help="the split ending against the default one, alternating")
    args = ap.parse_args()
    import importlib
    import torch
    pkg = entry.load_package()
    verifier = importlib.import_module(entry.PKG_NAME + ".verifier")
    poly = importlib.import_module(entry.PKG_NAME + ".poly")
    eng = pkg.H2Agg(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    eng.set_stream(stream.cuda_stream)

    def bracket(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            f()
            e1.record(stream)
        eng.synchronize()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def measure(f):
        f()
        f()
        eng.synchronize()
        return statistics.median(bracket(f) for _ in range(5))

    def slab(ncols, n, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        d = torch.randint(0, 256, (ncols * n, 32), dtype=torch.uint8, generator=g)
        d[:, 31] = (d[:, 31] & 0x0F) | 0x20            # 254 bits, below r
        return d.to(dev)

    sc = [(0x1234567 + 0x1111 * i).to_bytes(32, "little") for i in range(5)]
    print("# %s" % eng.describe())
    if args.routes:
        routes(args, eng, verifier, torch, dev, slab, sc, measure)
        return
    print("# 8 advice, 4 fixed, 1 instance, 6 gate polynomials, 8 permutation columns, 2 lookups, degree 4: 4 cosets, 34 polynomials")
    print("# one call per bracket, median of 5 brackets; times in ms")
    print("#  k    call ms | split: forward    gates  permutation  lookups  inverse | the transforms alone   share of the call")
    for k in [int(x) for x in args.ks.split(",") if x]:
        n = 1 << k
        cs = shape(k)
        vk = verifier.VerifyingKey(eng, verifier.encode_vk(cs, lambda p: p))
        counts = (8, 4, 1, 8, 4, 2, 2, 2)
        slabs = [slab(c, n, 97 * k + i) for i, c in enumerate(counts)]
        d_h = torch.empty((3 * n, 32), dtype=torch.uint8, device=dev)
        d_x = torch.zeros((4 * n, 32), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ptrs = [s.data_ptr() for s in slabs]
        call = lambda: eng.quotient_device(vk, *ptrs, None, *sc, d_h.data_ptr())
        t_call = measure(call)
        eng.debug_configure("phases", 1)
        call()
        split = dict(kv.split("=") for kv in eng.last_phases().split())
        eng.debug_configure("phases", 0)
        w_ext = pow(0x03DDB9F5166D18B798865EA93DD31F743215CF6DD39329C8D34F1ED960C37C9C, 1 << (28 - k - 2), poly.R_MOD)
        shifts = [(poly.ZETA_INT * pow(w_ext, c, poly.R_MOD) % poly.R_MOD).to_bytes(32, "little") for c in range(4)]

        def transforms():
            for t in range(3):
                eng.fr_fft_device(d_x.data_ptr() + 32 * n * t, k, True, None, d_x.data_ptr() + 32 * n * t)
            for s in shifts:
                for p in range(34):
                    src = ptrs[0] + 32 * n * (p % 8)
                    eng.fr_fft_device(src, k, False, s, d_x.data_ptr())
            eng.fr_fft_device(d_x.data_ptr(), k + 2, True, poly.ZETA, d_x.data_ptr())

        t_fft = measure(transforms)
        print("%4d  %9.3f | %14s %8s %12s %8s %8s | %20.3f   %16.2f" % (
            k, t_call, split.get("forward", "-"), split.get("gates", "-"), split.get("permutation", "-"), split.get("lookups", "-"),
            split.get("inverse", "-"), t_fft, t_fft / t_call))
        sys.stdout.flush()
        vk.close()
        del slabs, d_h, d_x
        torch.cuda.empty_cache()


def routes(args, eng, verifier, torch, dev, slab, sc, measure):
    print("# the two endings of h2agg_quotient_device, alternating in one process (h2agg_quotient_configure 0 / 1); times in ms")
    print("#  k  round |  default: call   inverse |    split: call   inverse")
    for k in [int(x) for x in args.ks.split(",") if x]:
        n = 1 << k
        vk = verifier.VerifyingKey(eng, verifier.encode_vk(shape(k), lambda p: p))
        counts = (8, 4, 1, 8, 4, 2, 2, 2)
        slabs = [slab(c, n, 97 * k + i) for i, c in enumerate(counts)]
        d_h = [torch.zeros((3 * n, 32), dtype=torch.uint8, device=dev) for _ in range(2)]
        torch.cuda.synchronize()
        ptrs = [s.data_ptr() for s in slabs]
        for route in (0, 1):
            eng.quotient_configure(route)
            eng.quotient_device(vk, *ptrs, None, *sc, d_h[route].data_ptr())
        eng.synchronize()
        if not torch.equal(d_h[0], d_h[1]):
            sys.exit("k = %d: the two routes differ" % k)
        for rnd in range(3):
            row = []
            for route in (0, 1):
                eng.quotient_configure(route)
                call = lambda: eng.quotient_device(vk, *ptrs, None, *sc, d_h[route].data_ptr())
                t_call = measure(call)
                eng.debug_configure("phases", 1)
                call()
                split = dict(kv.split("=") for kv in eng.last_phases().split())
                eng.debug_configure("phases", 0)
                row += [t_call, float(split.get("inverse", "nan"))]
            print("%4d  %5d | %14.3f %9.3f | %14.3f %9.3f" % (k, rnd, *row))
            sys.stdout.flush()
        eng.quotient_configure(0)
        vk.close()
        del slabs, d_h
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
