#!/usr/bin/env python3
"""Timing of h2agg_pk_quotient against the parent commit's h2agg_quotient_device, and of h2agg_pk_create.

    python tools/pk_time.py --parent-lib <the parent commit's libh2agg.so> [--ks 16,18,20] > profiles/pk.txt

The shape of tools/quotient_time.py: 8 advice, 4 fixed and 1 instance column, 6 gate polynomials, 8 permutation columns (four
sets), 2 lookups, degree 4: e = 2, four cosets; 34 input polynomials + 3 Lagrange columns = 37 columns per coset, of which
4 fixed + 8 sigma + 3 Lagrange = 15 are the key's.  Random canonical inputs (the work does not depend on the values).

One process.  The parent commit's library is a second shared object loaded beside this tree's with ctypes (another file,
another set of symbols: dlopen keeps them apart), with a context and a verifying key of its own on the same torch stream.
Per k, first the pieces of the three routes are compared byte for byte; then three alternating rounds of
  parent      h2agg_quotient_device of the parent's library
  pk cosets   h2agg_pk_quotient of a key built with H2AGG_PK_COSETS
  pk lean     h2agg_pk_quotient of a key built without
  create      h2agg_pk_create with H2AGG_PK_COSETS from host slabs (synchronous: wall clock, the object destroyed again)
each the median of five brackets of one call between two events on the stream (after two warm-up calls), and one more call
under the debug key "phases" for the library's own split (events at the stage boundaries, summed over the four cosets)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry
from quotient_time import shape


class Parent:
    """the few entry points of the parent's library this tool calls, with a context of its own"""

    def __init__(self, path, stream_ptr, blob):
        vp, u8p, i32 = C.c_void_p, C.c_char_p, C.c_int
        lib = self.lib = C.CDLL(path)
        for name, res, args in (("h2agg_create", i32, [i32, C.POINTER(vp)]), ("h2agg_destroy", None, [vp]),
                                ("h2agg_set_stream", i32, [vp, vp]), ("h2agg_synchronize", i32, [vp]),
                                ("h2agg_last_error", C.c_char_p, [vp]), ("h2agg_vk_create", i32, [vp, u8p, C.c_size_t, C.POINTER(vp)]),
                                ("h2agg_vk_destroy", None, [vp]), ("h2agg_debug_configure", i32, [vp, C.c_char_p, i32]),
                                ("h2agg_last_phases", C.c_char_p, [vp]),
                                ("h2agg_quotient_device", i32, [vp] * 10 + [u8p] * 6 + [vp])):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        if hasattr(lib, "h2agg_pk_quotient"):
            sys.exit("%s has h2agg_pk_quotient: it is not the parent commit's library" % path)
        self.ctx, self.vk = vp(), vp()
        self.check(lib.h2agg_create(0, C.byref(self.ctx)))
        self.check(lib.h2agg_set_stream(self.ctx, stream_ptr))
        self.check(lib.h2agg_vk_create(self.ctx, blob, len(blob), C.byref(self.vk)))

    def check(self, rc):
        if rc:
            sys.exit("parent library: status %d: %s" % (rc, (self.lib.h2agg_last_error(self.ctx) or b"").decode()))

    def quotient(self, ptrs, sc, d_h):
        self.check(self.lib.h2agg_quotient_device(self.ctx, self.vk, *ptrs, None, *sc, d_h))

    def synchronize(self):
        self.check(self.lib.h2agg_synchronize(self.ctx))

    def phases(self, call):
        self.check(self.lib.h2agg_debug_configure(self.ctx, b"phases", 1))
        call()
        line = (self.lib.h2agg_last_phases(self.ctx) or b"").decode()
        self.check(self.lib.h2agg_debug_configure(self.ctx, b"phases", 0))
        return line

    def close(self):
        self.lib.h2agg_vk_destroy(self.vk)
        self.lib.h2agg_destroy(self.ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libh2agg.so built from the parent commit")
    ap.add_argument("--ks", default="16,18,20")
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

    def bracket(f, sync):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            f()
            e1.record(stream)
        sync()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def measure(f, sync):
        f()
        f()
        sync()
        return statistics.median(bracket(f, sync) for _ in range(5))

    def slab(ncols, n, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        d = torch.randint(0, 256, (ncols * n, 32), dtype=torch.uint8, generator=g)
        d[:, 31] = (d[:, 31] & 0x0F) | 0x20            # 254 bits, below r
        return d

    sc = [(0x1234567 + 0x1111 * i).to_bytes(32, "little") for i in range(5)]
    print("# %s" % eng.describe())
    print("# 8 advice, 4 fixed, 1 instance, 6 gate polynomials, 8 permutation columns, 2 lookups, degree 4: 4 cosets; 37 columns per")
    print("# coset, 15 of them the key's.  One call per bracket, median of 5 brackets; phases from the library's own events; ms")
    print("#  k  round  route      |   call ms | forward    gates  permutation  lookups  inverse")
    for k in [int(x) for x in args.ks.split(",") if x]:
        n = 1 << k
        blob = verifier.encode_vk(shape(k), lambda p: p)
        vk = verifier.VerifyingKey(eng, blob)
        parent = Parent(args.parent_lib, stream.cuda_stream, blob)
        counts = (8, 4, 1, 8, 4, 2, 2, 2)                 # advice, fixed, instance, sigma, perm_z, lookup z / a' / s'
        host = [slab(c, n, 97 * k + i) for i, c in enumerate(counts)]
        slabs = [h.to(dev) for h in host]
        ptrs = [s.data_ptr() for s in slabs]
        witness = [ptrs[i] for i in (0, 2, 4, 5, 6, 7)]
        # the key takes Lagrange columns: the transforms of the coefficient slabs the parent's call is given
        lag = [torch.empty_like(slabs[i]) for i in (1, 3)]
        torch.cuda.synchronize()
        for t, i in zip(lag, (1, 3)):
            for c in range(counts[i]):
                eng.fr_fft_device(ptrs[i] + 32 * n * c, k, False, None, t.data_ptr() + 32 * n * c)
        eng.synchronize()
        fixed_lag, sigma_lag = (bytes(t.cpu().numpy()) for t in lag)
        keys = {"pk cosets": eng.pk_create(vk, fixed_lag, sigma_lag, pkg.PK_COSETS), "pk lean": eng.pk_create(vk, fixed_lag, sigma_lag, 0)}
        d_h = {name: torch.zeros((3 * n, 32), dtype=torch.uint8, device=dev) for name in ("parent", "pk cosets", "pk lean")}
        torch.cuda.synchronize()
        calls = {"parent": (lambda: parent.quotient(ptrs, sc, d_h["parent"].data_ptr()), parent.synchronize)}
        for name in keys:
            calls[name] = (lambda name=name: eng.pk_quotient(keys[name], *witness, None, *sc, d_h[name].data_ptr()), eng.synchronize)
        for name, (call, sync) in calls.items():
            call()
            sync()
        for name in keys:
            if not torch.equal(d_h[name], d_h["parent"]):
                sys.exit("k = %d: the pieces of '%s' differ from the parent's" % (k, name))
        print("# k = %d: the pieces of the three routes are equal byte for byte; h2agg_pk_bytes %d (cosets) / %d (lean); work memory %d / %d"
              " (h2agg_quotient_work_bytes %d)" % (k, eng.pk_bytes(vk, pkg.PK_COSETS), eng.pk_bytes(vk, 0),
                                                   eng.pk_quotient_work_bytes(keys["pk cosets"]),
                                                   eng.pk_quotient_work_bytes(keys["pk lean"]), eng.quotient_work_bytes(vk)))
        for rnd in range(3):
            for name, (call, sync) in calls.items():
                t_call = measure(call, sync)
                if name == "parent":
                    line = parent.phases(call)
                else:
                    eng.debug_configure("phases", 1)
                    call()
                    line = eng.last_phases()
                    eng.debug_configure("phases", 0)
                split = dict(kv.split("=") for kv in line.split())
                print("%4d  %5d  %-10s | %9.3f | %7s %8s %12s %8s %8s" % (
                    k, rnd, name, t_call, split.get("forward", "-"), split.get("gates", "-"), split.get("permutation", "-"),
                    split.get("lookups", "-"), split.get("inverse", "-")))
            walls = []
            for _ in range(3):
                t0 = time.perf_counter()
                h = eng.pk_create(vk, fixed_lag, sigma_lag, pkg.PK_COSETS)
                walls.append(1e3 * (time.perf_counter() - t0))
                eng.pk_destroy(h)
            print("%4d  %5d  %-10s | %9.3f |   (wall clock, host slabs in, every form complete; median of 3)" % (
                k, rnd, "create", statistics.median(walls)))
            sys.stdout.flush()
        for h in keys.values():
            eng.pk_destroy(h)
        parent.close()
        vk.close()
        del slabs, lag, d_h, host
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
