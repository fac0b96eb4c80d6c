#!/usr/bin/env python3
"""Timing of the batched lookup calls (h2agg_lookup_store_permute + h2agg_lookup_store_product) against the loop of single
calls of a library built from the PARENT commit, alternated in one process.

    python tools/lookup_batch_time.py --parent <parent libh2agg.so> [--ks 12,16,20] [--ls 4,16,64] > profiles/lookup_batch.txt

Method (that of tools/lookup_permute_time.py).  Every column is resident: this branch's library keeps a, s, ap, sp, z of all
L lookups in ONE column store; the parent's context gets device pointers to columns of the same size (torch tensors holding the
same bytes).  Both contexts run on one stream of the caller.  A leg is one pass over all L lookups, queued with no
synchronisation and no read-back:
  batch   h2agg_lookup_store_permute(status = NULL), h2agg_lookup_store_product(last = NULL): two calls
  loop    L x (h2agg_lookup_permute_device, h2agg_lookup_product_device) through the parent's library
Two events on the stream bracket REPS legs queued back to back; two warm-up legs per library first (they grow the work
memory).  The legs ALTERNATE — loop, batch, loop, batch, loop, batch — and every run is printed: the spread of the parent's
three runs is the yardstick a difference has to beat.  ratio = median loop / median batch.  u = 2^k - 6.  A size with
L u > 2^24 runs in several chunks (64 lookups at k = 20: four chunks of 16); the chunks column says how many.  Two inputs,
the input columns drawn from their tables' usable rows:
  random   254-bit table values: all 32 byte passes of both sorts move
  16-bit   table values below 2^16: two passes of each sort move, thirty return at their first instruction
With the debug key phases the batch's split (sort / rank, terms / invert / scan; milliseconds of one leg) is printed from one
more leg behind the timed ones.

Launches per leg, from the host code (csrc/lookup.inc, csrc/prod.inc; S = the sweep launches of a running product over u + 1
positions, I = those of an inversion over the elements given: 1 up to 2^11, 3 up to 2^22, 5 above):
  loop    L x (2 x (memset + 2 + 96) + memset + 9  +  1 + I(u) + S)
  batch   per chunk: (memset + 2 + 96) + memset + 9  +  1 + I(B u) + S      — a function of the chunks, not of L
The outputs of the two legs are compared byte for byte once per size; a mismatch ends the run with an error.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry

REPS = 5


def sweeps(n, t=11):
    """launches of one sweep pair over n elements: 1, 3, 5 (prod_kernels.hpp)"""
    levels = 0
    while True:
        n = (n + (1 << t) - 1) >> t
        levels += 1
        if n <= 1:
            return 2 * levels - 1


def chunks_of(L, u):
    """the lookups of every chunk (csrc/lookup.inc lk_batch_chunk, default configuration)"""
    B = min(max((1 << 24) // max(u, 1), 1), 1024)
    return [min(B, L - j) for j in range(0, L, B)]


def launches(L, u, batched):
    per_sort = 1 + 2 + 96
    if batched:
        return sum(per_sort + 1 + 9 + 1 + sweeps(nb * u) + sweeps(u + 1) for nb in chunks_of(L, u))
    return L * (2 * per_sort + 1 + 9 + 1 + sweeps(u) + sweeps(u + 1))


class Parent:
    """the few entry points of the parent's library this tool calls"""

    def __init__(self, path, stream):
        lib = self.lib = C.CDLL(path)
        vp, sz, u8p = C.c_void_p, C.c_size_t, C.c_char_p
        lib.h2agg_create.argtypes = [C.c_int, C.POINTER(vp)]
        lib.h2agg_set_stream.argtypes = [vp, vp]
        lib.h2agg_synchronize.argtypes = [vp]
        lib.h2agg_destroy.argtypes = [vp]
        lib.h2agg_destroy.restype = None
        lib.h2agg_lookup_permute_device.argtypes = [vp, vp, vp, C.c_uint, sz, vp, vp]
        lib.h2agg_lookup_product_device.argtypes = [vp, vp, vp, vp, vp, C.c_uint, sz, u8p, u8p, vp, vp]
        self.ctx = vp()
        self.check(lib.h2agg_create(0, C.byref(self.ctx)))
        self.check(lib.h2agg_set_stream(self.ctx, stream))

    @staticmethod
    def check(rc):
        if rc:
            sys.exit("the parent's library answered %d" % rc)

    def synchronize(self):
        self.check(self.lib.h2agg_synchronize(self.ctx))

    def close(self):
        self.lib.h2agg_destroy(self.ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--ks", default="12,16,20")
    ap.add_argument("--ls", default="4,16,64")
    args = ap.parse_args()
    import torch
    pkg = entry.load_package()
    poly = __import__("importlib").import_module(entry.PKG_NAME + ".poly")
    eng = pkg.H2Agg(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    eng.set_stream(stream.cuda_stream)
    parent = Parent(args.parent, stream.cuda_stream)
    beta, gamma = (0x1234567 * 0x89ABCDEF0123).to_bytes(32, "little"), (0xFEDCBA987 * 0x13579BDF).to_bytes(32, "little")

    def bracket(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            for _ in range(REPS):
                f()
            e1.record(stream)
        eng.synchronize()
        parent.synchronize()
        e1.synchronize()
        return e0.elapsed_time(e1) / REPS

    def tables(kind, L, n, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        s = torch.randint(0, 256, (L, n, 32), dtype=torch.uint8, generator=g)
        if kind == "random":
            s[:, :, 31] = (s[:, :, 31] & 0x0F) | 0x20    # 254 bits, below r
        else:
            s[:, :, 2:] = 0
        rows = torch.randint(0, n - 6, (L, n), generator=g)
        a = torch.stack([s[j][rows[j]] for j in range(L)])
        return a.contiguous(), s

    print("# %s" % eng.describe())
    print("# %d legs per bracket, three alternating brackets per leg; u = 2^k - 6; times in ms per leg (all L lookups)" % REPS)
    print("#  k    L  chunks input    launches loop / batch | loop (parent) runs        | batch runs                | ratio   spread of loop")
    for k in [int(x) for x in args.ks.split(",") if x]:
        n, u = 1 << k, (1 << k) - 6
        for L in [int(x) for x in args.ls.split(",") if x]:
            for kind in ("random", "16-bit"):
                a_h, s_h = tables(kind, L, n, 131 * k + L + len(kind))
                col = 32 * n
                with poly.ColumnStore(eng, 5 * L, k) as st:
                    st.write(0, bytes(a_h.numpy().tobytes()))
                    st.write(L, bytes(s_h.numpy().tobytes()))
                    d_a, d_s = a_h.to(dev), s_h.to(dev)
                    d_out = torch.zeros((3, L, n, 32), dtype=torch.uint8, device=dev)
                    torch.cuda.synchronize()
                    h = st.handle

                    def batch():
                        eng.lookup_store_permute(h, 0, h, L, L, u, h, 2 * L, h, 3 * L, False)
                        eng.lookup_store_product(h, 0, h, L, h, 2 * L, h, 3 * L, L, u, beta, gamma, h, 4 * L, False)

                    def loop():
                        lib, ctx = parent.lib, parent.ctx
                        pa, ps, po = d_a.data_ptr(), d_s.data_ptr(), d_out.data_ptr()
                        for j in range(L):
                            at = col * j
                            lib.h2agg_lookup_permute_device(ctx, pa + at, ps + at, k, u, po + at, po + L * col + at)
                            lib.h2agg_lookup_product_device(ctx, pa + at, ps + at, po + at, po + L * col + at, k, u, beta, gamma,
                                                            po + 2 * L * col + at, None)

                    for f in (loop, batch, loop, batch):
                        f()
                    eng.synchronize()
                    parent.synchronize()
                    for i in range(3 * L):
                        rows = u + 1 if i >= 2 * L else u
                        got = eng.columns_read(h, 2 * L + i, 1)
                        want = bytes(d_out[i // L, i % L].cpu().numpy().tobytes())
                        if got[:32 * rows] != want[:32 * rows]:
                            sys.exit("k = %d, L = %d, %s: column %d of the batch differs from the parent's loop" % (k, L, kind, i))
                    t_loop, t_batch = [], []
                    for _ in range(3):
                        t_loop.append(bracket(loop))
                        t_batch.append(bracket(batch))
                    eng.debug_configure("phases", 1)
                    eng.lookup_store_permute(h, 0, h, L, L, u, h, 2 * L, h, 3 * L, False)
                    split = eng.last_phases()
                    eng.lookup_store_product(h, 0, h, L, h, 2 * L, h, 3 * L, L, u, beta, gamma, h, 4 * L, False)
                    split += eng.last_phases()
                    eng.debug_configure("phases", 0)
                    eng.synchronize()
                    ml, mb = statistics.median(t_loop), statistics.median(t_batch)
                    print("%4d %4d  %4d   %-7s %8d / %-5d | %s | %s | %5.2f   %.3f    #%s" % (
                        k, L, len(chunks_of(L, u)), kind, launches(L, u, False), launches(L, u, True), " ".join("%8.3f" % t for t in t_loop),
                        " ".join("%8.3f" % t for t in t_batch), ml / mb, max(t_loop) - min(t_loop), split))
                    sys.stdout.flush()
                del d_a, d_s, d_out
                torch.cuda.empty_cache()
    parent.close()


if __name__ == "__main__":
    main()
