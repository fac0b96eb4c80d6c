#!/usr/bin/env python3
"""Timing of h2agg_witness_check: the call, its split by events, the interpreter alone, and each phase's copy bound.

    python tools/witness_check_time.py [--ks 16,20] > profiles/witness_check.txt
    python tools/witness_check_time.py --chunks        (measure build only: the chunked runs against the unchunked one)

The circuit is the honest prover's (tests/quotient_ref.py::circuit_witness, rebuilt here): advice a, b, c; fixed q_m, q_a
(selectors on every third row each) and a table t; one instance column; the gates q_m (a b - c) and q_a (a + b(wX) - c); the
lookup (b, 7 b) in (t, 7 t); a permutation over all seven columns whose cycles are the copies b[i] = t[j] and a[i] = c[j].
The witness satisfies the key: the work of the check does not depend on that, the report does (it is empty).

Method.  h2agg_witness_check is synchronous over host buffers; two warm-up calls (they grow the work memory), then five calls
with the debug key "phases" on: the library brackets its phases with events on the context's stream and h2agg_last_phases
returns them, summed over the chunks and lookups of the call.  Medians of the five.
  wall         wall-clock time of the call: adds the staging of the slabs (7 x 32 B per row) and of the mapping (7 x 8 B per
               row), the host's range scan of the mapping and the synchronisation
  gates        k_qe_eval<true> over the two gate polynomials
  permutation  k_wc_permutation over the seven columns
  lookups      two k_qe_eval<false> folds, the radix sort of the u folded table rows, k_wc_lookup
  report       k_wc_tile_count, k_wc_line, k_wc_place after each of the three, and k_wc_total
  eval         h2agg_vk_expressions_eval_device(which = 0, fold = y) over the same slabs, resident, two events around one call,
               median of five brackets: the same interpreter work with a folded column as its result instead of flags
Copy bounds: the bytes a phase has to move at 32 B per read, over the rate of a device-to-device copy of a 32 B-per-row
column measured in the same run on the same stream (which moves 64 B per row) — the copy's rate, not the data sheet's.
  gates        8 leaf reads per row (q_m a b c, q_a a b(wX) c): 256 B
  permutation  per cell the mapping's 8 B, the cell's 32 B and its image's 32 B: 7 x 72 B per row (a cell that maps to itself
               reads no image: the bound is an upper one for this traffic)
  lookups      the folds' 4 leaf reads and 2 writes (192 B), the byte histograms' read of the keys (32 B), a read and a write
               per key for each of the 32 passes (2048 B: no byte of a random key is constant), the search's own key and the
               last key it compares with (64 B): 2336 B per row; the other probes of the binary search are not in it
  report       two reads of the flag lines: 10 constraints x 2 x 1 bit per row = 2.5 B per row
"""
import argparse
import ctypes as C
import os
import random
import statistics
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
G1 = (1).to_bytes(32, "little") + (2).to_bytes(32, "little")
BF = 5
BOUND_BYTES = {"gates": 256.0, "permutation": 7 * 72.0, "lookups": 2336.0, "report": 2.5}


def shape(k):
    A, B, Cc, B1 = (("advice", q) for q in range(4))
    QM, QA, T = (("fixed", q) for q in range(3))
    gates = [[("product", QM, ("sum", ("product", A, B), ("neg", Cc)))], [("product", QA, ("sum", ("sum", A, B1), ("neg", Cc)))]]
    perm = [("advice", 0), ("advice", 1), ("advice", 2), ("fixed", 0), ("fixed", 1), ("fixed", 2), ("instance", 0)]
    return types.SimpleNamespace(
        k=k, num_advice_columns=3, num_instance_columns=1, num_challenges=0, degree=4, blinding_factors=BF,
        advice_column_phase=[0] * 3, challenge_phase=[], advice_queries=[(0, 0), (1, 0), (2, 0), (1, 1)], instance_queries=[(0, 0)],
        fixed_queries=[(0, 0), (1, 0), (2, 0)], permutation_columns=perm, fixed_commitments=[G1] * 3, permutation_commitments=[G1] * 7,
        vk_scalar=1, gates=gates, lookups=[([B, ("scaled", B, 7)], [T, ("scaled", T, 7)])])


def witness(k, seed):
    """-> (advice, fixed, instance: lists of columns of integers, copies)"""
    rng = random.Random(seed)
    n = 1 << k
    u = n - BF - 1
    rnd = lambda: rng.getrandbits(253)
    t = [rnd() for _ in range(n)]
    src = [rng.randrange(u) for _ in range(n)]
    b = [t[src[i]] if i < u else rnd() for i in range(n)]
    q_m = [int(i < u and i % 3 == 0) for i in range(n)]
    q_a = [int(i < u and i % 3 == 1) for i in range(n)]
    a, c = [0] * n, [0] * n
    copies = [(1, i, 5, src[i]) for i in range(u)]
    for i in range(n):
        if 0 < i < u and rng.getrandbits(1):
            j = rng.randrange(i)
            a[i] = c[j]
            copies.append((0, i, 2, j))
        else:
            a[i] = rnd()
        c[i] = a[i] * b[i] % R if q_m[i] else (a[i] + b[(i + 1) % n]) % R if q_a[i] else rnd()
    inst = [a[i] if i < 4 else 0 for i in range(n)]
    copies += [(6, i, 0, i) for i in range(4)]
    return [a, b, c], [q_m, q_a, t], [inst], copies


def enc(cols):
    return b"".join(x.to_bytes(32, "little") for col in cols for x in col)


def phases_of(line):
    return {k: float(v) for k, v in (item.split("=") for item in line.split())}


class Check:
    """one key, one witness, the buffers of the call allocated once"""

    def __init__(self, pkg, eng, verifier, k, seed):
        self.eng, self.k, self.n = eng, k, 1 << k
        self.vk = verifier.VerifyingKey(eng, verifier.encode_vk(shape(k), lambda p: p))
        advice, fixed, instance, copies = witness(k, seed)
        self.cols = (advice, fixed, instance)
        self.mapping = pkg.permutation_assembly(7, k, self.n - BF - 1, copies)
        self.theta = (0x7E7A + k).to_bytes(32, "little")
        self.ncons = 10
        self.max_rows = 16
        self.counts, self.first = (C.c_uint32 * self.ncons)(), (C.c_uint32 * self.ncons)()
        self.rows = (C.c_uint32 * (self.ncons * self.max_rows))()
        self.total = C.c_uint64()
        self.stage()

    def stage(self):
        self.slabs = [enc(cols) for cols in self.cols]

    def call(self):
        e = self.eng
        e._check(e._lib.h2agg_witness_check(e._ctx, self.vk._vk, 7, *self.slabs, None, self.theta, self.mapping, self.max_rows,
                                            self.counts, self.first, self.rows, C.byref(self.total)))
        return list(self.counts), list(self.first), list(self.rows), self.total.value


def chunks(pkg, eng, verifier):
    """the report of a broken witness at k = 12 under flag-word bounds that cut the gates and the permutation columns into
    chunks of 1, 2, 3 and 5 constraints, against the report under the product's bound"""
    try:
        eng.debug_configure("lean_acc", 0)
        eng.debug_configure("lean_acc", 1)
    except pkg.H2AggError:
        print("this is the product build: it reads no H2AGG_WC_FLAG_WORDS (build_ext.py --measure)")
        return 1
    chk = Check(pkg, eng, verifier, 12, 12)
    n = chk.n
    for row in (0, 63, 64, 2047, 2048, n - BF - 2):
        chk.cols[0][1][row] = (1 << 200) + row              # b leaves the table: gates, copies and the lookup fail
    chk.stage()
    os.environ.pop("H2AGG_WC_FLAG_WORDS", None)
    want = chk.call()
    assert want[3] > 0 and sum(1 for c in want[0] if c) >= 5, want[0]
    print("# k = 12, counts under the product's bound: %s, total %d" % (want[0], want[3]))
    zwords = n // 32
    for per_chunk in (1, 2, 3, 5):
        os.environ["H2AGG_WC_FLAG_WORDS"] = str(per_chunk * zwords)
        got = chk.call()
        print("chunks of %d constraints: %s" % (per_chunk, "the same report" if got == want else "DIFFERENT: %r" % (got,)))
        if got != want:
            return 1
    os.environ.pop("H2AGG_WC_FLAG_WORDS", None)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="16,20")
    ap.add_argument("--chunks", action="store_true")
    args = ap.parse_args()
    import importlib
    import torch
    pkg = entry.load_package()
    verifier = importlib.import_module(entry.PKG_NAME + ".verifier")
    eng = pkg.H2Agg(0)
    if args.chunks:
        sys.exit(chunks(pkg, eng, verifier))
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    eng.set_stream(stream.cuda_stream)
    print("# %s" % eng.describe())
    print("# h2agg_witness_check, the honest prover's circuit (2 gate polynomials, 7 permutation columns, 1 lookup), max_rows = 16;")
    print("# two warm-up calls, medians of 5 calls; times in ms; bound: the phase's copy bound, x: the phase over its bound")
    print("#  k       wall |     gates    bound      x | permutation    bound      x |   lookups    bound      x |    report    bound      x |"
          "  eval(fold)   column copy")
    for k in [int(x) for x in args.ks.split(",") if x]:
        n = 1 << k
        chk = Check(pkg, eng, verifier, k, k)
        assert chk.call()[3] == 0, "the witness satisfies the key"
        chk.call()
        eng.debug_configure("phases", 1)
        walls, rows = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            chk.call()
            walls.append((time.perf_counter() - t0) * 1e3)
            rows.append(phases_of(eng.last_phases()))
        eng.debug_configure("phases", 0)
        med = {name: statistics.median(r[name] for r in rows) for name in BOUND_BYTES}
        d = [torch.frombuffer(bytearray(s), dtype=torch.uint8).to(dev) for s in chk.slabs]
        d_out = torch.empty(32 * n, dtype=torch.uint8, device=dev)
        d_b = torch.empty_like(d_out)
        torch.cuda.synchronize()

        def bracket(f, reps=1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record(stream)
                for _ in range(reps):
                    f()
                e1.record(stream)
            eng.synchronize()
            e1.synchronize()
            return e0.elapsed_time(e1) / reps

        y = (0x1234567).to_bytes(32, "little")
        ev = lambda: eng.vk_expressions_eval_device(chk.vk, 0, 0, k, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), None, y,
                                                    d_out.data_ptr())
        bracket(ev, 2)
        t_eval = statistics.median(bracket(ev) for _ in range(5))
        cp = lambda: d_b.copy_(d_out)
        bracket(cp, 10)
        t_copy = statistics.median(bracket(cp, 10) for _ in range(5))
        per_byte = t_copy / (64.0 * n)                         # ms per byte moved
        line = "%4d  %9.3f |" % (k, statistics.median(walls))
        for name in ("gates", "permutation", "lookups", "report"):
            bound = BOUND_BYTES[name] * n * per_byte
            line += " %9.4f %8.4f %6.1f |" % (med[name], bound, med[name] / bound)
        print(line + "  %10.4f    %10.4f" % (t_eval, t_copy))
        sys.stdout.flush()
        chk.vk.close()
        del d, d_out, d_b, chk
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
