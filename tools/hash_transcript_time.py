#!/usr/bin/env python3
"""Timing of the ShaRead transcript family on the GPU box (profiles/hash_transcript.txt).

    python tools/hash_transcript_time.py [--max N] [--reps R]

1. host / device crossover of h2agg_hash_transcript_read_batch: the outer-proof-like script of the bench's P = 347 shape
   (synthetic.CircuitShape(10, 300)), batch sizes 1 .. N (default 4096; 16384 needs ~0.5 GB of proof bytes and ~0.9 GB of message
   streams), both digests, both backends, best of R calls each (uploads and downloads included: that is what a caller pays).
2. h2agg_verify_proofs at 4 / 16 / 64 such proofs written for SHA-256 against the same shape written for Poseidon.
The transcripts are well-formed random bytes (every point on the curve, every scalar canonical), not proofs: the pairing
rejects them, the cost is the same."""
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def outer_script(shape):
    n_pts, n_evals, n_w = shape.proof_items()
    nl = len(shape.lookups)
    return ("C" + "X" * shape.num_instance_columns + "P" * shape.num_advice_columns + "Q" + "PP" * nl + "QQ" + "P" * shape.n_sets +
            "P" * nl + "P" + "Q" + "P" * (shape.degree - 1) + "Q" + "S" * n_evals + "Q" + "P" * n_w + "QQ")


def best(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return min(ts) * 1e3


def main():
    nmax = int(sys.argv[sys.argv.index("--max") + 1]) if "--max" in sys.argv else 4096
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
    pkg = entry.load_package()
    syn = importlib.import_module(entry.PKG_NAME + ".synthetic")
    ver = importlib.import_module(entry.PKG_NAME + ".verifier")
    eng = pkg.H2Agg(0)
    print(eng.describe(), "| host threads:", pkg.host_threads())
    pool = syn.point_pool(eng, 0xA66)
    shape = syn.CircuitShape(10, 300, pool)
    script = outer_script(shape)
    base = [shape.random_transcript(pool, 500 + i) for i in range(64)]
    consts = shape.vk_scalar.to_bytes(32, "little")
    print("script: %d P, %d S, %d Q; %d bytes per proof" % (script.count("P"), script.count("S"), script.count("Q"), len(base[0])))
    print("\n# 1. h2agg_hash_transcript_read_batch, ms per call (best of %d)" % reps)
    print("%-10s %7s %12s %12s %10s" % ("digest", "proofs", "host", "device", "dev/host"))
    for kind in ("sha256", "keccak256"):
        n = 1
        while n <= nmax:
            proofs = [base[i % 64] for i in range(n)]
            ext = b"".join(pool[i % len(pool)] for i in range(n))
            ms = {}
            for backend in ("host", "device"):
                eng.transcript_configure(backend)
                ms[backend] = best(lambda: eng.hash_transcript_read_batch(kind, proofs, script, consts, ext), reps)
            print("%-10s %7d %12.3f %12.3f %10.2f" % (kind, n, ms["host"], ms["device"], ms["device"] / ms["host"]), flush=True)
            n *= 4
    eng.transcript_configure("auto")
    print("\n# 2. h2agg_verify_proofs (no pairing), ms per call (best of %d): the shape written for SHA-256 / Poseidon" % reps)
    comp = eng.g1_batch_compress(b"".join(pool))
    pool_c = [comp[32 * i:32 * i + 32] for i in range(len(pool))]
    table = eng.bases_upload(b"".join(pool[i % len(pool)] for i in range(1 << 10)))
    blob = ver.encode_vk(shape, lambda p: p)
    fr = syn.fr_stream(0xBEEF)
    inst = [b"".join(fr() for _ in range(64))]
    print("%7s %12s %12s" % ("proofs", "sha256", "poseidon"))
    for n in (4, 16, 64):
        row = []
        for kind, pl in (("sha256", pool), ("poseidon", pool_c)):
            vk = ver.VerifyingKey(eng, blob, transcript=kind)
            arg = [(vk, "syn", table, [(inst, shape.random_transcript(pl, 500 + i)) for i in range(n)])]
            got = ver.verify_proofs(eng, arg)
            assert [r[2] for r in got] == [0] * n, [r[2] for r in got]
            row.append(best(lambda: ver.verify_proofs(eng, arg), reps))
            vk.close()
        print("%7d %12.3f %12.3f" % (n, row[0], row[1]), flush=True)
    eng.bases_free(table)
    eng.close()


if __name__ == "__main__":
    main()
