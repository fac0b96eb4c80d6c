#!/usr/bin/env python3
"""Per-proof verification against the aggregation, on the bench's synthetic EVM-like proofs (bench.py full_pipeline_leg's
shape: P = 347 queries, 3 permutation sets, a lookup, 64 public inputs per proof).  For N = 1, 4, 16, 64 proofs, p50 / p95 of
  (a) h2agg_verify_proofs            every proof's own pair and pairing verdict, one call
  (b) h2agg_verify_aggregation       the same proofs folded with lambda, one pairing
  (c) N one-proof h2agg_verify_aggregation calls   what a caller had to do before (a) to find a bad proof
and the split of (a) by phase (h2agg_last_phases: "evaluate" is the tape + segmented multi_exp + tails, "pairing" the N
checks on the host pool), plus the segmented multi_exp alone (h2agg_g1_msm_segmented over the 2N side sizes of the batch,
host round trip included; a `rocprofv3 --kernel-trace --stats` run of this tool gives the kernels' device time).
--seg-c sweeps the window width.  Prints one JSON line."""
import argparse
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

G2 = bytes.fromhex(
    "edf692d95cbdde46ddda5ef7d422436779445c5e66006a42761e1f12efde0018c212f3aeb785e49712e7a9353349aaf1255dfb31b7bf60723a480d9293938e19"
    "aa7dfa6601cce64c7bd3430c69e7d1e38f40cb8d8071ab4aeb6d8cdba55ec8125b9722d1dcdaac55f38eb37033314bbc95330c69ad999eec75f05f58d0890609")


def pct(ts, q):
    s = sorted(ts)
    return round(1e3 * s[min(len(s) - 1, int(q * (len(s) - 1) + 0.5))], 3)


def phase_medians(lines):
    acc = {}
    for ln in lines:
        for tok in ln.split():
            if "=" in tok and not tok.startswith("["):
                k, v = tok.split("=", 1)
                try:
                    acc.setdefault(k, []).append(float(v))
                except ValueError:
                    pass
    return {k: round(sorted(v)[len(v) // 2], 3) for k, v in acc.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,4,16,64")
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--instance-log2", type=int, default=17)
    ap.add_argument("--seg-c", default="6", help="window widths of the segmented multi_exp to time (comma list, 4..8)")
    ap.add_argument("--only-each", type=int, default=0, help="time (a) only, at this N (for a rocprofv3 kernel trace)")
    args = ap.parse_args()
    pkg = entry.load_package()
    syn = importlib.import_module(entry.PKG_NAME + ".synthetic")
    ver = importlib.import_module(entry.PKG_NAME + ".verifier")
    eng = pkg.H2Agg(0)
    pool = syn.point_pool(eng, 0xA66)
    comp = eng.g1_batch_compress(b"".join(pool))
    pool_c = [comp[32 * i:32 * i + 32] for i in range(len(pool))]
    shape = syn.CircuitShape(args.instance_log2, 300, pool)
    vk = ver.VerifyingKey(eng, ver.encode_vk(shape, lambda p: p))
    table = eng.bases_upload(b"".join(pool[i % len(pool)] for i in range(1 << args.instance_log2)))
    fr = syn.fr_stream(0xF00D)
    sizes = [args.only_each] if args.only_each else [int(x) for x in args.sizes.split(",")]
    nmax = max(sizes)
    proofs = [([b"".join(fr() for _ in range(64))], shape.random_transcript(pool_c, 100 + i)) for i in range(nmax)]
    eng.debug_configure("phases", 1)
    out = {"tool": "verify_each_time", "shape": "bench full_pipeline_leg (P = 347)", "instance_log2": args.instance_log2,
           "host_threads": eng._lib.h2agg_host_threads(), "sizes": {}}

    def timed(fn, reps):
        fn()
        ts, ph = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
            ph.append(eng.last_phases())
        return ts, ph

    for n in sizes:
        arg = [(vk, "syn", table, proofs[:n])]
        rec = {}
        ts, ph = timed(lambda: ver.verify_proofs(eng, arg, G2, G2), args.reps)
        rec["a_verify_proofs_ms"] = {"p50": pct(ts, 0.5), "p95": pct(ts, 0.95), "phases_p50": phase_medians(ph)}
        if not args.only_each:
            ts, ph = timed(lambda: ver.verify_aggregation(eng, arg, G2, G2), args.reps)
            rec["b_verify_aggregation_ms"] = {"p50": pct(ts, 0.5), "p95": pct(ts, 0.95), "phases_p50": phase_medians(ph)}
            ones = [[(vk, "syn", table, [p])] for p in proofs[:n]]
            ts, _ph = timed(lambda: [ver.verify_aggregation(eng, a, G2, G2) for a in ones], max(3, args.reps // 4))
            rec["c_one_proof_aggregations_ms"] = {"p50": pct(ts, 0.5), "p95": pct(ts, 0.95)}
            rec["a_over_b"] = round(rec["a_verify_proofs_ms"]["p50"] / rec["b_verify_aggregation_ms"]["p50"], 2)
            rec["c_over_a"] = round(rec["c_one_proof_aggregations_ms"]["p50"] / rec["a_verify_proofs_ms"]["p50"], 2)
        out["sizes"][str(n)] = rec
    # the segmented multi_exp alone, over side sizes of this shape (w_x ~ 1 W per rotation group, w_g every commitment)
    if not args.only_each:
        n = nmax
        lens = [30, 347] * n
        tot = sum(lens)
        bases = b"".join(pool[i % len(pool)] for i in range(tot))
        scal = b"".join(fr() for _ in range(tot))
        seg = {}
        for c in [int(x) for x in args.seg_c.split(",")]:
            eng.debug_configure("seg_c", c)
            ts, _ph = timed(lambda: eng.g1_msm_segmented(bases, scal, lens), args.reps)
            seg[str(c)] = {"p50": pct(ts, 0.5), "p95": pct(ts, 0.95)}
        eng.debug_configure("seg_c", 0)
        out["segmented_msm_ms"] = {"segments": len(lens), "points": tot, "by_window_bits": seg}
    eng.debug_configure("phases", 0)
    vk.close()
    eng.bases_free(table)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
