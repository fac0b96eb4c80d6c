#!/usr/bin/env python3
"""Timing of the from-bytes verifier on GWC proofs and on Shplonk proofs of ONE circuit.

    python tools/shplonk_verify_time.py [--legs gwc,shplonk] [--out profiles/shplonk_verify.txt]

Circuit: the first shape of tests/test_verifier_pipeline.py (k = 5, three advice, two fixed and one instance column, two gates,
one lookup, degree 4, four permutation columns: 25 queries at four rotations), proofs by the trapdoor provers of tests/ — the
same body written once with a GWC tail (v, four W, u: tests/toy_prover_hash.py over the Poseidon transcript) and once with a
Shplonk tail (y, v, H1, u, H2: tests/toy_prover_shplonk.py).  Every timed call is checked: status 0 and verdict True per proof,
pairing_ok for the aggregation.

  legs     h2agg_verify_proofs and h2agg_verify_aggregation at 4 and at 16 proofs, per kind.
  time     the host clock around CALLS synchronous calls (each ends in the library's own device synchronise and the pairing on
           the host pool), divided by CALLS; one untimed round first, then ROUNDS rounds in which the legs ALTERNATE, so both
           kinds see the same machine at the same time.  Median [min .. max] over the rounds: the spread a difference has to
           exceed.  The aggregation runs with its plan cache on, as a caller has it: the recording is made in the warm-up.
  split    a pass of its own with the debug key phases on (it adds a synchronise per phase, so its sum is not the time above):
           h2agg_last_phases, the median of PHASE_CALLS calls per phase; phases under 1 % of the call are summed as `other`.
  tape     the aggregation recorded afresh (plan_cache 0) with phases on: the trace line's tape size and levels.
--legs gwc runs the GWC legs alone: they use no new entry point, so the same file times an older build of the library."""
import argparse
import importlib
import os
import re
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry
from oracle import bn254 as O
from oracle import poseidon as P
from tests import toy_prover as T
from tests import toy_prover_hash as TH
from tests.test_pairing_capi import g2b
from tests.test_verifier_pipeline import SHAPES

ROUNDS, CALLS, PHASE_CALLS = 5, 20, 5
SIZES = (4, 16)


def spread(xs):
    return "%8.3f [%8.3f .. %8.3f]" % (statistics.median(xs), min(xs), max(xs))


def phases_of(line):
    d = {}
    for tok in re.sub(r"\[[^\]]*\]", " ", line).split():      # (the bracketed trace notes are not phases)
        if "=" in tok:
            name, ms = tok.split("=")
            d[name] = d.get(name, 0.0) + float(ms)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="gwc,shplonk")
    ap.add_argument("--out", default=os.path.join(entry.ROOT, "profiles", "shplonk_verify.txt"))
    a = ap.parse_args()
    kinds = [k for k in a.legs.split(",") if k]
    pkg = entry.load_package()
    ver = importlib.import_module(entry.PKG_NAME + ".verifier")
    eng = pkg.H2Agg(0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    # ---- one circuit, max(SIZES) proofs of each kind (seeded: the GWC proofs are the same in every run)
    rng = O.SplitMix64(0x5E71F)
    dlogs = {}
    setup = T.Setup(5, rng.fr(), 16)
    cs = T.make_constraint_system(rng, dlogs=dlogs, **SHAPES[0])
    table = eng.bases_upload(b"".join(O.aff_to_bytes(p) for p in setup.g_lagrange))
    g2 = (g2b(setup.s_g2), g2b(setup.g2))
    blob = ver.encode_vk(cs, O.aff_to_bytes)
    proofs, vks = {}, {}
    for kind in kinds:
        prng = O.SplitMix64(0xA000 + len(kind))
        if kind == "gwc":
            prove = lambda *args: TH.prove(*args, P.PoseidonTranscriptWrite, P.PoseidonTranscriptRead)
            vks[kind] = ver.VerifyingKey(eng, blob)
        else:
            from tests import toy_prover_shplonk as TS
            prove = TS.prove
            vks[kind] = ver.VerifyingKey(eng, blob, multiopen="shplonk")
        rows = []
        for i in range(max(SIZES)):
            inst = [[[prng.fr() for _ in range(3 + col)] for col in range(cs.num_instance_columns)]]
            data = prove(cs, setup, prng, inst, dlogs, "circuit0_p%d" % i)
            rows.append(([b"".join(O.fe_to_bytes(v) for v in col) for col in inst[0]], data))
        proofs[kind] = rows

    def arg(kind, n):
        return [(vks[kind], "circuit0", table, proofs[kind][:n])]

    def call(leg):
        kind, what, n = leg
        if what == "proofs":
            got = ver.verify_proofs(eng, arg(kind, n), *g2)
            assert all(r[2] == 0 and r[3] is True for r in got), leg
        else:
            got = ver.verify_aggregation(eng, arg(kind, n), *g2)
            assert got[3] is True, leg

    legs = [(kind, what, n) for n in SIZES for what in ("proofs", "aggregation") for kind in kinds]
    times = {leg: [] for leg in legs}
    for r in range(ROUNDS + 1):                   # the first round warms up (and records the aggregations)
        for leg in legs:
            t0 = time.perf_counter()
            for _ in range(CALLS):
                call(leg)
            if r:
                times[leg].append((time.perf_counter() - t0) * 1e3 / CALLS)

    say("# %s" % eng.describe())
    say("# one circuit (k = 5, %d-byte GWC proofs%s), trapdoor proofs; %d rounds of %d calls per leg, legs alternating; ms per call, "
        "median [min .. max]" % (len(proofs["gwc"][0][1]) if "gwc" in proofs else 0,
                                 ", %d-byte Shplonk proofs" % len(proofs["shplonk"][0][1]) if "shplonk" in proofs else "", ROUNDS, CALLS))
    for n in SIZES:
        for what in ("proofs", "aggregation"):
            for kind in kinds:
                say("%2d proofs  h2agg_verify_%-11s %-7s %s" % (n, what, kind, spread(times[(kind, what, n)])))

    # ---- the split, and the recordings' tapes
    eng.debug_configure("phases", 1)
    try:
        say("# split (debug key phases on: a synchronise per phase), median of %d calls, ms" % PHASE_CALLS)
        for leg in legs:
            kind, what, n = leg
            rows = []
            for _ in range(PHASE_CALLS):
                call(leg)
                rows.append(phases_of(eng.last_phases()))
            med = {name: statistics.median([row.get(name, 0.0) for row in rows]) for name in rows[0]}
            total = sum(med.values())
            shown = ["%s %.3f" % (name, ms) for name, ms in med.items() if ms >= 0.01 * total]
            other = sum(ms for ms in med.values() if ms < 0.01 * total)
            say("%2d proofs  %-11s %-7s sum %.3f: %s, other %.3f" % (n, what, kind, total, ", ".join(shown), other))
        eng.debug_configure("plan_cache", 0)
        say("# the aggregation recorded afresh (plan_cache 0)")
        for n in SIZES:
            for kind in kinds:
                call((kind, "aggregation", n))
                line = eng.last_phases()
                say("%2d proofs  %-7s %s" % (n, kind, line[line.index("[tape:"):line.index("]", line.index("[tape:")) + 1] if "[tape:" in line else "no tape line"))
    finally:
        eng.debug_configure("plan_cache", 1)
        eng.debug_configure("phases", 0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    for vk in vks.values():
        vk.close()
    eng.bases_free(table)
    eng.close()


if __name__ == "__main__":
    main()
