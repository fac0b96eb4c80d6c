"""CPU: bench.py's helpers that must never cost the headline line — the rocm-smi power sample behind the timed region and the
tie between the committed counter evidence and the kernel sources."""
import json
import os

import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_power_sample_is_harmless_without_a_gpu():
    """no GPU here: rocm-smi (if present at all) prints no GPU[0] rows -> None, never an exception; the burst still runs"""
    calls = []
    got = bench.sample_power(lambda: calls.append(1), lambda: None, 0, seconds=0.05)
    assert calls, "the burst is re-issued while the sample is taken"
    assert got is None or {"package_w_during_msm_loop", "cap_w", "frac_of_cap"} <= set(got)


def test_committed_counter_evidence_matches_the_kernel_sources():
    """profiles/r*_traffic.json is stamped with the hash of the MSM kernel sources; bench.py calls it stale otherwise"""
    sha = bench.csrc_sha()
    newest = sorted(p for p in os.listdir(os.path.join(ROOT, "profiles")) if p.endswith("_traffic.json") and "batch" not in p)[-1]
    with open(os.path.join(ROOT, "profiles", newest)) as f:
        if json.load(f)["csrc_sha"] != sha:   # (mid-round state: bench.py then says "stale" instead of quoting the counters)
            pytest.skip("kernel sources changed since %s was collected: run tools/profile_round.sh on the GPU box" % newest)
    nbytes, valu, how = bench.pmc_evidence("msm_accumulate", 20)
    assert nbytes and valu and how.startswith("csrc_sha"), how


def test_dump_outputs_writes_exact_float_arrays(tmp_path):
    """--dump-outputs: canonical affine points become float32 bytes that convert back exactly; only float arrays, capped"""
    import numpy as np
    from oracle import bn254 as O
    pts = [O.G1, O.scalar_mul(O.R - 1, O.G1), O.scalar_mul(0x1234567, O.G1)]
    aff = b"".join(O.aff_to_bytes(p) for p in pts)
    a = bench.affine_array(aff)
    assert a.dtype == np.float32 and a.shape == (3, 2, 32)
    bench.dump_outputs(str(tmp_path / "d"), {"msm_result_affine": a})
    back = np.load(str(tmp_path / "d" / "msm_result_affine.npy"))
    assert back.dtype == np.float32 and back.astype(np.uint8).tobytes() == aff
    with pytest.raises(TypeError):
        bench.dump_outputs(str(tmp_path / "e"), {"raw": np.zeros(4, dtype=np.uint8)})
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path / "f"), {"big": np.zeros(bench.DUMP_LIMIT_BYTES // 8 + 1, dtype=np.float64)})
    assert not (tmp_path / "f").exists()


def test_steps_below_one_is_refused():
    import subprocess
    import sys
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "--steps must be at least 1" in p.stderr, p.stderr[-2000:]
