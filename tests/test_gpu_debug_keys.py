"""h2agg_debug_configure's key table against its documentation: the rows of DEBUG_KEYS (csrc/config_api.inc), the defaults of
the context's dbg_ members (csrc/h2agg.hip) and the "Test hooks" comment of include/h2agg.h name the same keys with the same
defaults, every key is accepted, and the ranged ones are refused just outside their range with a message that names them.

Every test here uses a context of its own and closes it: the session's engine is never left with a non-default key."""
import os
import re

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo2-snark-aggregator_amd", "csrc")
INT_MAX = 2**31 - 1

# key -> documented default (include/h2agg.h "Test hooks")
KEYS = {
    "pcie_slices": 0, "pcie_glv": 0, "pcie_chain": 1, "comb_msm": 1, "plan_cache": 1, "small_sort": 1, "eval_split": 1,
    "lean_acc": 1, "tape_lds": 1, "prewake": 1, "phases": 0, "fr_fft_local": 0, "fr_fft_batch_chunk": 0, "fr_poly_chunk": 0,
    "fr_scan_chunk": 0, "fr_sort_tile": 0, "commit_chunk": 0, "lean_full": 0, "pre_big": 0, "seg_chunk": 0, "seg_c": 0,
    "shard_fail": 0, "launch_cus": 0,
}
# key -> (lowest, highest) accepted value besides 0
RANGES = {
    "seg_c": (4, 8), "fr_fft_local": (1, 11), "fr_poly_chunk": (3, 11), "fr_scan_chunk": (3, 11), "fr_sort_tile": (4, 11),
    "fr_fft_batch_chunk": (0, INT_MAX), "commit_chunk": (0, INT_MAX), "launch_cus": (1, 1024),
}
REFUSED = [("seg_c", 3), ("seg_c", 9), ("fr_fft_local", -1), ("fr_fft_local", 12), ("fr_poly_chunk", 2), ("fr_poly_chunk", 12),
           ("fr_scan_chunk", 2), ("fr_scan_chunk", 12), ("fr_sort_tile", 3), ("fr_sort_tile", 12), ("fr_fft_batch_chunk", -1),
           ("commit_chunk", -1), ("launch_cus", -1), ("launch_cus", 1025)]


def header_keys():
    text = open(os.path.join(ROOT, "include", "h2agg.h")).read()
    end = text.index("int h2agg_debug_configure(")
    block = text[text.rindex("Test hooks", 0, end):end]
    return set(re.findall(r'"(\w+)"', block))


def table_rows():
    """key -> the context member its row sets"""
    text = open(os.path.join(CSRC, "config_api.inc")).read()
    body = text[text.index("const DebugKey DEBUG_KEYS[] = {"):]
    body = body[:body.index("};")]
    return dict(re.findall(r'\{"(\w+)", &h2agg_ctx::(dbg_\w+)', body))


def member_defaults():
    text = open(os.path.join(CSRC, "h2agg.hip")).read()
    return {m: int(v) for m, v in re.findall(r"^\s*int (dbg_\w+) = (-?\d+);", text, re.M)}


@pytest.fixture()
def own(pkg):
    e = pkg.H2Agg(0)
    yield e
    e.close()


def test_key_set_matches_header_and_table():
    assert header_keys() == set(KEYS)
    rows = table_rows()
    assert set(rows) == set(KEYS)
    assert len(set(rows.values())) == len(rows), "two keys set one member"
    defaults = member_defaults()
    for key, member in rows.items():
        assert member == "dbg_" + key
        assert defaults[member] == KEYS[key], key


def test_every_key_is_accepted_with_its_default(own):
    for key, default in KEYS.items():
        own.debug_configure(key, default)


def test_ranged_keys_are_refused_outside_their_range(pkg, own):
    for key, value in REFUSED:
        with pytest.raises(pkg.H2AggError) as ei:
            own.debug_configure(key, value)
        assert ei.value.code == pkg.ERR_INVALID, (key, value)
        assert "h2agg_debug_configure: " + key + " must be " in str(ei.value), (key, value)
    with pytest.raises(pkg.H2AggError, match="fr_poly_chunk must be 0 or 3 .. 11"):
        own.debug_configure("fr_poly_chunk", 12)
    with pytest.raises(pkg.H2AggError, match="commit_chunk must be >= 0"):
        own.debug_configure("commit_chunk", -1)
    with pytest.raises(pkg.H2AggError, match="launch_cus must be 0 or 1 .. 1024"):
        own.debug_configure("launch_cus", 1025)


def test_ranged_keys_are_accepted_at_both_ends_and_at_zero(own):
    for key, (lo, hi) in RANGES.items():
        for value in (lo, hi, 0):
            own.debug_configure(key, value)


def test_special_cases(pkg, own):
    with pytest.raises(pkg.H2AggError, match="measure build only") as ei:   # (the suite runs the product build)
        own.debug_configure("lean_acc", 0)
    assert ei.value.code == pkg.ERR_INVALID
    own.debug_configure("lean_acc", 1)
    with pytest.raises(pkg.H2AggError, match="h2agg_debug_configure: unknown key no_such_key") as ei:
        own.debug_configure("no_such_key", 1)
    assert ei.value.code == pkg.ERR_INVALID
    assert own._lib.h2agg_debug_configure(own._ctx, None, 0) == pkg.ERR_INVALID
