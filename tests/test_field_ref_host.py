"""The checkers of tests/field_ref.py can fail, the generators keep their contracts, and the probe library builds — no device needed.

tests/test_gpu_field_probe.py is only as good as field_ref's checks: here every check is fed an output that satisfies it (the
module's own Python model of the op) and then the wrong outputs a broken kernel would give — one limb off by one, a carry dropped
between two limbs, a value off by exactly m, a limb of 2^29, a lean "false" with one limb of acc changed — and must reject each.
"""
import pytest

from tests import field_ref as F
from tests import fp_probe

FQ, FR = F.FQ, F.FR
ALL = [(name, field) for name, fields in fp_probe.OPS.items() for field in fields]
IDS = ["%s-%s" % (n, fp_probe.FIELD_NAMES[f]) for n, f in ALL]
STEP = 97          # every 97th case of a set: the whole sets are checked on the device


@pytest.fixture(scope="module")
def probe():
    return fp_probe.Probe(fp_probe.build(verbose=False))


def test_probe_builds_and_exports_its_entry(probe):
    assert hasattr(probe.lib, "fp_probe_run")
    assert not fp_probe.stale()


def test_op_table_matches_the_library(probe):
    """every op of the Python table is instantiated for exactly its fields, and the library holds no op the table lacks"""
    assert probe.table() == {n: tuple(f) for n, f in fp_probe.OPS.items()}
    assert set(F.SPECS) == set(fp_probe.OPS)
    for name, field in ALL:
        nin, nout = probe.shape(field, name)
        assert 4 * max(nin, nout) <= 288     # fixed-size records: two XYZZ points at most
        fam, w = F.cases(field, name)[0]
        assert len(w) == nin and len(F.SPECS[name].model(field, w)) == nout, name


@pytest.mark.parametrize("name,field", ALL, ids=IDS)
def test_generators_keep_the_contract_and_the_model_passes(name, field):
    """building a case set runs the generators' REQUIRES assertions; the model's outputs pass the check"""
    cs = F.cases(field, name)
    assert len(cs) >= 64
    assert all(0 <= x < (1 << 32) for _, w in cs for x in w)
    sample = cs[::STEP] + cs[:8]
    F.verify(field, name, sample, [F.SPECS[name].model(field, w) for _, w in sample])


def _mutations(out, m, rows=1):
    """wrong result limbs a broken kernel would give, for a 9-limb result at out[0:9] (rows = 4: the limb-parallel records hold the
    result once per DPP row, and all four get the same wrong limbs — the rows agree, the value is what is wrong)"""
    r = list(out[:9])
    rest = list(out[9 * rows:])
    muts = []
    a = list(r); a[3] ^= 1; muts.append(("limb 3 off by one", a))
    a = list(r); a[0] = (a[0] + 1) & 0xFFFFFFFF; muts.append(("limb 0 off by one", a))
    for i in range(1, 9):
        if r[i] > 0:
            a = list(r); a[i] -= 1; muts.append(("carry into limb %d dropped" % i, a))
            a = list(r); a[i] -= 1; a[i - 1] += 1 << 29; muts.append(("limb %d holds 2^29 more: same integer, not tight" % (i - 1), a))
            if r[i] > 1:
                a = list(r); a[i] -= 2; a[i - 1] += 1 << 30; muts.append(("limb %d holds 2^30 more: same integer, not even nearly tight" % (i - 1), a))
            break
    v = F.val(r)
    if v + m < (1 << 261):
        muts.append(("value + m", F.tight(v + m)))
    if v + 2 * m < (1 << 261):
        muts.append(("value + 2m", F.tight(v + 2 * m)))
    if v >= m:
        muts.append(("value - m", F.tight(v - m)))
    return [(what, a * rows + rest) for what, a in muts]


VALUE_OPS = ["fp_add", "fp_dbl", "fp_triple", "fp_normalize", "fp_cond_sub", "fp_sub<2>", "fp_sub<8>", "fp_neg<4>", "fp_sub2<4>",
             "fp_sub_sub2<6>", "fp_sub_sgn<4,6>", "fp_sub_sgn<2,4>", "fp_mul_ps", "fp_mul_os", "fp_sqr_ps", "fp_mul2_ps", "fp_mul3_ps",
             "fp_mul_dual", "fp_sqr_dual", "fp_mul2_mul_mul", "fpa_mul_ip", "fpa_mul", "fpa_sqr", "fpa_mul2_ip1", "fpa_mul_dual_ip",
             "fpa_sqr_dual", "fpa_mul2_ip", "loose_tail<8,ip>", "fp_canonical", "fp_to_mont", "fp_from_mont", "fp_inv_int", "fp_inv",
             "lp_mul", "lp_sub<9>", "lp_neg<5>", "lp_triple"]


@pytest.mark.parametrize("name", VALUE_OPS)
def test_value_checks_reject_wrong_limbs(name):
    field = fp_probe.OPS[name][0]
    m, spec = F.MOD[field], F.SPECS[name]
    cs = F.cases(field, name)
    tried = {}
    for fam, w in cs[::STEP]:
        good = spec.model(field, w)
        assert spec.check(field, w, good) is None
        rows = 4 if name.startswith("lp_") else 1
        for what, bad in _mutations(good, m, rows=rows):
            if bad == good:
                continue
            if rows == 4 and "2^29 more" in what and F.is_nearly_tight(bad[:9]):
                continue                                   # a limb of 2^29 is inside the limb-parallel contract; 2^30 more is not
            if name == "fp_inv" and what.startswith("value") and F.val(bad[:9]) < 2 * m:
                continue                                   # its contract is "below 2m": the other representative is as good
            e = spec.check(field, w, bad)
            assert e is not None, "%s: '%s' passed the check (family %s)" % (name, what, fam)
            assert "rows disagree" not in e
            tried[what.split(" ")[0]] = tried.get(what.split(" ")[0], 0) + 1
    assert {"limb", "carry", "value"} <= set(tried), tried


@pytest.mark.parametrize("name", ["fp_sub_loose<10>", "fp_neg_loose<8>", "fp_neg_loose<4>"])
def test_loose_checks_reject_wrong_limbs(name):
    spec = F.SPECS[name]
    for fam, w in F.cases(FQ, name)[::STEP]:
        good = spec.model(FQ, w)
        assert spec.check(FQ, w, good) is None
        bad = list(good); bad[2] += 1
        assert spec.check(FQ, w, bad) is not None
        bad = list(good); bad[4] += 1 << 31; bad[5] -= 1 << 2      # the same integer, a limb far above its stated maximum
        assert spec.check(FQ, w, bad) is not None


@pytest.mark.parametrize("name", ["fp_is_canonical", "fp_maybe_zero_mod<10>", "fp_maybe_zero_mod2<10>", "fp_is_zero_mod<10>",
                                  "fp_maybe_zero_mod2<4>"])
def test_flag_checks_reject_the_other_answer(name):
    spec = F.SPECS[name]
    seen = set()
    for fam, w in F.cases(FQ, name):
        good = spec.model(FQ, w)
        seen.add(good[0])
        assert spec.check(FQ, w, [1 - good[0]]) is not None
    assert seen == {0, 1}


def test_filters_see_every_multiple_and_the_two_limb_filter_sees_through_2_pow_29():
    """the case sets hold what the issue names: k*m for every k < K (true everywhere), k*m + 2^29 (maybe / false / false), k*m +- 1"""
    p = F.MOD[FQ]
    for K in (4, 6, 10):
        fams = dict(F.cases(FQ, "fp_maybe_zero_mod<%d>" % K))
        for k in range(K):
            w = fams["%d*m" % k]
            assert [F.SPECS[n % K].model(FQ, w) for n in ("fp_maybe_zero_mod<%d>", "fp_maybe_zero_mod2<%d>", "fp_is_zero_mod<%d>")] == [[1], [1], [1]]
            w = fams["%d*m + 2^29" % k]
            assert F.val(w) == k * p + (1 << 29)
            assert [F.SPECS[n % K].model(FQ, w) for n in ("fp_maybe_zero_mod<%d>", "fp_maybe_zero_mod2<%d>", "fp_is_zero_mod<%d>")] == [[1], [0], [0]]
            w = fams["%d*m + 1" % k]
            assert [F.SPECS[n % K].model(FQ, w) for n in ("fp_maybe_zero_mod<%d>", "fp_maybe_zero_mod2<%d>", "fp_is_zero_mod<%d>")] == [[0], [0], [0]]


GROUP_OPS = ["xyzz_double", "xyzz_double_affine", "xyzz_add_affine", "xyzz_add_affine_affine", "xyzz_add", "lp_double", "lp_add_points",
             "xyzz_add_affine_lean<1,3>", "xyzz_add_affine_affine_lean<0,0>"]


@pytest.mark.parametrize("name", GROUP_OPS)
def test_group_checks_reject_wrong_points(name):
    spec = F.SPECS[name]
    p = F.P
    n = 0
    cs = F.cases(FQ, name)
    for fam, w in cs[::max(1, min(STEP, len(cs) // 12))]:
        good = spec.model(FQ, w)
        assert spec.check(FQ, w, good) is None
        if F.val(good[18:27]) == 0 or (len(good) == 37 and good[36] == 0):
            continue
        n += 1
        for c in range(4):                       # each coordinate: one limb off; off by p (same point, outside the invariant)
            bad = list(good); bad[9 * c + 2] ^= 1
            assert spec.check(FQ, w, bad) is not None, (name, fam, c)
            bound = (F.LP_BOUNDS if name.startswith("lp_") else F.XYZZ_BOUNDS)[c]
            v = F.val(good[9 * c:9 * c + 9])
            bad = list(good); bad[9 * c:9 * c + 9] = F.tight(v + -(-(bound * p - v) // p) * p)
            assert F.val(bad[9 * c:9 * c + 9]) >= bound * p and spec.check(FQ, w, bad) is not None, (name, fam, c)
        bad = list(good); bad[0] += 1 << 29; bad[1] -= 1     # a limb of 2^29 (and more): the same integer, not tight
        if bad[1] >= 0 and not name.startswith("lp_"):
            assert spec.check(FQ, w, bad) is not None
        # a consistent record of ANOTHER point
        other = F.model_record(F.O.double(F.rec_affine(good[:36]))) + list(good[36:])
        assert spec.check(FQ, w, other) is not None
    assert n >= 5


@pytest.mark.parametrize("name", ["xyzz_add_affine_lean<%d,%d>" % (d, v) for d in (0, 1) for v in range(4)])
def test_lean_false_must_be_said_and_must_leave_acc_alone(name):
    spec = F.SPECS[name]
    refused = 0
    var = int(name[-2])
    fams = set()
    for fam, w in F.cases(FQ, name):
        good = spec.model(FQ, w)
        if good[36] == 1:
            continue
        refused += 1
        fams.add("identity" if "identity base" in fam else ("same" if "same point" in fam else "opposite"))
        if refused % 7:
            continue
        assert spec.check(FQ, w, good) is None
        bad = list(good); bad[13] ^= 4                       # false, with one limb of acc changed
        assert spec.check(FQ, w, bad) is not None
        bad = F.model_record(F.O.INF) + [1]                   # true where the general formula was needed
        assert spec.check(FQ, w, bad) is not None
    assert fams == ({"same", "opposite", "identity"} if var & 1 else {"same", "opposite"})
    # q = +-acc in every representative of acc.x: U2 - X1 + 8p runs through its multiples
    ks = {fam.split("representatives ")[1][1] for fam, w in F.cases(FQ, name) if "same point" in fam and "point 0, ZZ" in fam}
    assert ks == set("01234567")
    # an ordinary pair that is refused is an error too
    fam, w = next((f, w) for f, w in F.cases(FQ, name) if "other point" in f)
    assert spec.check(FQ, w, list(w[:36]) + [0]) is not None


def test_lp_rows_must_agree():
    spec = F.SPECS["lp_mul"]
    fam, w = F.cases(FQ, "lp_mul")[5]
    good = spec.model(FQ, w)
    bad = list(good); bad[9 * 2 + 4] ^= 1
    assert spec.check(FQ, w, good) is None and spec.check(FQ, w, bad) is not None


def test_column_model_vectors_are_in_the_two_product_blocks():
    """both operand sets of tools/fp_column_bounds.py CASES, at the exact per-limb maxima, go through both blocks"""
    for name in ("fpa_mul2_ip", "fpa_mul2_ip1"):
        fams = [f for f, w in F.cases(FQ, name) if f.startswith("column model maxima")]
        assert fams == ["column model maxima of xyzz_add_affine_lean", "column model maxima of xyzz_add_affine_affine_lean"]
        for f, w in F.cases(FQ, name):
            if f in fams:
                assert max(w[27:35]) >= (1 << 30) and max(w[0:8]) >= (1 << 29)      # loose, as the model has them


PRODUCT_OPS = ["fp_mul_ps", "fp_mul_os", "fp_sqr_ps", "fp_sqr_os", "fp_mul2_ps", "fp_mul2_os", "fp_mul3_ps", "fp_mul_dual", "fp_sqr_dual",
               "fp_mul2_mul_mul", "fpa_mul_ip", "fpa_mul", "fpa_sqr", "fpa_mul2_ip1", "fpa_mul_dual_ip", "fpa_sqr_dual", "fpa_mul2_ip",
               "loose_tail<8,ip>", "loose_tail<8,ip1>", "loose_tail<4,ip>", "loose_tail<4,ip1>", "lp_mul"]


@pytest.mark.parametrize("name", PRODUCT_OPS)
def test_product_case_sets_hold_every_operand_at_all_ones_at_once(name):
    """the input that fills the 64-bit columns: limbs 0..7 of EVERY operand at 2^29 - 1 under the largest top limb its bound
    allows — present for every bound set of every product, the largest (169: the top limb at its maximum too) included"""
    for field in fp_probe.OPS[name]:
        sets = {}
        for fam, w in F.cases(field, name):
            if fam.startswith("column model") or fam == "random" or fam.endswith(": random"):
                continue
            key = fam.split(":")[0] if fam.startswith("bounds") else ""
            full = all(x == F.M29 for i in range(0, len(w) - len(w) % 9, 9) for x in w[i:i + 8])
            sets[key] = sets.get(key, False) or full
        assert sets and all(sets.values()), (name, [k for k, v in sets.items() if not v])
    if name == "lp_mul":     # and the top of the nearly tight contract: every limb of both operands at 2^29 + 3
        top = F.M29 + 1 + F.LP_SLACK
        assert sum(all(x == top for i in (0, 9) for x in w[i:i + 8]) for _, w in F.cases(F.FQ, name)) == 6     # one per bound set


def test_every_field_op_gets_4096_random_cases():
    """4096 seeded random in-contract cases for every op with random cases; the inversion has the 2048 its input list names, the
    group-law ops are structured only"""
    for name, fields in fp_probe.OPS.items():
        if name.startswith(("xyzz_", "lp_double", "lp_add_points")):
            continue
        for field in fields:
            n = sum("random" in fam.split(": ")[-1] and "random near" not in fam for fam, _ in F.cases(field, name))
            want = 2048 if name in ("fp_inv", "fp_inv_int") else F.NRANDOM
            assert n >= want and (name.startswith(("lp_", "fp_normalize")) or n <= want + 8), (name, field, n)
