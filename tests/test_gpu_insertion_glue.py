"""The bucket insertion's code BETWEEN its Montgomery products (csrc/msm_kernels.hpp k_msm_accumulate_lean / _lean_v): the
per-table "holds no identity base" flag and the instantiation without the identity test, the digit's sign folded into
r = +-S2 - Y1 (and into y2 - y1 for a bucket's second point), the instantiation without the endomorphism select, the loose
operands of the last product block, and the fix-up contract behind all of them.

Every multi_exp goes through h2agg_g1_msm_device_async over a resident table — the entry point the benchmark times — and is
compared with ((sum_i g_i s_i) mod r) * G: the sum in Python integers, one scalar multiplication by the oracle (tests/util.py
msm_want), canonical affine bytes.  Bases that are multiples of G with known coefficients come from the oracle
(bases_from_coefficients) or, where the case is about h2agg_bases_generate / n = 2^16, from the device with their coefficients
known and a sample checked against the oracle.
"""
import functools
import os
import subprocess
import sys
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from oracle import bn254 as O
from tests.test_gpu_dependent_bases import configured as configured_msm, family_case
from tests.util import bases_from_coefficients, fr_bytes, msm_want, norm, points_from_scalars, rand_frs

pytestmark = pytest.mark.gpu

LEAN_ID, LEAN_ENDO = 1, 2      # csrc/msm_kernels.hpp
DEV = "cuda:0"


@contextmanager
def configured(eng, full=False, **kw):
    """one MSM configuration (tests/test_gpu_dependent_bases.py); full: the bucket accumulation's instantiation for any table and
    any plan (h2agg_debug_configure "lean_full")"""
    with configured_msm(eng, **kw):
        try:
            eng.debug_configure("lean_full", int(full))
            yield
        finally:
            eng.debug_configure("lean_full", 0)


def to_dev(b):
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).to(DEV)


def msm_device(eng, handle, ss):
    """h2agg_g1_msm_device_async over the first len(ss) bases of a resident table -> canonical affine bytes (oracle-normalised)"""
    d_s = to_dev(fr_bytes(ss))
    d_out = torch.zeros(96, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    eng.g1_msm_device_async(handle, d_s.data_ptr(), len(ss), d_out.data_ptr())
    eng.synchronize()
    return norm(eng, bytes(d_out.cpu().numpy().tobytes()))


class Tables:
    """resident tables of g_i * G, one per creating path"""

    @staticmethod
    def upload(eng, gs):
        return eng.bases_upload(bases_from_coefficients(gs))

    @staticmethod
    def generate(eng, gs):
        d_k = to_dev(fr_bytes(gs))
        torch.cuda.synchronize()
        return eng.bases_generate(d_k.data_ptr(), len(gs))

    @staticmethod
    def fft(eng, gs):
        """forward transform of the inverse transform of the table: the same points, written by h2agg_bases_fft"""
        k = len(gs).bit_length() - 1
        assert len(gs) == 1 << k
        h0 = eng.bases_upload(bases_from_coefficients(gs))
        h1 = eng.bases_fft(h0, k, inverse=True)
        try:
            return eng.bases_fft(h1, k)
        finally:
            eng.bases_free(h0)
            eng.bases_free(h1)


PATHS = ["upload", "generate", "fft"]


@functools.lru_cache(maxsize=None)
def table64():
    rng = O.SplitMix64(0x1DF1A6)
    return tuple(rand_frs(rng, 64)), tuple(rand_frs(rng, 64))


IDENTITY_AT = {"none": (), "first": (0,), "last": (63,), "middle": (21, 40)}


# ------------------------------------------------------------------ the identity flag, both instantiations
@pytest.mark.parametrize("where", list(IDENTITY_AT))
@pytest.mark.parametrize("path", PATHS)
def test_identity_flag_and_both_instantiations(eng, path, where):
    gs, ss = (list(x) for x in table64())
    for i in IDENTITY_AT[where]:
        gs[i] = 0
    h = getattr(Tables, path)(eng, gs)
    try:
        assert eng.bases_download(h, 0, 64) == bases_from_coefficients(gs)
        assert eng.table_may_hold_identity(h) == bool(IDENTITY_AT[where])
        want = msm_want(gs, ss)
        for glv in (-1, 1):
            with configured(eng, glv=glv):
                assert msm_device(eng, h, ss) == want
                flagged = (LEAN_ID if IDENTITY_AT[where] else 0) | (LEAN_ENDO if glv > 0 else 0)
                assert eng.last_lean_variant() == flagged
            # the instantiation for any table and any plan, on the same table
            with configured(eng, glv=glv, full=True):
                assert msm_device(eng, h, ss) == want
                assert eng.last_lean_variant() == LEAN_ID | LEAN_ENDO
    finally:
        eng.bases_free(h)


def test_params_setup_tables_hold_no_identity(eng):
    """h2agg_params_setup: s^i * G and L_i(s) * G, never the identity (s != 0, s^n != 1)"""
    s = O.SplitMix64(0x5E7).fr()
    hg, hl = eng.params_setup(6, O.fe_to_bytes(s))
    try:
        ss = rand_frs(O.SplitMix64(0x5E8), 64)
        for h in (hg, hl):
            assert not eng.table_may_hold_identity(h)
        with configured(eng, glv=-1):
            assert msm_device(eng, hg, ss) == msm_want([pow(s, i, O.R) for i in range(64)], ss)
            assert eng.last_lean_variant() == 0
    finally:
        eng.bases_free(hg)
        eng.bases_free(hl)


@pytest.mark.parametrize("path", ["upload", "generate"])
def test_table_of_one_identity(eng, path):
    h = getattr(Tables, path)(eng, [0])
    try:
        assert eng.table_may_hold_identity(h)
        for glv in (-1, 1):
            with configured(eng, glv=glv):
                assert msm_device(eng, h, [0x1234567]) == bytes(64)
    finally:
        eng.bases_free(h)


# ------------------------------------------------------------------ the folded sign
def scalar_from_raw_digits(digits, c):
    return sum(d << (c * w) for w, d in enumerate(digits))


def signed_scalars(n, negative, seed, c=16):
    """every one of the low 15 c-bit windows holds a raw digit whose signed recoding is negative (0x8001 .. 0xfffe, so that the
    carry from below cannot push it to 0) resp. positive (1 .. 0x7ffe); the top window stays small: the scalar is < r"""
    rng = O.SplitMix64(seed)
    half = 1 << (c - 1)
    out = []
    for _ in range(n):
        ds = [(half + 1 + rng.next() % (half - 2)) if negative else (1 + rng.next() % (half - 2)) for _ in range(15)]
        s = scalar_from_raw_digits(ds + [1 + rng.next() % 0x1000], c)
        assert s < O.R and all(((s >> (c * w)) & 0xffff) in (range(0x8001, 0xffff) if negative else range(1, 0x7fff)) for w in range(15))
        out.append(s)
    return out


@functools.lru_cache(maxsize=None)
def random_table(n):
    gs = rand_frs(O.SplitMix64(0x7AB1E + n), n)
    return gs, bases_from_coefficients(gs)


@pytest.mark.parametrize("negative", [True, False])
@pytest.mark.parametrize("n", [64, 1024])
def test_sign_fold_all_digits_of_one_sign(eng, n, negative):
    gs, bases = random_table(n)
    ss = signed_scalars(n, negative, 0x516 + n + negative)
    want = msm_want(gs, ss)
    h = eng.bases_upload(bases)
    try:
        assert not eng.table_may_hold_identity(h)
        with configured(eng, window_bits=16, glv=-1):
            assert msm_device(eng, h, ss) == want
            assert eng.last_lean_variant() == 0
        with configured(eng, glv=-1):                   # the default width for this size
            assert msm_device(eng, h, ss) == want
        with configured(eng, window_bits=16, glv=-1, full=True):
            assert msm_device(eng, h, ss) == want
    finally:
        eng.bases_free(h)


@pytest.mark.parametrize("n", [64, 1024])
def test_sign_fold_alternating_signs_in_one_bucket(eng, n):
    """the scalars d and 2^16 - d alternate: window 0 recodes them to +d and -d, so bucket |d| of window 0 receives every point,
    with alternating signs, in whatever order the sort leaves them; and s, r - s alternate: equal up to sign mod r"""
    gs, bases = random_table(n)
    d = 0x2b67
    rng = O.SplitMix64(0xA17)
    s0 = rng.fr()
    h = eng.bases_upload(bases)
    try:
        for ss in ([d if i % 2 == 0 else (1 << 16) - d for i in range(n)],
                   [d if i % 3 else (1 << 16) - d for i in range(n)],
                   [s0 if i % 2 == 0 else O.R - s0 for i in range(n)]):
            want = msm_want(gs, ss)
            for lanes in (1, 0):
                with configured(eng, window_bits=16, glv=-1, big=4096, lanes=lanes):
                    assert msm_device(eng, h, ss) == want
            with configured(eng, glv=1, big=4096):
                assert msm_device(eng, h, ss) == want
    finally:
        eng.bases_free(h)


def test_sign_fold_recoding_boundaries(eng):
    gs, bases = random_table(64)
    edge = [O.R - 1, 1, 1 << 15, (1 << 15) + 1, (1 << 16) - 1]
    h = eng.bases_upload(bases)
    try:
        for rot in range(len(edge)):
            ss = [edge[(i + rot) % len(edge)] for i in range(64)]
            want = msm_want(gs, ss)
            for cfg in ({"window_bits": 16, "glv": -1}, {"glv": -1}, {"window_bits": 16, "glv": 1}, {}):
                with configured(eng, **cfg):
                    assert msm_device(eng, h, ss) == want, (rot, cfg)
    finally:
        eng.bases_free(h)


# ------------------------------------------------------------------ buckets of 1, 2, 3 and 4 entries
def signed_digit_scalar(digits, c):
    s = sum(d << (c * w) for w, d in enumerate(digits))
    assert 0 < s < O.R
    return s


@pytest.mark.parametrize("signs", ["plus", "minus", "mixed"])
@pytest.mark.parametrize("c", [8, 16])
def test_buckets_of_one_to_four_entries(eng, c, signs):
    """n = 4.  Window 0: one bucket of 4 (copy, affine + affine, two mixed additions); window 1: buckets of 3 and 1; window 2:
    two buckets of 2; the top digit (+1 for all) keeps the scalars positive.  Signed digits d_w with |d_w| < 2^(c-1) - 1 are
    what the recoding gives back from sum d_w 2^(c w)."""
    a, b, g, e, f = 5, 9, 17, 33, 65
    sg = {"plus": [1, 1, 1, 1], "minus": [-1, -1, -1, -1], "mixed": [1, -1, -1, 1]}[signs]
    digits = [[a, b, e], [a, b, e], [a, b, f], [a, g, f]]
    ss = [signed_digit_scalar([sg[i] * d for d in digits[i]] + [1], c) for i in range(4)]
    gs, bases = random_table(64)
    h = eng.bases_upload(bases[:64 * 4])
    try:
        with configured(eng, window_bits=c, glv=-1, lanes=1):
            assert msm_device(eng, h, ss) == msm_want(gs[:4], ss)
            assert eng.last_lean_variant() == 0
        with configured(eng, window_bits=c, glv=-1, lanes=1, full=True):
            assert msm_device(eng, h, ss) == msm_want(gs[:4], ss)
    finally:
        eng.bases_free(h)


# ------------------------------------------------------------------ the fix-up path is still taken
@pytest.mark.parametrize("glv", [-1, 1])
@pytest.mark.parametrize("family", ["one_point", "alternating_sign", "small_multiples"])
def test_fix_up_equal_opposite_repeated_bases(eng, family, glv):
    case = family_case(family, 600)
    h = eng.bases_upload(case.bases)
    try:
        assert eng.table_may_hold_identity(h) == (0 in [m % O.R for m in case.ms])
        for c in (0, 8):
            with configured(eng, window_bits=c, glv=glv):
                assert msm_device(eng, h, case.ss) == case.want
    finally:
        eng.bases_free(h)


@pytest.mark.parametrize("path", ["upload", "generate"])
def test_fix_up_identity_among_ordinary_points_of_one_bucket(eng, path):
    """equal scalars: every window has one bucket, and it holds the identity bases beside the ordinary ones — at its head, in the
    middle and at its end, whatever order the sort leaves"""
    n = 64
    gs = list(table64()[0])
    for i in (0, 1, 30, 31, 63):
        gs[i] = 0
    s = O.SplitMix64(0x1D).fr()
    h = getattr(Tables, path)(eng, gs)
    try:
        assert eng.table_may_hold_identity(h)
        for ss in ([s] * n, [s if i % 2 else O.R - s for i in range(n)]):
            for cfg in ({"glv": -1, "big": 4096, "lanes": 1}, {"glv": -1, "big": 4096}, {"glv": 1, "big": 4096}, {}):
                with configured(eng, **cfg):
                    assert msm_device(eng, h, ss) == msm_want(gs, ss), cfg
    finally:
        eng.bases_free(h)


# ------------------------------------------------------------------ the digit-major sort path, and GLV
def generated_table(eng, ks):
    """k_i * G made on the device (what the benchmark does), a sample checked against the oracle"""
    h = Tables.generate(eng, ks)
    idx = [0, 1, len(ks) // 2, len(ks) - 1]
    want = points_from_scalars([ks[i] for i in idx])
    for j, i in enumerate(idx):
        assert eng.bases_download(h, i, 1) == want[64 * j:64 * j + 64]
    return h


def test_digit_major_sort_path_uniform_scalars(eng):
    n = 1 << 16
    rng = O.SplitMix64(0xD160)
    ks, ss = rand_frs(rng, n), rand_frs(rng, n)
    h = generated_table(eng, ks)
    try:
        assert not eng.table_may_hold_identity(h)
        with configured(eng, glv=-1):
            assert msm_device(eng, h, ss) == msm_want(ks, ss)
            assert eng.last_lean_variant() == 0
    finally:
        eng.bases_free(h)


@pytest.mark.parametrize("with_identity", [False, True])
def test_glv_plan_with_the_flag(eng, with_identity):
    n = 1 << 12
    rng = O.SplitMix64(0x61F + with_identity)
    ks, ss = rand_frs(rng, n), rand_frs(rng, n)
    if with_identity:
        for i in (0, 777, n - 1):
            ks[i] = 0
    h = generated_table(eng, ks)
    try:
        assert eng.table_may_hold_identity(h) == with_identity
        with configured(eng, glv=1):
            assert msm_device(eng, h, ss) == msm_want(ks, ss)
            assert eng.last_lean_variant() == LEAN_ENDO | (LEAN_ID if with_identity else 0)
    finally:
        eng.bases_free(h)


# ------------------------------------------------------------------ the register budget of every instantiation
def test_every_lean_instantiation_within_128_vgprs_and_no_scratch():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool = os.path.join(root, "tools", "kernel_resources.py")
    out = subprocess.run([sys.executable, tool, "k_msm_accumulate_lean"], capture_output=True, text=True, check=True).stdout
    rows = [l.rsplit(None, 4) for l in out.splitlines()[1:] if l.strip()]
    names = [r[0] for r in rows]
    assert len(rows) == 12, out          # 3 chain modes x (the full set + 3 reduced ones)
    for ch in (0, 1, 2):
        assert "k_msm_accumulate_lean<%d, true>" % ch in names, out
        for var in (0, 1, 2):
            assert "k_msm_accumulate_lean_v<%d, true, %d>" % (ch, var) in names, out
    for name, vgpr, _sgpr, scratch, _lds in rows:
        assert int(vgpr) <= 128 and int(scratch) == 0, (name, vgpr, scratch)
