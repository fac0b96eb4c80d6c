"""CPU: the constants poly.py and the binding restate agree with the HIP sources they restate."""
import importlib
import os
import re

import __graft_entry__ as entry

CSRC = os.path.join(entry.PKG_DIR, "csrc")


def test_zeta_is_the_glv_lambda_of_the_msm(pkg):
    poly = importlib.import_module(entry.PKG_NAME + ".poly")
    src = open(os.path.join(CSRC, "sort_kernels.hpp")).read()
    lam = int(re.search(r"lambda = (0x[0-9a-f]{64})", src).group(1), 16)
    assert poly.ZETA_INT == lam
    words = lambda name: [int(x, 16) for x in re.search(name + r"\[\d\] = \{([^}]*)\}", src).group(1).replace("u", "").split(",")]
    assert sum(w << (32 * i) for i, w in enumerate(words("A1"))) == poly._GLV_A1
    assert sum(w << (32 * i) for i, w in enumerate(words("B1N"))) == poly._GLV_B1N
    r = poly.R_MOD
    assert pow(lam, 3, r) == 1 and lam != 1 and (poly._GLV_A1 - poly._GLV_B1N * lam) % r == 0


def test_fused_stage_count_matches_the_kernel_header(pkg):
    src = open(os.path.join(CSRC, "fr_fft_kernels.hpp")).read()
    assert int(re.search(r"FR_FFT_LOCAL = (\d+);", src).group(1)) == pkg.FR_FFT_LOCAL
    g1 = open(os.path.join(CSRC, "g1_fft_kernels.hpp")).read()
    assert int(re.search(r"FFT_MAX_K = (\d+);", g1).group(1)) == pkg.FR_FFT_MAX_K
