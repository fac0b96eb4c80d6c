"""TEST INFRASTRUCTURE ONLY — builds and loads the field-layer probe (tests/cpp/fp_probe.hip, fp_probe_group.hip): every primitive
of csrc/fp.hpp, csrc/fp_asm.inc, the group law of csrc/g1.hpp, the lean insertion forms of csrc/msm_kernels.hpp and the
limb-parallel code of csrc/lp_kernels.hpp as a kernel over raw limbs.  The library is tests/libfp_probe.so (git-ignored); it
is built with the product's flags and include path, from the product's headers as they stand, and stays out of libh2agg.so.

    python tests/fp_probe.py [--force]        build, print the op table
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "halo2-snark-aggregator_amd", "csrc")
CPP = os.path.join(HERE, "cpp")
OUT = os.path.join(HERE, "libfp_probe.so")
OBJ_DIR = os.path.join(HERE, "build")
SOURCES = ["fp_probe.hip", "fp_probe_group.hip"]       # compiled side by side, linked into one library
DEPS = [os.path.join(CPP, f) for f in SOURCES + ["fp_probe.hpp"]] + [
    os.path.join(CSRC, f) for f in ("fp.hpp", "fp_asm.inc", "g1.hpp", "msm_kernels.hpp", "sort_kernels.hpp",
                                    "batch_kernels.hpp", "fb_sort_kernels.hpp", "lp_kernels.hpp")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-I", CSRC]   # build_ext.FLAGS + -I csrc

FQ, FR = 0, 1
FIELD_NAMES = {FQ: "Fq", FR: "Fr"}

# name -> fields the product instantiates the primitive for.  tests/test_field_ref_host.py holds this table against the
# library's own (fp_probe_op_name / fp_probe_shape), so neither side can drop an op unnoticed.
_LEAN = ["%s<%d,%d>" % (f, d, v) for d in (1, 0) for f in ("xyzz_add_affine_lean", "xyzz_add_affine_affine_lean") for v in range(4)]
OPS = {
    # linear
    "fp_add": (FQ, FR), "fp_dbl": (FQ,), "fp_triple": (FQ,), "fp_normalize": (FQ, FR), "fp_cond_sub": (FQ, FR),
    "fp_is_canonical": (FQ, FR),
    # subtractions, every K the product uses
    "fp_sub<1>": (FR,), "fp_sub<2>": (FQ, FR), "fp_sub<3>": (FR,), "fp_sub<4>": (FQ,), "fp_sub<6>": (FQ,), "fp_sub<8>": (FQ,),
    "fp_neg<2>": (FQ, FR), "fp_neg<4>": (FQ,), "fp_sub2<4>": (FQ,), "fp_sub_sub2<6>": (FQ,),
    "fp_sub_sgn<4,6>": (FQ,), "fp_sub_sgn<2,4>": (FQ,), "fp_sub_loose<10>": (FQ,), "fp_neg_loose<8>": (FQ,), "fp_neg_loose<4>": (FQ,),
    # products
    "fp_mul_ps": (FQ, FR), "fp_mul_os": (FQ, FR), "fp_sqr_ps": (FQ, FR), "fp_sqr_os": (FQ, FR), "fp_mul2_ps": (FQ,),
    "fp_mul2_os": (FQ,), "fp_mul3_ps": (FQ, FR), "fp_mul_dual": (FQ,), "fp_sqr_dual": (FQ,), "fp_mul2_mul_mul": (FQ,),
    "fpa_mul_ip": (FQ,), "fpa_mul": (FQ,), "fpa_sqr": (FQ,), "fpa_mul2_ip1": (FQ,), "fpa_mul_dual_ip": (FQ,),
    "fpa_sqr_dual": (FQ,), "fpa_mul2_ip": (FQ,),
    "loose_tail<8,ip>": (FQ,), "loose_tail<8,ip1>": (FQ,), "loose_tail<4,ip>": (FQ,), "loose_tail<4,ip1>": (FQ,),
    # reduction and tests
    "fp_canonical": (FQ, FR), "fp_to_mont": (FQ, FR), "fp_from_mont": (FQ, FR),
    "fp_maybe_zero_mod<4>": (FQ,), "fp_maybe_zero_mod<6>": (FQ,), "fp_maybe_zero_mod<10>": (FQ,),
    "fp_maybe_zero_mod2<4>": (FQ,), "fp_maybe_zero_mod2<6>": (FQ,), "fp_maybe_zero_mod2<10>": (FQ,),
    "fp_is_zero_mod<2>": (FQ, FR), "fp_is_zero_mod<4>": (FQ,), "fp_is_zero_mod<6>": (FQ,), "fp_is_zero_mod<8>": (FQ,),
    "fp_is_zero_mod<10>": (FQ,),
    "fp_unpack": (FQ, FR), "fp_pack": (FQ, FR),
    # inversion
    "fp_inv_int": (FQ, FR), "fp_inv": (FQ, FR),
    # group law
    "xyzz_double": (FQ,), "xyzz_double_affine": (FQ,), "xyzz_add_affine": (FQ,), "xyzz_add_affine_affine": (FQ,),
    "xyzz_add": (FQ,), "xyzz_add_chains": (FQ,),
    **{n: (FQ,) for n in _LEAN},
    # limb-parallel
    "lp_mul": (FQ,), "lp_sub<3>": (FQ,), "lp_sub<5>": (FQ,), "lp_sub<7>": (FQ,), "lp_sub<9>": (FQ,), "lp_sub<11>": (FQ,),
    "lp_neg<3>": (FQ,), "lp_neg<5>": (FQ,), "lp_triple": (FQ,), "lp_double": (FQ,), "lp_add_points": (FQ,),
}


def _hipcc() -> str:
    h = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return h if os.path.exists(h) else "hipcc"


def stale() -> bool:
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    return any(os.path.getmtime(d) > t for d in DEPS)


def build(force: bool = False, verbose: bool = True) -> str:
    """tests/libfp_probe.so, rebuilt when a source or one of the product's headers it includes is newer."""
    if not force and not stale():
        return OUT
    os.makedirs(OBJ_DIR, exist_ok=True)
    hipcc = _hipcc()
    t0 = time.time()
    objs, procs = [], []
    for s in SOURCES:
        obj = os.path.join(OBJ_DIR, s.replace(".hip", ".o"))
        cmd = [hipcc] + FLAGS + ["-c", os.path.join(CPP, s), "-o", obj]
        if verbose:
            print("[fp_probe] " + " ".join(cmd), flush=True)
        procs.append((cmd, subprocess.Popen(cmd)))
        objs.append(obj)
    failed = [cmd for cmd, p in procs if p.wait() != 0]
    if failed:
        raise subprocess.CalledProcessError(1, failed[0])
    tmp = OUT + ".tmp"
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp] + objs
    if verbose:
        print("[fp_probe] " + " ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    os.replace(tmp, OUT)
    if verbose:
        print("[fp_probe] built in %.0f s" % (time.time() - t0), flush=True)
    return OUT


class Probe:
    """ctypes face of the library.  Loading needs no device; run() does."""

    def __init__(self, path: str | None = None):
        self.lib = C.CDLL(path or build(verbose=False))
        self.lib.fp_probe_op_count.restype = C.c_int
        self.lib.fp_probe_op_name.restype = C.c_char_p
        self.lib.fp_probe_op_name.argtypes = [C.c_int]
        self.lib.fp_probe_shape.restype = C.c_int
        self.lib.fp_probe_shape.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        self.lib.fp_probe_run.restype = C.c_int
        self.lib.fp_probe_run.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
        self.op_ids = {self.lib.fp_probe_op_name(i).decode(): i for i in range(self.lib.fp_probe_op_count())}

    def shape(self, field: int, name: str):
        """(input words, output words) per case, or None when the library has no such (field, op)"""
        if name not in self.op_ids:
            return None
        a, b = C.c_int(0), C.c_int(0)
        if self.lib.fp_probe_shape(field, self.op_ids[name], C.byref(a), C.byref(b)) != 0:
            return None
        return a.value, b.value

    def table(self):
        """{name: fields} as the library holds it"""
        return {n: tuple(f for f in (FQ, FR) if self.shape(f, n)) for n in self.op_ids}

    def run(self, field: int, name: str, cases):
        """cases: a list of flat word lists, one per case -> the output records, as lists of words.  Raises on a HIP error."""
        import numpy as np
        nin, nout = self.shape(field, name)
        n = len(cases)
        a = np.asarray(cases, dtype=np.uint64)
        assert a.shape == (n, nin), "%s: records of %d words, got %r" % (name, nin, a.shape)
        assert int(a.max(initial=0)) < (1 << 32)
        hin = np.ascontiguousarray(a.astype(np.uint32))
        hout = np.zeros((n, nout), dtype=np.uint32)
        rc = self.lib.fp_probe_run(field, self.op_ids[name], hin.ctypes.data, n, hout.ctypes.data)
        if rc != 0:
            raise RuntimeError("fp_probe_run(%s, %s): HIP error %d" % (FIELD_NAMES[field], name, rc))
        return hout.tolist()


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    p = Probe(OUT)
    for name, fields in p.table().items():
        print("%-40s %s" % (name, " ".join("%s %r" % (FIELD_NAMES[f], p.shape(f, name)) for f in fields)))
