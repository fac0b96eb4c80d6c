"""CPU: the host half of the Fr tape (csrc/tape_compile.hpp: schedule_levels, tape_lds_assign — the liveness allocator behind the
LDS register file of the kernel csrc/schema.hpp k_tape_run_lds — and compile_tape, which the product calls).  The header is
plain C++: tests/cpp/tape_lds_driver.cpp includes the PRODUCT's file as it stands and simulates the kernel's level / barrier
semantics on random programs: every register must come out right, no slot may be written in a level that reads it, programs
with more live values than slots must be refused untouched.  (The kernel itself:
tests/test_gpu_parity.py::test_fr_tape_register_file_in_lds.)"""
import os
import shutil
import subprocess

import __graft_entry__ as entry


def test_tape_lds_allocator(tmp_path):
    exe = str(tmp_path / "tape_lds_driver")
    subprocess.run([shutil.which("g++") or "g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(entry.PKG_DIR, "csrc"),
                    os.path.join(entry.ROOT, "tests", "cpp", "tape_lds_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "TAPE-LDS-ALLOC-OK" in r.stdout, r.stdout + r.stderr
