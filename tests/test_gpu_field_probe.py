"""The field layer and the group-law formulas on the device, at their contract edges.

Every primitive of csrc/fp.hpp and csrc/fp_asm.inc, the formulas of csrc/g1.hpp, the lean insertion forms of
csrc/msm_kernels.hpp and the limb-parallel code of csrc/lp_kernels.hpp runs as a kernel of its own over raw limbs
(tests/cpp/fp_probe.hip, built into tests/libfp_probe.so by tests/fp_probe.py) and is held against plain Python integers
(tests/field_ref.py): exact integer equations for the linear ops and the subtractions, the Montgomery identity r*R = T + q*m
with 0 <= q < R for every product, the oracle's group law for the formulas.  The inputs are the edges of each op's contract —
limb vectors of all ones, values at the top of their allowed range, every representative x + k*m, the worst-case vectors of
tools/fp_column_bounds.py, q = +-acc in every representative — and 4096 seeded random in-contract cases for every field and
limb-parallel op (2048 for the inversion, whose input list is its own; the group-law ops are structured only); the generators
assert each REQUIRES before anything is uploaded.
"""
import pytest

from tests import field_ref as F
from tests import fp_probe

pytestmark = pytest.mark.gpu

ALL = [(name, field) for name, fields in fp_probe.OPS.items() for field in fields]
IDS = ["%s-%s" % (n, fp_probe.FIELD_NAMES[f]) for n, f in ALL]


@pytest.fixture(scope="module")
def probe():
    """the probe library, rebuilt if one of its sources or of the product's headers is newer"""
    return fp_probe.Probe(fp_probe.build(verbose=False))


_hip_error = []     # the first HIP error of this module: after it no further probe kernel is launched


@pytest.mark.parametrize("name,field", ALL, ids=IDS)
def test_op_on_the_device(probe, name, field):
    if _hip_error:
        pytest.fail("not launched: an earlier probe kernel ended in a HIP error (%s)" % _hip_error[0])
    cs = F.cases(field, name)
    try:
        outs = probe.run(field, name, [w for _, w in cs])
    except RuntimeError as e:
        # a HIP error is a fault of the device or of a kernel, not a wrong result: the remaining probe tests fail without a launch
        _hip_error.append(str(e))
        raise
    F.verify(field, name, cs, outs)
