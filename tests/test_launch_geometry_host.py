"""The launch caps that go by the CU count, held together (no GPU): every one of them is a call of launch_cap (csrc/host.inc),
the per-CU factors and the elements per workgroup the sources carry are the LAUNCH_* constants of the package, and
tests/launch_ref.py counts trips the way the kernels' loops take them."""
import os
import re

from tests import launch_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo2-snark-aggregator_amd", "csrc")


def src(name):
    return open(os.path.join(CSRC, name)).read()


def constant(name, text):
    m = re.search(r"constexpr int %s = ([^;]+);" % name, text)
    assert m, name
    return m.group(1).strip()


def function_body(text, head):
    at = text.index(head)
    return text[at:text.index("\n}\n", at)]


def test_cu_count_sizes_a_grid_through_launch_cap_only():
    users = {}
    for name in sorted(os.listdir(CSRC)):
        hits = len(re.findall(r"\bcu_count\b", src(name)))
        if hits:
            users[name] = hits
    assert set(users) == {"h2agg.hip", "host.inc"}
    body = function_body(src("host.inc"), "size_t launch_cap(const h2agg_ctx* c, unsigned per_cu)")
    assert "c->dbg_launch_cus ? c->dbg_launch_cus : c->cu_count" in body and "* per_cu" in body
    outside = src("host.inc").replace(body, "")
    assert not re.search(r"c->cu_count", outside)
    # the context sets it from the device and prints it; nothing else in h2agg.hip reads it
    assert len(re.findall(r"c->cu_count", src("h2agg.hip"))) == 2


def test_launch_constants_match_the_sources(pkg):
    block = int(constant("BLOCK", src("batch_kernels.hpp")))
    assert int(constant("SM_THREADS", src("scalar_mul_kernels.hpp"))) == 128
    assert constant("SM_GROUPS", src("scalar_mul_kernels.hpp")) == "SM_THREADS / 4"
    sm_groups = 128 // 4

    grid_for = function_body(src("host.inc"), "int grid_for(const h2agg_ctx* c, size_t n)")
    assert "(n + BLOCK - 1) / BLOCK" in grid_for
    assert re.findall(r"launch_cap\(c, (\d+)\)", grid_for) == [str(pkg.LAUNCH_ELEMENTWISE[0])]
    assert pkg.LAUNCH_ELEMENTWISE == (8, block)

    for name in ("chips_api.inc", "bases_api.inc"):
        text = src(name)
        assert re.findall(r"launch_cap\(c, (\d+)\)", text) == [str(pkg.LAUNCH_SCALAR_MUL[0])], name
        assert "+ SM_GROUPS - 1) / SM_GROUPS" in text, name
    assert pkg.LAUNCH_SCALAR_MUL == (16, sm_groups)

    run = src("msm_run.inc")
    order = function_body(run, "void msm_order(")
    assert set(re.findall(r"launch_cap\(c, (\d+)\)", order)) == {str(pkg.LAUNCH_SIZE_ORDER[0])}
    assert "dim3(g), dim3(BLOCK)" in order and "(r.p.NBT + BLOCK * 8 - 1) / (BLOCK * 8)" in order
    assert pkg.LAUNCH_SIZE_ORDER == (4, block)

    big = function_body(run, "void msm_big_kernels(")
    assert re.findall(r"launch_cap\(c, (\d+)\)", big) == [str(pkg.LAUNCH_MSM_FIX[0]), str(pkg.LAUNCH_MSM_BIG[0])]
    assert re.search(r"k_msm_accumulate_fix, dim3\(\(unsigned\)std::min<size_t>\(launch_cap\(c, 12\), "
                     r"\(\(size_t\)p\.NBT \* lpb \+ 63\) / 64\)\), dim3\(64\)", big)
    assert "k_msm_accumulate_big, dim3((unsigned)grid), dim3(64)" in big
    assert "k_msm_big_combine, dim3((unsigned)gk), dim3(64)" in big
    assert pkg.LAUNCH_MSM_FIX == (12, 64) and pkg.LAUNCH_MSM_BIG == (8, 64)
    # every cap in the library is one of the five
    every = set()
    for name in os.listdir(CSRC):
        if name != "host.inc":
            every |= set(re.findall(r"launch_cap\(c, (\d+)\)", src(name)))
    every |= set(re.findall(r"launch_cap\(c, (\d+)\)", grid_for))
    assert every == {"4", "8", "12", "16"}


def test_trip_counts():
    t = launch_ref.trips
    T = 8 * 256
    assert [t(n, 256, 8, 1) for n in (1, 256, T, T + 1, 2 * T, 2 * T + 1)] == [1, 1, 1, 2, 2, 3]
    assert t(524288, 256, 8, 256) == 1 and t(524289, 256, 8, 256) == 2      # a 256-CU device
    assert [t(n, 32, 16, 1) for n in (512, 513, 1029)] == [1, 2, 3]
    assert t(131072, 32, 16, 256) == 1 and t(131073, 32, 16, 256) == 2
    # a short input takes fewer workgroups and still one trip
    assert launch_ref.workgroups(300, 256, 8, 1) == 2 and t(300, 256, 8, 1) == 1
    # jac_batch_normalise: a lane's eight points are a stride apart
    assert [t(n, 256, 8, 1, share=8) for n in (T + 1, 8 * T, 8 * T + 1, 9 * T + 3)] == [1, 1, 2, 2]
    assert [launch_ref.shared_points(n, 256, 8, 1, 8) for n in (T, T + 1, 8 * T, 9 * T + 3)] == [1, 2, 8, 8]
    assert launch_ref.shared_points(T + 1, 256, 8, 1, 8, lane=1) == 1
    # msm_order sizes its grid by 8 * 256 buckets per workgroup and strides by 256
    assert launch_ref.workgroups(3 * 2048, 256, 4, 256, sized_by=2048) == 3 and t(3 * 2048, 256, 4, 256, sized_by=2048) == 8
    assert launch_ref.workgroups(1 << 15, 256, 4, 1, sized_by=2048) == 4 and t(1 << 15, 256, 4, 1, sized_by=2048) == 32
