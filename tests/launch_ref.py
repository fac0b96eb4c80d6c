"""The launch geometry of the grid-stride kernels whose workgroup cap goes by the CU count (csrc/host.inc launch_cap), restated
for the tests: how often a lane's loop body can run for an input of n elements.  A test that claims to walk a loop twice
asserts it with trips(), the way tests/test_gpu_lookup_permute.py asserts its loop_counts."""


def workgroups(n, per_workgroup, per_cu, cus, sized_by=None):
    """the grid of the launch: one workgroup per per_workgroup elements (sized_by, where the host sizes the grid by another
    count than a trip takes: msm_order asks for one workgroup per 8 * 256 buckets), at most per_cu for each of cus compute
    units"""
    per = sized_by or per_workgroup
    return max(1, min((n + per - 1) // per, per_cu * cus))


def trips(n, per_workgroup, per_cu, cus, sized_by=None, share=1):
    """the number of times the loop body of the launch's first lane runs (no other lane's runs more often): the grid takes
    workgroups() * per_workgroup elements per trip, times `share` where a lane takes that many elements a stride apart in
    one trip (jac_batch_normalise: TA_K = 8 points under one inversion)"""
    step = workgroups(n, per_workgroup, per_cu, cus, sized_by) * per_workgroup * share
    return (n + step - 1) // step


def shared_points(n, per_workgroup, per_cu, cus, share, lane=0):
    """how many of its `share` points the given lane holds in its first trip of such a loop"""
    stride = workgroups(n, per_workgroup, per_cu, cus) * per_workgroup
    return sum(1 for j in range(share) if lane + j * stride < n)
