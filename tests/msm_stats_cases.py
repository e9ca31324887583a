"""The MSM routes that tests/test_msm_gpu.py pins against the parent of the plan refactor: one case per route of the launch plan
(csrc/msm_plan.inc), at the smallest shape that takes it.  tests/golden/gen_msm_stats_parent.py runs the same cases on a library
built from the parent commit and records `pairs` and `tasks` of hm_get_msm_stats: both move if the task length L or the task
bound T_max of the plan drift.

A case is (n, layout, columns): layout "plain" registers one copy of the points, "table" lets the library build the fixed-base
table (from 2^17 points); columns > 1 is one best_multiexp_batch call of that many dense columns."""

SEED = 0x6D736D706C616E01        # of bench.bench_inputs
EXTRA = 77                       # the columns of a group are shifted / flipped views of n + EXTRA scalars

CASES = {
    "small_plan_1000": (1000, "plain", 1),
    "small_group_of_three_4096": (1 << 12, "plain", 3),
    "general_plain_2p19_77": ((1 << 19) + 77, "plain", 1),
    "table_2p17": (1 << 17, "table", 1),
    "table_2p17_group_of_three": (1 << 17, "table", 3),
    "table_2p20": (1 << 20, "table", 1),
}


def run_case(name):
    """-> (results (columns, 12) u64, closed forms (columns, 12) u64, msm_stats() after the call)."""
    import numpy as np
    import torch
    import bench
    import halo2_experiments_amd as h
    n, layout, columns = CASES[name]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    s, bases, t = bench.bench_inputs(n + EXTRA, 0, SEED, dev)
    t = t[:n].contiguous()
    cols = [s[:n].contiguous(), s[EXTRA: EXTRA + n].contiguous(), s[:n].flip(0).contiguous()][:columns]
    exp = np.stack([bench.known_answer(c, t, dev) for c in cols])
    handle = h.register_bases(bases[:n].contiguous(), plain=layout == "plain")
    try:
        got = h.best_multiexp(cols[0], handle)[None, :] if columns == 1 else h.best_multiexp_batch(cols, handle)
        stats = h.msm_stats()
    finally:
        h.release_bases(handle)
    return got, exp, stats
