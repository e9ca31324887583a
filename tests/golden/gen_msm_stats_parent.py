"""Writes tests/golden/msm_stats_parent.json: `pairs` and `tasks` of hm_get_msm_stats for every case of tests/msm_stats_cases.py.

Run it on an MI355X against a library built from the PARENT of the commit that introduced csrc/msm_plan.inc (7da210b), so that
the file records what the launch plan gave before it became a function of its own:

    git worktree add /tmp/parent 7da210b && make -C /tmp/parent/halo2-experiments_amd/csrc libhalo2_mi355x.so
    HALO2_MI355X_LIB=/tmp/parent/halo2-experiments_amd/csrc/libhalo2_mi355x.so python tests/golden/gen_msm_stats_parent.py [OUT]

Every result is checked against the closed form before anything is written."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import msm_stats_cases as cases
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "msm_stats_parent.json")
    rows = {}
    for name in cases.CASES:
        got, exp, st = cases.run_case(name)
        assert np.array_equal(got, exp), name
        rows[name] = {k: int(st[k]) for k in ("pairs", "tasks", "window_bits", "windows")}
        print(name, rows[name], flush=True)
    with open(out, "w") as f:
        json.dump({"parent": "7da210b", "cases": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
