"""The MSM's launch plans (csrc/msm_plan.inc through libhm_hostcheck.so) over everything the C ABI accepts, and
tests/golden/msm_plans.json: one SHA-256 per family over every row, and the full rows of the shapes the tests and bench.py run.

    python tests/golden/gen_msm_plans.py          # rewrites tests/golden/msm_plans.json

A row is its inputs followed by the plan: unsigned 64-bit words.  A family's digest is the SHA-256 of the ASCII header
"<family> <rows> <words per row>\\n" followed by the rows' words as 16 lower-case hexadecimal digits each, least significant byte
first, row after row.  tests/test_msm_plan_host.py imports this module for the domain, the field names and the digests.

The file was recorded from the tree in which the host code of msm.hip and msm_small.hip had been moved into msm_plan.inc expression
for expression, every later-retired switch still a field of MsmKnobs at its default; retiring them left every digest as it is.  One
column was not the parent's at that state: the LDS limit of the tiled second-level scatter's two launches, a limit the parent never
raised and the commit that added msm_plan.inc does."""
import ctypes
import hashlib
import itertools
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "msm_plans.json")

# the order of the scalars in hc_msm_plan / hc_msm_small_plan (csrc/host_check.cpp)
PLAN_FIELDS = ("route single_set group c W n_wide SW sn NB NBP NBT pairs_max L G chunk T_max SEG nseg k4_m k4_h RW res_stride ib fb cb NC "
               "ps_G ps_gpc ps_nsc sbits br_big br_slice br_capacity coop_sort direct_buckets digits first_level p1_scatter p2_scatter item "
               "tasks reduction sum_levels sum_count0 sum_count1 sum_count2 sum_count3 res_bytes ws_bytes").split()
REGIONS = ("digits chist ctot cstart tmp bcnt boff toff bsum sorted tb torder tkeys partial bucket seg seg2 res big slices brlist brcount "
           "gcur").split()
LAUNCHES = ("digits init p1_hist p1_scan p1_starts p1_scatter big_regions p2_hist p2_hist_coop scan_partial scan_blocksums scan_final "
            "p2_scatter p2_scatter_coop task_fill task_hist task_keyscan task_order accumulate finalize finalize_slices finalize_big rowcol "
            "bits segments sum_0 sum_1 sum_2 sum_3 to_ext").split()
LAUNCH_FIELDS = ("gx", "gy", "block", "lds", "lds_cap")
SMALL_FIELDS = "group W wide n_wide NB pairs_max H NBh V L SEG nseg G1n T_max ws_stride res_stride ws_bytes lds_sort lds_sort_cap".split()
SMALL_REGIONS = "digits toff gctr nz nzc desc sorted partial seg1 blkidx res live".split()
SMALL_LAUNCHES = "digits sort accumulate reduce1 reduce2".split()
CONSTANTS = ("PT_WORDS ACC_THREADS WIN_THREADS TARGET_TASKS SORT_THREADS P1_IPT P1_BIG_IPT P2_TILE PS_MAX_SC SCAN_BLOCK TASK_KEYS "
             "FINALIZE_SERIAL FINALIZE_SLICE SUM_SPAN SA_THREADS S_TASK_KEYS S_MAX_L GROUP_MAX LDS_DEFAULT LDS_FINE LDS_ALL").split()
# the variants of every stage, by the enums of msm_plan.inc
ENUMS = {
    "route": ("empty", "small", "general"),
    "digits": ("plain", "counting"),
    "first_level": ("none", "hist", "counted"),
    "p1_scatter": ("none", "vec", "vec_big", "tiled", "direct"),
    "p2_scatter": ("digits", "direct", "tiled", "vec"),
    "item": ("u32", "u32_positional", "u64"),
    "tasks": ("fill", "ordered"),
    "reduction": ("chain", "rowcol", "rowcol_wave"),
}

PLAN_INPUTS = ("n", "group_in", "precomp_c", "override", "digits_count", "k3b_copy", "k4_wave_sums", "err")
PLAN_COLUMNS = list(PLAN_INPUTS) + PLAN_FIELDS + [f"{r}.{f}" for r in REGIONS for f in ("off", "bytes")] + \
    [f"{l}.{f}" for l in LAUNCHES for f in LAUNCH_FIELDS]
SMALL_INPUTS = ("n", "group_in", "live_rows", "override", "c", "err")
SMALL_COLUMNS = list(SMALL_INPUTS) + SMALL_FIELDS + [f"{r}.{f}" for r in SMALL_REGIONS for f in ("off", "bytes")] + \
    [f"{l}.{f}" for l in SMALL_LAUNCHES for f in ("gx", "gy", "gz")]

u64p, u32p, i64p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int64)


def load():
    from halo2_experiments_amd import _lib
    if not os.path.exists(_lib.HOSTCHECK_PATH):
        subprocess.run(["make", "-C", _lib.CSRC, "libhm_hostcheck.so"], check=True, capture_output=True)
    lib = ctypes.CDLL(_lib.HOSTCHECK_PATH)
    lib.hc_msm_window.restype = None
    lib.hc_msm_window.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64, i64p, u64p]
    lib.hc_msm_plan.restype = ctypes.c_int
    lib.hc_msm_plan.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, i64p, u64p, u32p]
    lib.hc_msm_small_plan.restype = ctypes.c_int
    lib.hc_msm_small_plan.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, u64p, u32p]
    lib.hc_msm_constants.restype = None
    lib.hc_msm_constants.argtypes = [u64p]
    return lib


class Planner:
    def __init__(self):
        self.lib = load()
        self.buf = np.zeros(1024, dtype=np.uint64)
        self.counts = np.zeros(3, dtype=np.uint32)
        c = np.zeros(len(CONSTANTS), dtype=np.uint64)
        self.lib.hc_msm_constants(c.ctypes.data_as(u64p))
        self.constants = dict(zip(CONSTANTS, (int(x) for x in c)))

    @staticmethod
    def knobs(override=0, switches=(-1, -1, -1)):
        return np.array([override, *switches], dtype=np.int64)

    def window(self, n, precomp_c=0, live_rows=0, override=0):
        """-> (msm_window, the five-launch chain's window or 0, msm_precomp_window(n), msm_table_group_max(n, precomp_c))"""
        out = np.zeros(4, dtype=np.uint64)
        self.lib.hc_msm_window(n, precomp_c, live_rows, self.knobs(override).ctypes.data_as(i64p), out.ctypes.data_as(u64p))
        return tuple(int(x) for x in out)

    def plan_row(self, n, group, precomp_c, override=0, switches=(-1, -1, -1)):
        err = self.lib.hc_msm_plan(n, group, precomp_c, self.knobs(override, switches).ctypes.data_as(i64p), self.buf.ctypes.data_as(u64p),
                                   self.counts.ctypes.data_as(u32p))
        assert tuple(self.counts) == (len(PLAN_FIELDS), len(REGIONS), len(LAUNCHES)), tuple(self.counts)
        head = [n, group, precomp_c, override, *(s + 1 for s in switches), -err]
        return np.concatenate([np.array(head, dtype=np.uint64), self.buf[: len(PLAN_COLUMNS) - len(head)]])

    def small_row(self, n, group, live_rows, override, c):
        err = self.lib.hc_msm_small_plan(n, group, c, self.buf.ctypes.data_as(u64p), self.counts.ctypes.data_as(u32p))
        assert tuple(self.counts) == (len(SMALL_FIELDS), len(SMALL_REGIONS), len(SMALL_LAUNCHES)), tuple(self.counts)
        head = [n, group, live_rows, override, c, -err]
        return np.concatenate([np.array(head, dtype=np.uint64), self.buf[: len(SMALL_COLUMNS) - len(head)]])


def sizes():
    """2^k, 2^k +- 1, 3 * 2^(k - 1) and 2^k + 12 345 for k = 0 .. 30, below 2^31"""
    out = set()
    for k in range(31):
        out.update((1 << k, (1 << k) - 1, (1 << k) + 1, 3 * (1 << k) // 2, (1 << k) + 12345))
    return sorted(n for n in out if 1 <= n < (1 << 31))


SWITCHES = list(itertools.product((-1, 0, 1), repeat=3))
OVERRIDES = [0] + list(range(2, 23))


def plain_rows(pl):
    """the plain layout: every size, every window hm_msm_set_window accepts, every setting of the three switches"""
    return np.stack([pl.plan_row(n, 1, 0, ov, sw) for n in sizes() for ov in OVERRIDES for sw in SWITCHES])


def table_rows(pl):
    """the table layout: precomp_c = msm_precomp_window(n) where n * W < 2^31; groups from 1 up to msm_table_group_max"""
    rows = []
    for n in sizes():
        c = pl.window(n)[2]
        if n * ((255 + c - 1) // c) >= (1 << 31):
            continue
        for group in range(1, pl.window(n, c)[3] + 1):
            rows.extend(pl.plan_row(n, group, c, 0, sw) for sw in SWITCHES)
    return np.stack(rows)


def small_rows(pl):
    """the five-launch chain: groups of 1 .. 8 with live_rows in {0, n / 256, n}, and single MSMs under every override it takes"""
    rows = []
    for n in sizes():
        if n >= (1 << 19):
            continue
        for live in sorted({0, n // 256, n}):
            c = pl.window(n, 0, live)[1]
            assert c != 0
            rows.extend(pl.small_row(n, group, live, 0, c) for group in range(1, 9))
        for ov in OVERRIDES[1:]:
            c = pl.window(n, 0, 0, ov)[1]
            if c:
                rows.append(pl.small_row(n, 1, 0, ov, c))
    return np.stack(rows)


FAMILIES = {"small": (small_rows, SMALL_COLUMNS), "plain": (plain_rows, PLAN_COLUMNS), "table": (table_rows, PLAN_COLUMNS)}
# the shapes the tests and bench.py run: (layout, n)
PINNED = [("table", 1000), ("table", 1 << 12), ("table", 1 << 17), ("table", (1 << 19) + 77), ("table", 1 << 20), ("table", (1 << 20) + 12345),
          ("table", 1 << 24), ("plain", 1 << 24)]


def digest(family, rows):
    h = hashlib.sha256(f"{family} {rows.shape[0]} {rows.shape[1]}\n".encode())
    h.update(np.ascontiguousarray(rows, dtype="<u8").tobytes().hex().encode())
    return h.hexdigest()


def pinned_rows(pl):
    """{name: {column: value}}: on the table the registration's own window, on the plain layout the default one; a size that
    routes to the five-launch chain (a table set is never that small in practice) is pinned as that chain's plan as well"""
    out = {}
    for layout, n in PINNED:
        pc = pl.window(n)[2] if layout == "table" else 0
        row = pl.plan_row(n, 1, pc)
        out[f"{layout}_{n}"] = dict(zip(PLAN_COLUMNS, (int(x) for x in row)))
        c_small = pl.window(n)[1]
        if c_small:
            out[f"small_{n}"] = dict(zip(SMALL_COLUMNS, (int(x) for x in pl.small_row(n, 1, 0, 0, c_small))))
    return out


def record(pl=None):
    pl = pl or Planner()
    fam = {}
    for name, (gen, columns) in FAMILIES.items():
        rows = gen(pl)
        assert rows.shape[1] == len(columns)
        fam[name] = {"rows": int(rows.shape[0]), "sha256": digest(name, rows)}
    return {"families": fam, "pinned": pinned_rows(pl)}


if __name__ == "__main__":
    with open(OUT, "w") as f:
        json.dump(record(), f, indent=1)
        f.write("\n")
    print(json.dumps(record()["families"], indent=1))
