"""The MSM's host side without a GPU: csrc/msm_plan.inc, compiled for the host (libhm_hostcheck.so), over everything the C ABI
accepts -- every size form below 2^31, every window hm_msm_set_window takes, every table group, every small group and every
setting of the three switches (tests/golden/gen_msm_plans.py holds the domain).

* pinned: one SHA-256 per family and the full rows of the shapes the tests and bench.py run (tests/golden/msm_plans.json);
* asserted on every row, whatever the golden says: the workspace regions are aligned, disjoint and as large as what their kernels
  index (the formulas below are written from the kernels' indexing, not from the carving), every dynamic LDS size fits what its
  kernel is allowed, every grid fits the launch limits, the chunks cover the items, every variant appears only where its
  preconditions hold, T_max is at least its stated bound, msm_window agrees with the plan and msm_table_group_max never admits a
  group the plan refuses;
* reachability: every variant of every stage that is left in the code is reached by some row."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import gen_msm_plans as g  # noqa: E402


@pytest.fixture(scope="module")
def pl():
    return g.Planner()


@pytest.fixture(scope="module")
def families(pl):
    return {name: gen(pl) for name, (gen, _) in g.FAMILIES.items()}


@pytest.fixture(scope="module")
def golden():
    with open(g.OUT) as f:
        return json.load(f)


class Rows:
    """columns of a family by name, as int64 (every value is below 2^63)"""

    def __init__(self, rows, columns):
        assert rows.max() < (1 << 63)
        self.a = rows.astype(np.int64)
        self.at = {c: i for i, c in enumerate(columns)}

    def __getitem__(self, name):
        return self.a[:, self.at[name]]

    def where(self, mask):
        r = Rows.__new__(Rows)
        r.a, r.at = self.a[mask], self.at
        return r

    def describe(self, i, names=("n", "group_in", "precomp_c", "override", "digits_count", "k3b_copy", "k4_wave_sums")):
        return {k: int(self[k][i]) for k in names if k in self.at}


def check(rows, ok, what):
    """every row satisfies `ok`; the message names the first that does not"""
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, f"{what}: {bad.size} rows, first {rows.describe(bad[0])}"


def enum(name, value):
    return g.ENUMS[name].index(value)


def planned(rows):
    """the rows the general pipeline plans (no error, not the five-launch chain)"""
    return rows.where((rows["err"] == 0) & (rows["route"] == enum("route", "general")))


# ---- pinned ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(g.FAMILIES))
def test_digest_of_every_row(families, golden, family):
    rows = families[family]
    assert {"rows": int(rows.shape[0]), "sha256": g.digest(family, rows)} == golden["families"][family]


def test_rows_of_the_shapes_the_tests_and_the_benchmark_run(pl, golden):
    assert g.pinned_rows(pl) == golden["pinned"]
    assert {f"{layout}_{n}" for layout, n in g.PINNED} <= set(golden["pinned"])


# ---- the general pipeline -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["plain", "table"])
def test_regions_are_aligned_and_disjoint(families, family):
    r = planned(Rows(families[family], g.PLAN_COLUMNS))
    off = np.stack([r[f"{x}.off"] for x in g.REGIONS], axis=1)
    size = np.stack([r[f"{x}.bytes"] for x in g.REGIONS], axis=1)
    check(r, (off % 256 == 0).all(axis=1), "a region is not 256-byte aligned")
    order = np.argsort(off, axis=1)
    o, s = np.take_along_axis(off, order, axis=1), np.take_along_axis(size, order, axis=1)
    check(r, (o[:, 1:] >= o[:, :-1] + s[:, :-1]).all(axis=1) & (s > 0).all(axis=1), "two regions overlap")
    check(r, r["ws_bytes"] >= o[:, -1] + s[:, -1], "the workspace ends before its last region")


def needs(r, c):
    """bytes every region's kernels index, from their launch parameters (the formulas beside the kernels in msm.hip)"""
    n, group, W, SW, NC, NBT, T = r["n"], r["group"], r["W"], r["SW"], r["NC"], r["NBT"], r["T_max"]
    pt = c["PT_WORDS"] * 4
    has1 = r["cb"] != 0
    item = np.where(r["item"] == enum("item", "u64"), 8, 4)
    chain = r["reduction"] == enum("reduction", "chain")
    coop = r["coop_sort"] != 0
    out1 = (r["nseg"] + c["SUM_SPAN"] - 1) // c["SUM_SPAN"]                  # outputs of the first msm_sum_points_kernel pass
    out2 = (out1 + c["SUM_SPAN"] - 1) // c["SUM_SPAN"]                       # ... of the second, written back over the segments
    return {
        "digits": W * n * 4 * group,                                           # digits[(e * W + w) * n + i]
        "chist": np.where(has1, SW * r["p1_scatter.gx"] * NC * 4, 0),          # [set][chunk][bin], a chunk per workgroup of the first level
        "ctot": np.where(has1, SW * NC * 4, 0),
        "cstart": np.where(has1, (SW * NC + 1) * 4, 0),                        # region starts, then the pair count
        "tmp": np.where(has1, SW * r["sn"] * item, 0),                         # every item of every set once
        "bcnt": NBT * 4, "boff": NBT * 4, "toff": (NBT + 1) * 4,
        "bsum": r["scan_partial.gx"] * 8,                                      # (pairs, tasks) per scan block
        "sorted": r["pairs_max"] * 4,
        "tb": T * 4, "torder": T * 4,
        "tkeys": 2 * c["TASK_KEYS"] * 4,
        "partial": T * pt,
        "bucket": NBT * pt,
        "seg": np.where(chain, np.maximum(SW * r["nseg"], SW * out2) * pt, SW * ((1 << r["k4_m"]) + (1 << r["k4_h"])) * pt),
        "seg2": np.where(chain & (r["sum_levels"] > 0), SW * out1 * pt, 0),
        "res": np.where(r["single_set"] != 0, group, 1) * (4 + r["RW"] * 32) * 4,
        "big": (NBT + 4) * 4,                                                  # two counters, padding, then at most a bucket each
        "slices": (T // c["FINALIZE_SLICE"] + T // (c["FINALIZE_SLICE"] + 1) + 1) * 8,   # ceil(cnt / SLICE) over buckets above SLICE partials
        "brlist": np.where(coop, r["br_capacity"] * 8, 0),
        "brcount": 4 + 0 * n,
        "gcur": np.where(coop, NBT * 4, 0),
    }


@pytest.mark.parametrize("family", ["plain", "table"])
def test_regions_hold_what_their_kernels_index(pl, families, family):
    r = planned(Rows(families[family], g.PLAN_COLUMNS))
    for name, need in needs(r, pl.constants).items():
        check(r, r[f"{name}.bytes"] >= need, f"region {name} is smaller than what its kernels index")
    check(r, r["res_bytes"] <= r["res.bytes"], "the result copy reads past its region")
    # the cooperative work list: every slice of every region above `big` items -- at most pairs / slice full slices and one partial
    # slice per such region, of which there are at most pairs / big
    coop = r.where(r["coop_sort"] != 0)
    check(coop, coop["br_capacity"] >= coop["pairs_max"] // coop["br_slice"] + coop["pairs_max"] // coop["br_big"] + 1, "work list too short")
    check(coop, coop["br_big"] == 4 * coop["br_slice"], "big regions are those above four slices")
    rest = r.where(r["coop_sort"] == 0)
    check(rest, rest["br_big"] == 0xFFFFFFFF, "a plan without the cooperative scatter must call no region big")


# Rows the plan has always produced that break the LDS rule, excluded BY NAME from that one assertion and from nothing else: the plain
# layout under hm_msm_set_window(21 or 22) between 2^24 and 2^26 points leaves 15 or 16 coarse bits, and msm_part1_hist_kernel and
# msm_part1_scatter_kernel (one LDS counter per coarse bin, no raised limit) are asked for 128 KiB, at 16 bits for 256 KiB -- more
# than a workgroup has.  (n, window override); every setting of the three switches gives the same plan there.
LDS_EXCESS_ROWS = {(16777217, 22), (16789561, 22), (25165824, 22), (33554431, 22), (33554432, 22), (33554433, 21), (33554433, 22),
                   (33566777, 21), (33566777, 22), (50331648, 21), (50331648, 22), (67108863, 21), (67108863, 22), (67108864, 21),
                   (67108864, 22)}
LDS_EXCESS_LAUNCHES = ("p1_hist", "p1_scatter")


@pytest.mark.parametrize("family", ["plain", "table"])
def test_launches_fit_the_lds_and_the_grid_limits(pl, families, family):
    r = planned(Rows(families[family], g.PLAN_COLUMNS))
    c = pl.constants
    listed = np.array([family == "plain" and (int(n), int(ov)) in LDS_EXCESS_ROWS for n, ov in zip(r["n"], r["override"])])
    seen = set()
    for name in g.LAUNCHES:
        used = r.where(r[f"{name}.gx"] > 0)
        fits = used[f"{name}.lds"] <= used[f"{name}.lds_cap"]
        if name in LDS_EXCESS_LAUNCHES:
            known = listed[r[f"{name}.gx"] > 0]
            seen |= {(int(n), int(ov)) for n, ov in zip(used["n"][known & ~fits], used["override"][known & ~fits])}
            fits = fits | known
        check(used, fits, f"{name}: dynamic LDS above what the kernel is allowed")
        check(used, np.isin(used[f"{name}.lds_cap"], [c["LDS_DEFAULT"], c["LDS_FINE"], c["LDS_ALL"]]), f"{name}: unknown LDS limit")
        check(used, (used[f"{name}.gx"] < (1 << 31)) & (used[f"{name}.gy"] >= 1) & (used[f"{name}.gy"] <= 65535), f"{name}: grid out of range")
        check(used, (used[f"{name}.block"] >= 64) & (used[f"{name}.block"] <= 1024) & (used[f"{name}.block"] % 64 == 0), f"{name}: block size")
    assert seen == (LDS_EXCESS_ROWS if family == "plain" else set())        # a listed row that came to fit must leave the list
    always = ("digits init p2_hist scan_partial scan_blocksums scan_final p2_scatter accumulate finalize finalize_slices finalize_big").split()
    for name in always:
        check(r, r[f"{name}.gx"] > 0, f"{name} is not launched")
    # the tightest case: the big-tile vector-load scatter at 2 048 coarse bins
    if family == "table":
        big = r.where((r["p1_scatter"] == enum("p1_scatter", "vec_big")) & (r["NC"] == 2048))
        assert big.a.shape[0] > 0
        assert int(big["p1_scatter.lds"].max()) == 155776 and int(big["p1_scatter.lds_cap"].min()) == 157696 == c["LDS_ALL"]


@pytest.mark.parametrize("family", ["plain", "table"])
def test_plan_invariants(pl, families, family):
    c = pl.constants
    r = planned(Rows(families[family], g.PLAN_COLUMNS))
    check(r, r["G"] * r["chunk"] >= r["sn"], "the chunks of the first level do not cover the items")
    check(r, r["NC"] == 1 << r["cb"], "NC")
    check(r, r["fb"] + r["cb"] == r["c"] - 1, "fine and coarse bits must add up to the bucket bits")
    check(r, r["NBT"] == r["SW"] * ((1 << (r["c"] - 1)) + 1), "NBT")
    check(r, r["pairs_max"] < (1 << 31), "more pairs than 31 bits index")
    check(r, r["L"] >= 16, "L")
    # T_max: the device may shorten L, then tasks <= 2 * TARGET_TASKS + one per bucket, and never more than one per pair
    bound = np.minimum(r["pairs_max"], np.maximum(r["pairs_max"] // r["L"], 2 * c["TARGET_TASKS"]) + r["NBT"])
    check(r, r["T_max"] >= bound, "T_max is below its stated bound")
    check(r, r["accumulate.gx"] * c["ACC_THREADS"] >= r["T_max"], "the accumulation grid does not cover T_max")
    # an item holds its fine bucket, a sign and its index (or, positional, the low bits of it) in its width
    u64, pos = r["item"] == enum("item", "u64"), r["item"] == enum("item", "u32_positional")
    check(r, np.where(r["cb"] != 0, r["fb"] + 1 + r["ib"] <= np.where(u64, 64, 32), True), "an item does not fit its word")
    check(r, pos | ((1 << r["ib"]) >= r["sn"]), "the index bits do not cover the items")
    check(r, r["fb"] <= 15, "more fine counters than a workgroup's LDS holds")
    # positional plans
    p = r.where(pos)
    check(p, (p["ps_nsc"] >= 1) & (p["ps_nsc"] <= c["PS_MAX_SC"]) & (p["sbits"] >= 16) & (p["ib"] == p["sbits"]) & (p["fb"] <= 12), "positional plan")
    check(p, (p["single_set"] != 0) & (p["ps_G"] == p["G"]) & (p["ps_gpc"] * p["chunk"] == 1 << p["sbits"]) & (p["G"] <= 4096)
          & (p["ps_nsc"] << p["sbits"] >= p["sn"]), "positional chunks")
    check(p, p["p2_scatter"] == enum("p2_scatter", "vec"), "positional items need the vector-load second level")
    check(r.where(~pos), r.where(~pos)["ps_nsc"] == 0, "super-chunks without positional items")
    # variants against item widths
    check(r, (r["p1_scatter"] == enum("p1_scatter", "none")) == (r["cb"] == 0), "first-level scatter against cb")
    check(r, (r["first_level"] == enum("first_level", "none")) == (r["cb"] == 0), "first level against cb")
    check(r, np.isin(r["p1_scatter"], [enum("p1_scatter", "vec"), enum("p1_scatter", "vec_big")]) <= ~u64, "vector-load scatter with 64-bit items")
    check(r, (r["p1_scatter"] == enum("p1_scatter", "tiled")) <= u64, "tiled first-level scatter with 32-bit items")
    check(r, (r["p2_scatter"] == enum("p2_scatter", "tiled")) <= u64, "tiled second-level scatter with 32-bit items")
    check(r, (r["p2_scatter"] == enum("p2_scatter", "vec")) <= ~u64, "vector-load second level with 64-bit items")
    check(r, (r["p2_scatter"] == enum("p2_scatter", "digits")) == (r["cb"] == 0), "second level from the digits against cb")
    check(r, np.isin(r["p2_scatter"], [enum("p2_scatter", "tiled"), enum("p2_scatter", "vec")]) == (r["coop_sort"] != 0), "cooperative scatter")
    check(r, (r["tasks"] == enum("tasks", "fill")) == (r["pairs_max"] < (1 << 19)), "task ordering")
    # the counting digits form: only where its stated preconditions hold, never against its switch, by default where it fills the chip
    valid = (r["single_set"] != 0) & (r["cb"] != 0) & ~u64 & (r["n"] % r["chunk"] == 0) & (r["G"] * r["chunk"] == r["sn"]) & (r["W"] * r["NC"] * 4 <= 48 * 1024)
    counting = r["digits"] == enum("digits", "counting")
    check(r, counting <= valid, "the counting digits form outside its preconditions")
    sw = r["digits_count"] - 1
    check(r, np.where(sw == 0, ~counting, True) & np.where(sw == 1, counting == valid, True), "the counting digits form against its switch")
    check(r, np.where(sw == -1, counting == (valid & ((r["n"] // r["chunk"]) * r["group"] >= 256)), True), "the counting digits form's default")
    check(r, counting == (r["first_level"] == enum("first_level", "counted")), "counted first level without the counting digits")
    check(r.where(counting), r.where(counting)["digits.gx"] * r.where(counting)["chunk"] == r.where(counting)["n"], "counting digits grid")
    # the reduction
    chain = r["reduction"] == enum("reduction", "chain")
    check(r, chain == ~((r["single_set"] != 0) & (r["NB"] >= 16)), "a shared set of 16 buckets or more takes the two-launch reduction")
    check(r, (r["direct_buckets"] != 0) == (~chain & (r["k3b_copy"] - 1 != 1)), "direct bucket reads")
    check(r, (r["k4_m"] + r["k4_h"] == r["c"] - 1) & (r["RW"] <= 128), "row / column split")
    wave = r["reduction"] == enum("reduction", "rowcol_wave")
    sw = r["k4_wave_sums"] - 1
    check(r, np.where(~chain & (sw >= 0), wave == (sw == 1), True), "one-wave sums against their switch")
    check(r, np.where(~chain & (sw < 0), wave == (((1 << r["k4_h"]) + (1 << (r["k4_m"] - 1))) * r["SW"] >= 2048), True), "one-wave sums' default")


def test_window_and_errors_on_the_plain_layout(pl, families):
    r = Rows(families["plain"], g.PLAN_COLUMNS)
    live = r.where(r["route"] != enum("route", "empty"))
    want = np.array([pl.window(int(n), 0, 0, int(ov))[0] for n, ov in zip(live["n"], live["override"])])
    check(live, live["c"] == want, "msm_window disagrees with the plan")
    check(live, np.where(live["override"] > 0, live["c"] == live["override"], True), "the override must win")
    small = live["route"] == enum("route", "small")
    check(live, small == ((live["n"] < (1 << 19)) & (live["c"] <= 15)), "route")
    # the only refusal: more (point, window) pairs than 31 bits index
    W = (255 + live["c"] - 1) // live["c"]
    check(live, (live["err"] != 0) == (~small & (live["n"] * W >= (1 << 31))), "unexpected refusal")
    check(live, np.isin(live["err"], [0, 1]), "error code")
    # the three switches belong to the shared bucket set: a plain plan never moves with them
    key = np.stack([live["n"], live["override"]], axis=1)
    base = live.where((live["digits_count"] == 0) & (live["k3b_copy"] == 0) & (live["k4_wave_sums"] == 0))
    lookup = {tuple(k): row[7:] for k, row in zip(np.stack([base["n"], base["override"]], axis=1).tolist(), base.a)}
    assert all(np.array_equal(lookup[tuple(k)], row[7:]) for k, row in zip(key.tolist(), live.a))


def test_table_groups_are_never_refused(pl, families):
    r = Rows(families["table"], g.PLAN_COLUMNS)
    check(r, (r["err"] == 0) & (r["route"] == enum("route", "general")), "msm_table_group_max admitted what msm_plan refuses")
    check(r, r["c"] == r["precomp_c"], "a table set carries its window")
    check(r, (r["SW"] == r["group_in"]) & (r["single_set"] == 1), "a bucket set per element")
    # and the next larger group is refused by the group rule, not by a later launch
    for n in (1000, 1 << 12, 1 << 17, (1 << 18) + 1):
        c = pl.window(n)[2]
        gmax = pl.window(n, c)[3]
        assert 1 <= gmax <= pl.constants["GROUP_MAX"]
        assert (gmax + 1) * n * ((255 + c - 1) // c) >= (1 << 31) or (gmax + 1) * n * ((255 + c - 1) // c) * 4 > (3 << 30) or gmax == 8
    assert pl.window(1 << 19, pl.window(1 << 19)[2])[3] == 1


# ---- the five-launch chain -----------------------------------------------------------------------------------------------------------
def test_small_plans(pl, families):
    c = pl.constants
    r = Rows(families["small"], g.SMALL_COLUMNS)
    check(r, r["err"] == 0, "refused")
    want = np.array([pl.window(int(n), 0, int(live), int(ov))[1] for n, live, ov in zip(r["n"], r["live_rows"], r["override"])])
    check(r, r["c"] == want, "window")
    off = np.stack([r[f"{x}.off"] for x in g.SMALL_REGIONS], axis=1)
    size = np.stack([r[f"{x}.bytes"] for x in g.SMALL_REGIONS], axis=1)
    check(r, (off % 256 == 0).all(axis=1) & (r["ws_stride"] % 256 == 0), "alignment")
    check(r, (off[:, 1:] >= off[:, :-1] + size[:, :-1]).all(axis=1) & (size > 0).all(axis=1), "two regions overlap")
    per_element = len(g.SMALL_REGIONS) - 2
    check(r, off[:, per_element - 1] + size[:, per_element - 1] <= r["ws_stride"], "an element's arrays leave its stride")
    check(r, r["res.off"] >= r["ws_stride"] * r["group"], "the results overlap the last element's arrays")
    check(r, r["ws_bytes"] >= r["live.off"] + r["live.bytes"], "the workspace ends before the survivor counters")
    n, W, V, NBh, T = r["n"], r["W"], r["V"], r["NBh"], r["T_max"]
    blocks = (n + c["SA_THREADS"] - 1) // c["SA_THREADS"]
    need = {"digits": blocks * c["SA_THREADS"] * W * 4, "toff": V * (NBh + 1) * 4, "gctr": 8, "nz": V * NBh * 4, "nzc": V * 4, "desc": T * 16,
            "sorted": r["pairs_max"] * 4, "partial": T * c["PT_WORDS"] * 4, "seg1": V * r["G1n"] * c["PT_WORDS"] * 4, "blkidx": blocks * 4,
            "res": r["group"] * (4 + W * 32) * 4, "live": c["GROUP_MAX"] * 4}
    for name, b in need.items():
        check(r, r[f"{name}.bytes"] >= b, f"region {name} is smaller than what its kernels index")
    check(r, (r["wide"] <= r["c"]) & (r["NB"] == 1 << (r["wide"] - 1)) & (r["H"] * NBh == r["NB"]) & (V == W * r["H"]) & (W <= 128), "windows")
    check(r, r["n_wide"] * r["wide"] + (W - r["n_wide"]) * (r["wide"] - 1) == 255, "the windows cover the 255 digit bits")
    check(r, (r["L"] >= 2) & (r["L"] <= c["S_MAX_L"]), "L")
    check(r, T >= r["pairs_max"] // r["L"] + V * NBh, "T_max is below its stated bound")       # sum of ceil(cnt / L) <= pairs / L + buckets
    check(r, (r["nseg"] * r["SEG"] >= NBh) & (r["G1n"] * c["WIN_THREADS"] >= r["nseg"]), "segments")
    check(r, (r["lds_sort"] <= r["lds_sort_cap"]) & (r["lds_sort"] >= (NBh + 1 + 2 * c["S_TASK_KEYS"]) * 4), "sort LDS")
    for name in g.SMALL_LAUNCHES:
        check(r, (r[f"{name}.gx"] >= 1) & (r[f"{name}.gx"] < (1 << 31)) & (r[f"{name}.gy"] >= 1) & (r[f"{name}.gy"] <= 65535)
              & (r[f"{name}.gz"] >= 1) & (r[f"{name}.gz"] <= 65535), f"{name}: grid out of range")
    check(r, r["accumulate.gx"] * c["ACC_THREADS"] >= T, "the accumulation grid does not cover T_max")


# ---- reachability --------------------------------------------------------------------------------------------------------------------
# The kernel instantiations of the sort are chosen by (item, first level, first-level scatter, second-level scatter).  This is the
# whole set the sweep reaches: msm.hip's launch_sort / launch_sort_scatter hold a branch, and msm_set_lds_attributes a row, for these
# and for nothing else -- 64-bit items (plain sets above 2^26 points) come in ONE combination, so the kernels of the other forms
# have no 64-bit instantiation.  (Which kernels that attribute table names is host code of msm.hip that no second compiler reads:
# the LDS test above checks each launch against the limit the PLAN states for it, not that table.)
SORT_COMBINATIONS = {
    ("u32", "none", "none", "digits"),
    ("u32", "hist", "vec", "direct"), ("u32", "hist", "vec", "vec"), ("u32", "hist", "vec_big", "direct"), ("u32", "hist", "vec_big", "vec"),
    ("u32", "hist", "direct", "vec"), ("u32", "counted", "vec", "vec"),
    ("u32_positional", "hist", "vec_big", "vec"), ("u32_positional", "counted", "vec_big", "vec"),
    ("u64", "hist", "tiled", "tiled"),
}


def test_every_variant_left_in_the_code_is_reached(pl, families):
    rows = np.concatenate([families["plain"], families["table"], pl.plan_row(0, 1, 0)[None, :]])      # n = 0: the empty route
    everything = Rows(rows, g.PLAN_COLUMNS)
    empty = everything.where(everything["n"] == 0)
    assert empty.a.shape[0] == 1 and empty["route"][0] == enum("route", "empty") and empty["err"][0] == 0 and empty["ws_bytes"][0] == 0
    assert all(empty[f"{name}.gx"][0] == 0 for name in g.LAUNCHES)                 # nothing is launched for no points
    r = planned(everything)
    reached = {"route": sorted({g.ENUMS["route"][v] for v in np.unique(everything["route"])})}
    for stage in ("digits", "first_level", "p1_scatter", "p2_scatter", "item", "tasks", "reduction"):
        reached[stage] = sorted({g.ENUMS[stage][v] for v in np.unique(r[stage])})     # a value outside the enum is an IndexError
    print("variants reached:", json.dumps(reached))
    for stage, names in g.ENUMS.items():
        assert reached[stage] == sorted(names), stage
    combos = {tuple(g.ENUMS[k][v] for k, v in zip(("item", "first_level", "p1_scatter", "p2_scatter"), t))
              for t in np.unique(np.stack([r["item"], r["first_level"], r["p1_scatter"], r["p2_scatter"]], axis=1), axis=0).tolist()}
    print("sort combinations reached:", sorted(combos))
    assert combos == SORT_COMBINATIONS
