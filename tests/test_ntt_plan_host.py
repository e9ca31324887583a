"""The NTT's host side without a GPU: csrc/ntt_plan.inc's ``ntt_check_call`` and ``ntt_plan``, the two pure functions the one driver
(ntt.hip: ntt_run) asks before it takes a stream slot, through libhm_hostcheck.so.

* the plan against a Python restatement of what it replaced -- ``plan_digits``, the table choices of ``ntt_get_tables``, the pass loop of
  ``ntt_run`` and the four coset run functions in front of it, as they stood before the plan -- over log_n 0..28 x batch {1, 2, 3, 48,
  65535} x cosets {0, 1, 2, 16} x log_z 0..min(log_n, 12) x every form the C entries make x in place / out of place, restricted to the
  calls the check admits;
* the invariants of every such row, among them that the largest twiddle index the pass kernel forms (its indexing is restated here) lies
  inside the table the plan hands it;
* the refusal table: every row tests/test_capi.py, tests/test_ntt_gpu.py and the domain tests send that this check decides, and the order
  in which two broken rules are reported;
* the same sweep in a stand-alone program (tests/ntt_plan_host.cpp) built with AddressSanitizer and UBSan."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import graph_programs as gp
from halo2_experiments_amd import _lib

LOG_TILE, DIRECT_LOG, TWO_PASS_MAX = 11, 21, 21
SCALE, COSET3, POST3, IN_TABLE, IN_TABLES, OUT_TABLE, OUT_TABLES = 1, 2, 4, 8, 16, 32, 64
PLAIN, FUSED, TABLE = 0, 1, 2
INPUT, ARRAY, SCRATCH = 0, 1, 2
LOG_NS = range(29)
BATCHES = (1, 2, 3, 48, 65535)
COSETS = (0, 1, 2, 16)
# what the C entries make: hm_ntt / hm_ntt_batch (scale and coset optional) / hm_ifft / hm_coset_ntt, hm_extended_to_coeff,
# hm_coeff_to_extended (with log_z), hm_coeff_to_coset, hm_coeff_to_cosets, hm_coset_to_coeff, hm_cosets_to_coeff
FORMS = (0, SCALE, COSET3, SCALE | COSET3, SCALE | POST3, IN_TABLE, IN_TABLES, SCALE | OUT_TABLE, SCALE | OUT_TABLES)
OUT, IN = (1 << 56) + 0x1000, 0x1000             # aligned, 2^56 apart (65535 arrays of 2^28 are 2^49 bytes); nothing is ever read through them
HEAD = ("log_n", "s", "log_stride", "log_c", "last", "log_r0", "log_rows", "log_lb", "fin_mode", "has_coset", "direct_tw", "log_z", "has_table")
PASS = HEAD + ("variant", "gx", "gy", "gz", "src", "dst", "stage", "tw_lo", "tw_hi")


@pytest.fixture(scope="module")
def hc():
    lib = gp.hostcheck()
    lib.hc_ntt_check_call.restype = ctypes.c_char_p
    lib.hc_ntt_plan.restype = None
    return lib


def words(log_n=10, batch=1, fwd=0, inv=0, log_z=0, fused=0, in_place=True, at_in=IN, at_out=OUT):
    return np.array([log_n, batch, fwd, inv, log_z, fused, int(in_place), at_in, at_out], dtype=np.uint64)


def check(hc, **kw):
    why = hc.hc_ntt_check_call(words(**kw).ctypes.data_as(ctypes.c_void_p))
    return None if why is None else why.decode()


class Buffers:
    def __init__(self):
        self.head, self.passes, self.tables = np.zeros(12, np.uint64), np.zeros((3, 22), np.int64), np.zeros((6, 3), np.uint64)
        self.ptr = [a.ctypes.data_as(ctypes.c_void_p) for a in (self.head, self.passes, self.tables)]


def plan(hc, buf, call):
    hc.hc_ntt_plan(call.ctypes.data_as(ctypes.c_void_p), *buf.ptr)
    h = [int(x) for x in buf.head]
    p = dict(passes=h[0], digits=h[1:4], arrays=h[4], lds_bytes=h[5], scratch_bytes=h[6], tail=h[7], tail_grid=h[8:10], table_bytes=h[10])
    p["tables"] = [tuple(int(x) for x in row) for row in buf.tables[:h[11]]]
    p["pass"] = [dict(zip(PASS, (int(x) for x in buf.passes[i]))) for i in range(h[0])]
    return p


# ---- the host side as it stood before the plan, each part in its own words ---------------------------------------------------------
def plan_digits_before(log_n):
    if log_n <= LOG_TILE:
        return [log_n]
    passes = 2 if log_n <= TWO_PASS_MAX else 3
    rem, digits = log_n, []
    for p in range(passes):
        digits.append((rem + (passes - p) - 1) // (passes - p))
        rem -= digits[-1]
    if passes == 2 and digits[0] > digits[1]:
        digits.reverse()
    return digits


def tables_before(log_n):
    """ntt_get_tables: name -> (count, shift)"""
    digits = plan_digits_before(log_n)
    passes, log_lb, t = len(digits), (log_n + 1) // 2, {}
    if passes > 1:
        if log_n <= DIRECT_LOG and passes == 2:
            t["lo"] = (1 << log_n, 0)
        else:
            t["lo"] = (1 << log_lb, 0)
            t["hi"] = (1 << (log_n - log_lb), log_lb)
            log_m1 = log_n - digits[0]
            if passes == 3 and log_m1 <= DIRECT_LOG:
                t["mid"] = (1 << log_m1, digits[0])
    for s in digits:
        t.setdefault(("stage", s), (1 if s == 0 else 1 << (s - 1), log_n - s))
    return t


def ntt_run_before(log_n, batch, fused, n_in_scales, d_in_scale, d_in, log_z):
    """the pass loop of ntt_run -> [(head, variant, grid, src, dst, name of the tw_lo table)], scratch bytes"""
    cosets, in_batch = n_in_scales, batch
    if cosets:
        batch *= cosets
    digits, tabs = plan_digits_before(log_n), tables_before(log_n)
    passes, n = len(digits), 1 << log_n
    fin_mode = 2 if fused & POST3 else 1 if fused & SCALE else 0
    log_stride, rows = log_n, []
    for p in range(passes):
        h = dict.fromkeys(HEAD, 0)
        h["log_n"], h["s"] = log_n, digits[p]
        log_stride -= digits[p]
        h["log_stride"], h["last"], h["log_lb"], h["log_rows"] = log_stride, int(p == passes - 1), (log_n + 1) // 2, log_n - digits[p]
        h["log_r0"] = digits[0] if h["last"] and passes == 3 else 0
        h["fin_mode"] = fin_mode if h["last"] else 0
        h["has_coset"] = int(p == 0 and bool(fused & COSET3))
        h["log_z"] = log_z if p == 0 and d_in else 0
        h["has_table"] = int(p == 0 and bool(d_in_scale or cosets))
        log_c = LOG_TILE - h["s"] if LOG_TILE > h["s"] else 0
        h["log_c"] = min(log_c, h["log_rows"] if h["last"] else h["log_stride"])
        tiles = n >> (h["s"] + h["log_c"])
        src = (INPUT if d_in else ARRAY) if p == 0 else SCRATCH
        dst = ARRAY if p == passes - 1 else SCRATCH
        lo = "lo"
        if not h["last"]:
            if log_n <= DIRECT_LOG and passes == 2:
                h["direct_tw"] = 1
            elif p == 1 and "mid" in tabs:
                h["direct_tw"], lo = 1, "mid"
        if h["has_table"]:
            variant, grid = TABLE, (tiles, in_batch, cosets if cosets else 1)
        elif h["has_coset"] | h["fin_mode"]:
            variant, grid = FUSED, (tiles, batch, 1)
        else:
            variant, grid = PLAIN, (tiles, batch, 1)
        rows.append((h, variant, grid, src, dst, lo))
    return rows, (n * 32 * batch if passes > 1 else 0)


def entries_before(log_n, batch, cosets, log_z, fused, in_place):
    """the run function each form went through -> ntt_run's rows, the scratch bytes, the trailing launch (kind, grid) and the arrays"""
    n = 1 << log_n
    if fused & IN_TABLE:                                       # ntt_coset_run
        return ntt_run_before(log_n, batch, 0, 0, True, not in_place, 0) + (None, batch)
    if fused & IN_TABLES:                                      # ntt_cosets_run
        return ntt_run_before(log_n, batch, 0, cosets, False, True, 0) + (None, batch * cosets)
    if fused & OUT_TABLE:                                      # ntt_coset_inverse_run
        return ntt_run_before(log_n, batch, SCALE, 0, False, False, 0) + ((1, ((n + 255) // 256, batch)), batch)
    if fused & OUT_TABLES:                                     # ntt_cosets_inverse_run
        return ntt_run_before(log_n, cosets, SCALE, 0, False, False, 0) + ((2, ((n + 255) // 256, cosets)), cosets)
    return ntt_run_before(log_n, batch, fused, 0, False, not in_place, log_z) + (None, batch)


def sweep():
    """every call of the grid, as keyword arguments of ``words``, with the coset count the form reads"""
    for log_n, batch, cosets, fused, in_place in itertools.product(LOG_NS, BATCHES, COSETS, FORMS, (True, False)):
        tabled = fused & (IN_TABLES | OUT_TABLES)
        if bool(cosets) != bool(tabled):                        # the other forms have no coset count; none: tests of their own below
            continue
        if fused & (OUT_TABLE | OUT_TABLES) and not in_place:   # the inverse coset forms never had an input of their own
            continue
        for log_z in range(min(log_n, 12) + 1) if fused in (0, COSET3) else (0,):
            yield dict(log_n=log_n, batch=batch, fwd=cosets if fused & IN_TABLES else 0, inv=cosets if fused & OUT_TABLES else 0, log_z=log_z,
                       fused=fused, in_place=in_place), cosets


def checksum_term(p):
    t = p["passes"] + 3 * p["scratch_bytes"] + 5 * p["table_bytes"] + 29 * p["tail"] + 31 * p["arrays"]
    for i, q in enumerate(p["pass"]):
        t += 7 * (q["gx"] * (i + 1) + q["gy"] + q["gz"] + q["log_c"] + 11 * q["variant"] + 13 * q["src"] + 17 * q["dst"] + 19 * q["direct_tw"]
                  + 23 * (q["tw_lo"] + 1))
    return t


@pytest.fixture(scope="module")
def swept(hc):
    """(admitted calls with their plans' checksum terms, refused count) -- walked once, asserted on the way"""
    buf = Buffers()
    rows = refused = total = 0
    three_pass_coset_forms = extending = 0
    for kw, cosets in sweep():
        call = words(**kw)
        if hc.hc_ntt_check_call(call.ctypes.data_as(ctypes.c_void_p)) is not None:
            refused += 1
            continue
        p = plan(hc, buf, call)
        log_n, batch, log_z, fused, in_place = kw["log_n"], kw["batch"], kw["log_z"], kw["fused"], kw["in_place"]
        n = 1 << log_n
        # ---- the plan is what the old code computed ----
        before, scratch, tail, arrays = entries_before(log_n, batch, cosets, log_z, fused, in_place)
        tabs = tables_before(log_n)
        assert p["passes"] == len(before) and p["digits"][:p["passes"]] == plan_digits_before(log_n), kw
        assert (p["scratch_bytes"], p["arrays"], p["lds_bytes"]) == (scratch, arrays, 36 << LOG_TILE), kw
        assert (p["tail"], tuple(p["tail_grid"])) == ((0, (0, 0)) if tail is None else tail), kw
        assert sorted(p["tables"]) == sorted((dict(lo=0, hi=1, mid=2).get(k, 3),) + v for k, v in tabs.items()), kw
        for q, (h, variant, grid, src, dst, lo) in zip(p["pass"], before):
            assert {k: q[k] for k in HEAD} == h and (q["variant"], (q["gx"], q["gy"], q["gz"]), q["src"], q["dst"]) == (variant, grid, src, dst), (kw, q)
            spec = lambda i: None if i < 0 else p["tables"][i][1:]
            assert spec(q["stage"]) == tabs[("stage", q["s"])] and spec(q["tw_lo"]) == tabs.get(lo) and spec(q["tw_hi"]) == tabs.get("hi"), (kw, q)
        # ---- the invariants ----
        assert sum(p["digits"]) == log_n and all(d <= LOG_TILE for d in p["digits"]) and 1 <= p["passes"] <= 3, kw
        assert p["table_bytes"] == 36 * sum(c for _, c, _ in p["tables"]), kw
        assert p["scratch_bytes"] == (n * 32 * p["arrays"] if p["passes"] > 1 else 0), kw
        for i, q in enumerate(p["pass"]):
            first, last = i == 0, i == p["passes"] - 1
            assert q["s"] + q["log_c"] <= LOG_TILE and q["gx"] << (q["s"] + q["log_c"]) == n, (kw, q)
            assert 1 <= q["gx"] < 1 << 31 and 1 <= q["gy"] <= 65535 and 1 <= q["gz"] <= 65535 and q["gy"] * q["gz"] <= p["arrays"], (kw, q)
            assert q["src"] == ((ARRAY if in_place else INPUT) if first else SCRATCH) and q["dst"] == (ARRAY if last else SCRATCH), (kw, q)
            assert q["last"] == int(last) and q["log_stride"] == log_n - sum(p["digits"][:i + 1]), (kw, q)
            # the stage table: ntt_round forms (base_lo + (m << q0)) << (s - 1 - q) with base_lo + (m << q0) < 2^q, q <= s - 1
            _, count, shift = p["tables"][q["stage"]]
            assert shift == log_n - q["s"] and count >= max(1, (1 << q["s"]) >> 1), (kw, q)
            if last:
                continue
            # the epilogue of a non-last pass: column i0 + c < 2^log_stride, digit value k < 2^s
            product = ((1 << q["log_stride"]) - 1) * ((1 << q["s"]) - 1)
            shift_m = log_n - (q["s"] + q["log_stride"])
            _, lo_count, lo_shift = p["tables"][q["tw_lo"]]
            if q["direct_tw"]:                                  # load_tw(tw_lo, (i0 + c) * k): omega_m^e = omega_n^(e << shift_m)
                assert product < lo_count and lo_shift == shift_m, (kw, q)
            else:                                               # ex = ((i0 + c) * k) << shift_m; tw_hi[ex >> log_lb] * tw_lo[ex & lbmask]
                _, hi_count, hi_shift = p["tables"][q["tw_hi"]]
                ex = product << shift_m
                assert ex < n and lo_shift == 0 and lo_count == 1 << q["log_lb"] and hi_shift == q["log_lb"] and ex >> q["log_lb"] < hi_count, (kw, q)
        if log_z:
            assert p["passes"] >= 2 and log_z <= p["digits"][0] and hc.hc_ntt_extending_applies(log_n, log_z) == 1, kw
            extending += 1
        three_pass_coset_forms += p["passes"] == 3 and bool(fused & (IN_TABLE | IN_TABLES | OUT_TABLE | OUT_TABLES))
        rows += 1
        total += checksum_term(p)
    assert three_pass_coset_forms > 100 and extending > 100
    return rows, refused, total % (1 << 64)


def test_the_plan_is_the_old_host_side_and_keeps_its_invariants(swept):
    rows, refused, _ = swept

    def admitted(kw, cosets):
        """what the check leaves of the grid: the grid's limits, one array per inverse coset, the extending form where the old
        predicate had it (and out of place), the multi-coset form out of place"""
        digits = plan_digits_before(kw["log_n"])
        if kw["batch"] * max(cosets, 1) > 65535 or (kw["fused"] & OUT_TABLES and kw["batch"] > 1) or (kw["fused"] & IN_TABLES and kw["in_place"]):
            return False
        return kw["log_z"] == 0 or (not kw["in_place"] and len(digits) >= 2 and kw["log_z"] <= digits[0])

    grid = list(sweep())
    assert rows == sum(admitted(kw, cosets) for kw, cosets in grid) > 3000 and rows + refused == len(grid)


def test_the_extending_predicate_is_the_plans(hc):
    """what coeff_to_extended_locked asked ntt_plan_first_digit: log_z > 0, at least two passes, log_z <= the first digit"""
    for log_n, log_z in itertools.product(range(29), range(30)):
        digits = plan_digits_before(log_n)
        assert hc.hc_ntt_extending_applies(log_n, log_z) == int(log_z > 0 and len(digits) >= 2 and log_z <= digits[0]), (log_n, log_z)
    assert hc.hc_ntt_extending_applies(29, 1) == 0 and hc.hc_ntt_extending_applies(40, 3) == 0


def test_nothing_to_do_is_an_empty_plan(hc):
    buf = Buffers()
    for kw in (dict(batch=0), dict(batch=3, fused=IN_TABLES, fwd=0, in_place=False), dict(batch=1, fused=SCALE | OUT_TABLES, inv=0),
               dict(batch=0, at_out=OUT + 8)):
        assert check(hc, **kw) is None
        p = plan(hc, buf, words(**kw))
        assert p["passes"] == 0 and p["arrays"] == 0 and p["scratch_bytes"] == 0 and p["tail"] == 0, kw


def refused(why, text):
    assert why is not None and text in why, why
    return True


def test_what_the_suites_send(hc):
    """tests/test_capi.py: test_device_pointer_entry_points_without_a_device; tests/test_ntt_gpu.py: the extending form's refusals and the
    device entries' refusals"""
    assert check(hc) is None
    # hm_coeff_to_cosets: 17 cosets; an output 128 bytes behind one 256-byte input
    assert refused(check(hc, log_n=3, fused=IN_TABLES, fwd=17, in_place=False, at_in=0x1000, at_out=0x100000), "more than 16 cosets")
    assert refused(check(hc, log_n=3, fused=IN_TABLES, fwd=2, in_place=False, at_in=0x1000, at_out=0x1080), "the output overlaps the coefficients")
    assert refused(check(hc, log_n=3, fused=IN_TABLES, fwd=2, in_place=False, at_in=0x1000, at_out=0x1000), "the output overlaps the coefficients")
    assert check(hc, log_n=3, fused=IN_TABLES, fwd=2, in_place=False, at_in=0x1000, at_out=0x1100) is None
    # hm_coeff_to_coset: log_n = 29; an output 32 bytes into the input; the same array is the in-place form
    assert refused(check(hc, log_n=29, fused=IN_TABLE, in_place=False, at_in=0x1000, at_out=0x100000), "log_n > 28")
    assert refused(check(hc, log_n=3, fused=IN_TABLE, in_place=False, at_in=0x1000, at_out=0x1020), "partially overlaps")
    assert check(hc, log_n=3, fused=IN_TABLE, in_place=True, at_out=0x1000) is None
    # hm_coeff_to_extended: log_n = 12 beyond log_ext = 11 (the difference wraps)
    assert refused(check(hc, log_n=11, log_z=(11 - 12) % (1 << 32), in_place=False), "need log_n <= log_ext <= 28")
    # the device entries: a pointer 8 bytes off (either one), batch 65536, batch * cosets beyond the grid, 17 inverse cosets
    assert refused(check(hc, at_out=OUT + 8), "not 16-byte aligned")
    assert refused(check(hc, log_n=14, log_z=2, in_place=False, at_in=IN + 8), "not 16-byte aligned")
    assert check(hc, at_in=IN + 8) is None                     # not read when in place
    assert refused(check(hc, batch=65536), "batch > 65535")
    assert refused(check(hc, batch=4096, fused=IN_TABLES, fwd=16, in_place=False), "batch * cosets > 65535")
    assert check(hc, batch=4095, fused=IN_TABLES, fwd=16, in_place=False) is None
    assert refused(check(hc, fused=SCALE | OUT_TABLES, inv=17), "more than 16 cosets")
    # the extending form where the plan has none: one pass, or more zero bits than the first digit
    assert refused(check(hc, log_n=11, log_z=1, in_place=False), "multi-pass plan")
    assert refused(check(hc, log_n=14, log_z=8, in_place=False), "multi-pass plan") and check(hc, log_n=14, log_z=7, in_place=False) is None
    # shapes no entry forms
    assert refused(check(hc, fused=128), "unknown fused constant") and refused(check(hc, fused=IN_TABLE | IN_TABLES, fwd=1), "not both")
    assert refused(check(hc, fused=IN_TABLE | OUT_TABLE), "input tables and output tables")
    assert refused(check(hc, batch=2, fused=OUT_TABLES, inv=2), "one array per coset")
    assert refused(check(hc, log_n=14, log_z=2, in_place=True), "out of place")
    assert refused(check(hc, fused=IN_TABLES, fwd=2, in_place=True), "the output overlaps the coefficients")


def test_two_broken_rules_are_reported_in_one_order(hc):
    """log_n, the input's length, the cosets, the batch, batch * cosets, the form, the alignment, the overlap"""
    call = dict(log_n=29, log_z=30, fused=IN_TABLES, fwd=17, batch=65536, in_place=False, at_in=OUT + 8, at_out=OUT + 8)
    order = [("log_n", 14, "log_n > 28"), ("log_z", 0, "need log_n <= log_ext"), ("fwd", 16, "more than 16 cosets"), ("batch", 65535, "batch > 65535"),
             ("batch", 2, "batch * cosets > 65535"), ("at_in", OUT + 16, "not 16-byte aligned"), ("at_out", OUT + 16, "not 16-byte aligned"),
             ("at_in", OUT + (1 << 30), "the output overlaps the coefficients")]
    for field, good, text in order:
        assert refused(check(hc, **call), text), (field, call)
        call[field] = good
    assert check(hc, **call) is None


def test_the_sweep_under_the_sanitizers(swept, tmp_path):
    """tests/ntt_plan_host.cpp walks the same grid and asserts the invariants itself; its row count, refusal count and checksum are those
    of this file's sweep through libhm_hostcheck.so"""
    exe = str(tmp_path / "ntt_plan_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-I", _lib.CSRC, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ntt_plan_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.stdout, r.stderr[-2000:])
    rows, refused_calls, total = swept
    assert r.stdout.split() == ["rows", str(rows), "refused", str(refused_calls), "checksum", str(total)]
