"""The sorted-column circuit ("the ids of this committed column are pairwise distinct") on the CPU: the shape of
circuits.sorted_column and its parameter limits, synthesis.SortedColumnLayout against the tests' own MockProver -- ascending ids pass,
a duplicate, a swapped pair and a gap one too wide fail, a run that wraps past r passes with distinct ids, which is the soundness
argument as a test -- ``over`` against those verdicts, the B + k <= 253 limit, the C layout numbers, the kernel's lane function
compiled for the host with the bound checks on (libhm_hostcheck.so) against assign_ints word for word, the argsort's record order,
and a mutation sweep of every advice cell against an expectation written by hand."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from halo2_experiments_amd import _lib, circuits, poseidon as ps, synthesis as sy
from halo2_experiments_amd.domain import FR_MODULUS as R
from halo2_experiments_amd.evaluation import Advice, Fixed

import mutation_cases as mc
import sorted_column_cases as sc

SL = sy.SortedColumnLayout


def test_shape_of_the_constraint_system():
    cs = circuits.sorted_column(4, 4)
    assert (cs.num_advice, cs.num_fixed, cs.num_instance) == (5, 2, 1)
    assert [name for name, _ in cs.gates] == [sc.GATE] and len(cs.polynomials()) == 1
    assert cs.lookups == [([Advice(c)], [Fixed(0)]) for c in (1, 2, 3, 4)]
    assert cs.equality == [("advice", c) for c in (1, 2, 3, 4)]
    assert cs.degree() == 4 and cs.unblinded_advice == (0,)
    assert cs.parameters == dict(max_bits=4, acc_cols=4, sorted=True)
    adv_q, fix_q, inst_q = cs.queries()
    assert sorted(adv_q) == [(0, 0), (0, 1)] + [(c, 0) for c in range(1, 5)] and sorted(fix_q) == [(0, 0), (1, 0)] and inst_q == []
    assert "not transcribed" in " ".join(circuits.sorted_column.__doc__.split()).lower()       # the circuit is the project's own
    SL(5, 4, 4, 3).check_constraint_system(cs)
    for other in (circuits.sorted_column(4, 3), circuits.overflow_check_v2(4, 4, unblinded_value=True), circuits.poseidon()):
        with pytest.raises(ValueError):
            SL(5, 4, 4, 3).check_constraint_system(other)


@pytest.mark.parametrize("max_bits, acc_cols", [(0, 4), (17, 1), (4, 0), (16, 16), (11, 24), (1, 254)])
def test_parameter_limits_raise(max_bits, acc_cols):
    with pytest.raises(ValueError):
        circuits.sorted_column(max_bits, acc_cols)
    with pytest.raises(ValueError):
        SL(20, max_bits, acc_cols, 1)


def test_the_sum_of_the_gaps_must_stay_below_r():
    """B + k <= 253: (16, 16) at k = 5 is 261, (16, 15) at k = 17 is 257, (16, 14) at k = 17 is 241"""
    with pytest.raises(ValueError, match="253"):
        SL(5, 16, 16, 3)
    with pytest.raises(ValueError, match=r"= 257 exceeds 253.*agree mod r"):
        SL(17, 16, 15, 3)
    assert SL(17, 16, 14, 3).N_ADVICE == 15 and circuits.sorted_column(16, 15).num_advice == 16       # the circuit alone knows no k
    assert SL(13, 12, 20, 3).width + 13 == 253
    with pytest.raises(ValueError, match="254"):
        SL(14, 12, 20, 3)
    lib = _lib.load()
    a, b = ctypes.c_uint32(7), ctypes.c_uint32(7)
    for args in ((16, 15, 17, 3), (12, 20, 14, 3), (0, 4, 5, 3), (4, 4, 5, 27), (4, 4, 5, 0), (5, 4, 5, 3)):
        assert lib.hm_sorted_witness_layout(*args, ctypes.byref(a), ctypes.byref(b)) == -1 and (a.value, b.value) == (7, 7), args
    assert lib.hm_sorted_witness_layout(16, 14, 17, 3, ctypes.byref(a), ctypes.byref(b)) == 0 and (a.value, b.value) == (15, 1 << 16)
    assert sy.sorted_c_layout(5, 4, 4, 26) == {"n_advice": 5, "table_rows": 16}
    assert sy.sorted_c_layout(17, 16, 8, (1 << 17) - 6) == {"n_advice": 9, "table_rows": 1 << 16}
    # the witness forms and the argsort refuse bad arguments before they look for a device
    fake, far = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x100000)
    assert lib.hm_sorted_witness_bn256_fr_dev(16, 15, 17, 1, 3, fake, far, None, None) == -1
    assert lib.hm_sorted_witness_bn256_fr_dev(4, 4, 5, 1, 3, None, far, None, None) == -1
    assert lib.hm_sorted_witness_bn256_fr_dev(4, 4, 5, 1, 3, ctypes.c_void_p(0x1008), far, None, None) == -1
    assert lib.hm_sorted_witness_bn256_fr_dev(4, 4, 5, 1, 3, fake, ctypes.c_void_p(0x1020), None, None) == -1          # overlap
    u64p = ctypes.POINTER(ctypes.c_uint64)
    perm = ctypes.cast(far, u64p)
    assert lib.hm_fr_argsort_bn256_dev(fake, 0, perm, None) == -1 and lib.hm_fr_argsort_bn256_dev(fake, (1 << 26) + 1, perm, None) == -1
    assert lib.hm_fr_argsort_bn256_dev(None, 4, perm, None) == -1 and lib.hm_fr_argsort_bn256_dev(fake, 4, None, None) == -1
    assert lib.hm_fr_argsort_bn256_dev(ctypes.c_void_p(0x1008), 4, perm, None) == -1
    assert lib.hm_fr_argsort_bn256_dev(fake, 4, ctypes.cast(ctypes.c_void_p(0x100004), u64p), None) == -1
    assert lib.hm_fr_argsort_bn256_dev(fake, 4, ctypes.cast(ctypes.c_void_p(0x1040), u64p), None) == -1                  # overlap
    if lib.hm_device_count() == 0:
        assert lib.hm_fr_argsort_bn256_dev(fake, 4, perm, None) == -2


def test_layout_rows():
    lay = SL(5, 4, 4, 5)
    assert (lay.n, lay.N_ADVICE, lay.table_rows, lay.used_rows, lay.rows_needed(4, 5), lay.min_k(4, 5)) == (32, 5, 16, 16, 16, 5)
    fixed = lay.fixed_columns()
    assert fixed[SL.RANGE] == list(range(16)) + [0] * 16 and fixed[SL.SELECTOR] == [1, 1, 1, 1] + [0] * 28
    assert lay.selector_rows() == {SL.SELECTOR: [0, 1, 2, 3]} and lay.copies() == [] and lay.instance() == [[]]
    one = SL(5, 4, 4, 1)
    assert one.selector_rows() == {SL.SELECTOR: []} and one.fixed_columns()[SL.SELECTOR] == [0] * 32       # one id: nothing to compare
    assert SL(5, 4, 4, 26).used_rows == 26 and SL.min_k(4, 27) == 6 and SL.rows_needed(16, 1) == 1 << 16
    with pytest.raises(ValueError, match="min_k = 6"):
        SL(5, 4, 4, 27)
    with pytest.raises(ValueError):
        SL(5, 4, 4, 0)
    with pytest.raises(ValueError):
        lay.assign_ints([1, 2, 3])
    assert sy.permutation_cells(circuits.sorted_column(4, 4), lay) == [[(j, i) for i in range(32)] for j in range(4)]


@pytest.mark.parametrize("rows", [1, 2, 26])
def test_verdicts_of_the_yardstick(rows):
    lay, cs = SL(5, 4, 4, rows), circuits.sorted_column(4, 4)
    cases = sc.columns_at_4_4(rows)
    assert [name for name, *_ in cases] == {1: ["ascending"], 2: ["ascending", "duplicate", "swapped", "gap 2^16 + 1", "gap 2^16"],
                                            26: ["ascending", "duplicate", "swapped", "gap 2^16 + 1", "gap 2^16", "wraps mod r"]}[rows]
    for name, ids, satisfied, over in cases:
        adv = lay.assign_ints(ids)
        fails = sc.verify(lay, cs, adv)
        assert (fails == []) == satisfied, (name, fails)
        assert all(f[0] == "gate" and f[1] == sc.GATE for f in fails), name          # the limbs are cut to range: only the gate can fail
        assert lay.over(ids) == over == len(fails), name
        if satisfied:
            assert len(set(ids)) == rows, name                   # what the circuit is for
        assert adv[0][:rows] == ids and all(adv[c][row] == 0 for c in range(5) for row in range(rows, 32)), name
        assert all(adv[c][rows - 1] == 0 for c in range(1, 5)), name


def test_the_edges_by_hand():
    lay, cs = SL(5, 4, 4, 2), circuits.sorted_column(4, 4)
    adv = lay.assign_ints([7, 7 + (1 << 16)])                    # d = 2^16 - 1: every limb 15
    assert [adv[c][0] for c in range(5)] == [7, 15, 15, 15, 15] and sc.verify(lay, cs, adv) == []
    adv = lay.assign_ints([7, 7 + (1 << 16) + 1])                # d = 2^16: the low 16 bits are zero
    assert [adv[c][0] for c in range(5)] == [7, 0, 0, 0, 0] and sc.verify(lay, cs, adv) == [("gate", sc.GATE, 0, 0)]
    adv = lay.assign_ints([7, 7])                                # d = -1 = r - 1
    assert [adv[c][0] for c in range(1, 5)] == [((R - 1) >> s) & 15 for s in (12, 8, 4, 0)] and len(sc.verify(lay, cs, adv)) == 1
    # the wrap: r - 2, r - 1, 0, 1 are consecutive mod r, distinct, and satisfied -- the gaps' sum, not the ids, stays below r
    lay4 = SL(5, 4, 4, 4)
    adv = lay4.assign_ints([R - 2, R - 1, 0, 1])
    assert all(adv[c][row] == 0 for c in range(1, 5) for row in range(4)) and sc.verify(lay4, cs, adv) == [] and lay4.over([R - 2, R - 1, 0, 1]) == 0
    # a limb out of range with the id adjusted: the gate holds, the lookup does not
    adv = lay.assign_ints([7, 9])
    adv[2][0], adv[0][1] = 16, 7 + 1 + 16 * 256 + 1
    assert sc.verify(lay, cs, adv) == [("lookup", 1, 0)]


# ---- the kernel's lane function on the host (libhm_hostcheck.so, -DHM_BOUNDS) ------------------------------------------------------
@pytest.fixture(scope="module")
def hostcheck():
    if not os.path.exists(_lib.HOSTCHECK_PATH):
        subprocess.run(["make", "-C", _lib.CSRC, "libhm_hostcheck.so"], check=True, capture_output=True)
    lib = ctypes.CDLL(_lib.HOSTCHECK_PATH)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    lib.hc_sorted_witness.restype = ctypes.c_int
    lib.hc_sorted_witness.argtypes = [ctypes.c_uint32] * 3 + [ctypes.c_size_t, ctypes.c_uint32, u32p, u32p, u32p]
    lib.hc_sorted_record_less.restype = ctypes.c_int
    lib.hc_sorted_record_less.argtypes = [u32p, u32p]
    return lib


@pytest.mark.parametrize("k, max_bits, acc_cols, rows", [(5, 4, 4, 26), (9, 4, 4, 300), (17, 16, 8, 300)])
def test_lane_function_on_the_host_equals_assign_ints(hostcheck, k, max_bits, acc_cols, rows):
    """every word the kernel writes, through range_plain / range_limb_ext with their bound checks on; m = 2 circuits.  300 rows do
    not fit the 26 usable rows of k = 5, so (4, 4) runs at k = 5 with every usable row and at k = 9 with 300; the live rows are
    compared with assign_ints, the rest must be zero on both sides."""
    u32p, m = ctypes.POINTER(ctypes.c_uint32), 2
    log_n = k
    n = 1 << log_n
    ids = [sc.host_ids(max_bits, acc_cols, rows, seed=c) for c in range(m)]
    assert 0 in ids[0] and R - 1 in ids[0] and ids[0][2] == ids[0][3] and ids[0][4] > ids[0][5]
    words = np.ascontiguousarray(ps.ints_to_words([v for vs in ids for v in vs]).view(np.uint32))
    adv = np.full((m, 1 + acc_cols, n, 8), 0xFFFFFFFF, dtype=np.uint32)
    over = np.full(m, 77, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(u32p)
    assert hostcheck.hc_sorted_witness(max_bits, acc_cols, log_n, m, rows, p(words), p(adv), p(over)) == 0
    lay = SL(k, max_bits, acc_cols, rows)
    for c in range(m):
        exp = lay.assign_ints(ids[c])
        got = [ps.words_to_ints(col[:rows].view(np.uint64)) for col in adv[c]]
        assert got == [col[:rows] for col in exp]
        assert not adv[c, :, rows:].any() and not any(any(col[rows:]) for col in exp)
        assert over[c] == lay.over(ids[c])
    assert over.min() >= 3                                       # r - 1 -> 0 is a gap of 0; the equal, descending and too wide pairs count


def test_the_host_entry_refuses_what_the_layout_refuses(hostcheck):
    u32p = ctypes.POINTER(ctypes.c_uint32)
    z = np.zeros(8, dtype=np.uint32)
    p = z.ctypes.data_as(u32p)
    for args in ((0, 4, 5, 1, 3), (17, 1, 5, 1, 3), (4, 0, 5, 1, 3), (16, 15, 17, 1, 3), (4, 4, 25, 1, 3), (4, 4, 5, 1, 0), (4, 4, 5, 1, 33)):
        assert hostcheck.hc_sorted_witness(*args, p, p, p) == -1, args


def test_record_order(hostcheck):
    """the argsort's comparison: the top key word decides first, the row last"""
    u32p = ctypes.POINTER(ctypes.c_uint32)
    rec = lambda key, row: np.array([(key >> (32 * i)) & 0xFFFFFFFF for i in range(8)] + [row], dtype=np.uint32)
    less = lambda a, b: hostcheck.hc_sorted_record_less(a.ctypes.data_as(u32p), b.ctypes.data_as(u32p))
    keys = [0, 1, 1 << 32, (1 << 32) + 1, 1 << 224, (1 << 224) + 1, R - 1, (1 << 256) - 1]
    recs = [rec(key, row) for key in keys for row in (0, 5, 0xFFFFFFFF)]
    for i, a in enumerate(recs):
        for j, b in enumerate(recs):
            assert less(a, b) == int(i < j), (i, j)


# ---- the mutation sweep -------------------------------------------------------------------------------------------------------------
def test_mutation_sweep_every_advice_cell():
    """(4, 4), k = 5, rows = 5: every advice cell plus 1 and plus a random element, judged by the tests' own checker through
    mutation_cases.host_verdicts, against the expectation written by hand in sorted_column_cases.py"""
    c = sc.sweep_case()
    cells = [(col, row) for row in range(c.n) for col in range(c.cs.num_advice)]
    assert len(cells) == 160 and len(sc.EXPECTED_GATE_ROWS) == 21
    sets = {}
    for name, delta in sc.DELTAS.items():
        verdicts = mc.host_verdicts(c, cells, delta)
        for cell, (gates, copies, lookups, gate_rows) in zip(cells, verdicts):
            assert copies == 0 and gates == gate_rows == sc.EXPECTED_GATE_ROWS.get(cell, 0), (name, cell)
        sets[name] = mc.caught_by(cells, verdicts)
        assert not any(row >= c.usable for _, row in sets[name]["failing"])
    assert sets["one"]["gate"] == sets["random"]["gate"] == set(sc.EXPECTED_GATE_ROWS)
    assert sets["one"]["lookup"] == sc.EXPECTED_LOOKUP_ONE and sets["random"]["lookup"] == sc.EXPECTED_LOOKUP_RANDOM
    assert sets["one"]["lookup"] == {cell for cell in sc.EXPECTED_LOOKUP_RANDOM if c.advice[cell[0]][cell[1]] == 15}
    # every cell that holds something is constrained; the free cells are the zero rows no selector reaches
    nonzero = {(col, row) for col in range(5) for row in range(c.n) if c.advice[col][row]}
    assert nonzero <= set(sc.EXPECTED_GATE_ROWS) and (0, 4) in nonzero
    # the negative control: with the selector on the last live row as well, the gate would read the zero padding and fail there
    fixed = [list(col) for col in c.fixed]
    fixed[SL.SELECTOR][4] = 1
    import mock_prover as yardstick
    assert yardstick.verify(c.cs, fixed, c.advice, c.instance, c.copies, c.n, c.usable) == [("gate", sc.GATE, 0, 4)]
