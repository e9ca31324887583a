"""The range-check circuit (the reference's OverflowChipV2) on the CPU: the shape of circuits.overflow_check_v2, its parameter limits,
synthesis.RangeCheckLayout against the tests' own MockProver on the reference's two cases
(/root/reference/src/circuits/overflow_check_v2.rs:66-90) and a limb out of range, assign_ints where limbs straddle 64-bit words
against the plain shift-and-mask, the C layout numbers, and the kernel's lane function compiled for the host with the limb-bound checks
on (libhm_hostcheck.so) against assign_ints."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from halo2_experiments_amd import _lib, circuits, poseidon as ps, synthesis as sy
from halo2_experiments_amd.evaluation import Advice, Fixed

import mock_prover
from range_check_cases import values as _values

RC = sy.RangeCheckLayout


def test_shape_of_the_constraint_system():
    cs = circuits.overflow_check_v2(4, 4)
    assert (cs.num_advice, cs.num_fixed, cs.num_instance) == (5, 2, 1)
    assert [name for name, _ in cs.gates] == ["equality check between decomposed value and value"]
    assert len(cs.polynomials()) == 1 and len(cs.lookups) == 4
    assert cs.lookups == [([Advice(c)], [Fixed(0)]) for c in (1, 2, 3, 4)]
    assert cs.equality == [("advice", c) for c in (1, 2, 3, 4)]
    assert cs.degree() == 4
    assert cs.unblinded_advice == () and circuits.overflow_check_v2(4, 4, unblinded_value=True).unblinded_advice == (0,)
    assert circuits.merkle_sum_tree().unblinded_advice == ()
    ref = circuits.CONSTRAINT_SYSTEMS["overflow_check_v2_k5"]()
    assert (ref.num_advice, ref.num_fixed, ref.num_instance, len(ref.lookups)) == (5, 2, 1, 4)
    adv_q, fix_q, inst_q = cs.queries()
    assert sorted(adv_q) == [(c, 0) for c in range(5)] and sorted(fix_q) == [(0, 0), (1, 0)] and inst_q == []
    RC(5, 4, 4, 3).check_constraint_system(cs)
    with pytest.raises(ValueError):
        RC(5, 4, 4, 3).check_constraint_system(circuits.overflow_check_v2(4, 3))
    with pytest.raises(ValueError):
        RC(5, 4, 4, 3).check_constraint_system(circuits.poseidon())


@pytest.mark.parametrize("max_bits, acc_cols", [(0, 4), (17, 1), (4, 0), (16, 16), (11, 24), (1, 254)])
def test_parameter_limits_raise(max_bits, acc_cols):
    with pytest.raises(ValueError):
        circuits.overflow_check_v2(max_bits, acc_cols)
    with pytest.raises(ValueError):
        RC(20, max_bits, acc_cols, 1)


def test_parameter_limits_hold_at_the_edge():
    assert circuits.overflow_check_v2(16, 15).num_advice == 16 and circuits.overflow_check_v2(11, 23).num_advice == 24
    assert circuits.overflow_check_v2(1, 253).num_advice == 254 and circuits.overflow_check_v2(1, 1).num_advice == 2
    assert circuits.overflow_check_v2(16, 15).degree() == 4 and RC(17, 16, 15, 1).N_ADVICE == 16


def test_layout_rows():
    lay = RC(5, 4, 4, 3)
    assert (lay.n, lay.N_ADVICE, lay.table_rows, lay.used_rows, lay.rows_needed(4, 3), lay.min_k(4, 3)) == (32, 5, 16, 16, 16, 5)
    fixed = lay.fixed_columns()
    assert fixed[RC.RANGE] == list(range(16)) + [0] * 16 and fixed[RC.SELECTOR] == [1, 1, 1] + [0] * 29
    assert lay.selector_rows() == {RC.SELECTOR: [0, 1, 2]} and lay.copies() == [] and lay.instance() == [[]]
    assert RC(5, 4, 4, 26).used_rows == 26 and RC.min_k(4, 26) == 5 and RC.min_k(4, 27) == 6 and RC.min_k(16, 1) == 17
    with pytest.raises(ValueError, match="min_k = 6"):
        RC(5, 4, 4, 27)
    with pytest.raises(ValueError):
        RC(5, 5, 4, 3)                      # the table alone needs 32 rows
    with pytest.raises(ValueError):
        RC(5, 4, 4, 0)
    assert sy.permutation_cells(circuits.overflow_check_v2(4, 4), lay) == [[(j, i) for i in range(32)] for j in range(4)]


def _verify(lay, cs, adv):
    return mock_prover.verify(cs, lay.fixed_columns(), adv, [[0] * lay.n], lay.copies(), lay.n, lay.n - sy.BLINDING_ROWS)


def test_the_references_cases():
    """test_none_overflow_case: a = 2^16 - 2, b = 1, a + b; test_overflow_case: b = 3, so a + b = 2^16 + 1 does not fit 4 x 4 bits"""
    lay, cs = RC(5, 4, 4, 3), circuits.overflow_check_v2(4, 4)
    good = lay.assign_ints([65534, 1, 65535])
    assert [good[c][0] for c in range(5)] == [65534, 15, 15, 15, 14] and [good[c][2] for c in range(5)] == [65535, 15, 15, 15, 15]
    assert _verify(lay, cs, good) == []
    bad = lay.assign_ints([65534, 3, 65537])
    assert [bad[c][2] for c in range(5)] == [65537, 0, 0, 0, 1]
    assert _verify(lay, cs, bad) == [("gate", "equality check between decomposed value and value", 0, 2)]


def test_a_limb_out_of_range_fails_its_lookup():
    lay, cs = RC(5, 4, 4, 3), circuits.overflow_check_v2(4, 4)
    adv = lay.assign_ints([65534, 1, 65535])
    adv[2][1] = 16                                           # limb of weight 2^8 on row 1
    adv[0][1] = 16 * 256 + 1                                 # ... with the value adjusted: the gate holds
    assert _verify(lay, cs, adv) == [("lookup", 1, 1)]


@pytest.mark.parametrize("max_bits, acc_cols", [(12, 6), (8, 31), (16, 4), (1, 253), (16, 15)])
def test_assign_ints_is_shift_and_mask(max_bits, acc_cols):
    rows = 40
    k = RC.min_k(max_bits, rows)
    lay = RC(k, max_bits, acc_cols, rows)
    values = _values(max_bits, acc_cols, rows, seed=max_bits * 1000 + acc_cols)
    adv = lay.assign_ints(values)
    mask = (1 << max_bits) - 1
    for row, v in enumerate(values):
        assert adv[0][row] == v
        for i in range(acc_cols):
            assert adv[1 + i][row] == (v >> (max_bits * (acc_cols - 1 - i))) & mask
        total = sum(adv[1 + i][row] << (max_bits * (acc_cols - 1 - i)) for i in range(acc_cols))
        assert (total == v) == (v < 1 << (max_bits * acc_cols))
    assert all(adv[c][row] == 0 for c in range(1 + acc_cols) for row in range(rows, lay.n))


@pytest.mark.parametrize("k, max_bits, acc_cols, rows", [(5, 4, 4, 3), (5, 4, 4, 26), (13, 12, 6, 100), (9, 8, 31, 100), (17, 16, 4, (1 << 17) - 6)])
def test_c_layout_agrees(k, max_bits, acc_cols, rows):
    assert sy.range_c_layout(k, max_bits, acc_cols, rows) == {"n_advice": 1 + acc_cols, "table_rows": 1 << max_bits}


def test_c_layout_refuses_what_the_layout_refuses():
    lib = _lib.load()
    a, b = ctypes.c_uint32(7), ctypes.c_uint32(7)
    for args in ((0, 4, 5, 3), (17, 1, 20, 3), (4, 0, 5, 3), (16, 16, 20, 3), (4, 4, 5, 27), (5, 4, 5, 3), (4, 4, 25, 3), (4, 4, 5, 0)):
        assert lib.hm_range_witness_layout(*args, ctypes.byref(a), ctypes.byref(b)) == -1, args
        assert (a.value, b.value) == (7, 7)
    assert lib.hm_range_witness_layout(4, 4, 5, 3, None, ctypes.byref(b)) == -1
    assert lib.hm_range_witness_layout(4, 4, 5, 26, ctypes.byref(a), ctypes.byref(b)) == 0 and (a.value, b.value) == (5, 16)
    # the witness forms refuse bad arguments before they look for a device
    z = np.zeros(4, dtype=np.uint64)
    zp, fake = z.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.c_void_p(0x1000)
    assert lib.hm_range_witness_bn256_fr_dev(4, 4, 5, 1, 3, None, fake, None, None) == -1
    assert lib.hm_range_witness_bn256_fr_dev(4, 4, 5, 0, 3, fake, ctypes.c_void_p(0x100000), None, None) == -1
    assert lib.hm_range_witness_bn256_fr_dev(4, 4, 5, 1, 3, ctypes.c_void_p(0x1008), ctypes.c_void_p(0x100000), None, None) == -1
    assert lib.hm_range_witness_bn256_fr_dev(4, 4, 5, 1, 3, fake, ctypes.c_void_p(0x1020), None, None) == -1          # overlap
    assert lib.hm_range_witness_bn256_fr(4, 4, 5, 1, 27, zp, zp, None) == -1
    if lib.hm_device_count() == 0:
        assert lib.hm_range_witness_bn256_fr_dev(4, 4, 5, 1, 3, fake, ctypes.c_void_p(0x100000), None, None) == -2


# ---- the kernel's lane function on the host (libhm_hostcheck.so, -DHM_BOUNDS) ------------------------------------------------------
@pytest.fixture(scope="module")
def hostcheck():
    if not os.path.exists(_lib.HOSTCHECK_PATH):
        subprocess.run(["make", "-C", _lib.CSRC, "libhm_hostcheck.so"], check=True, capture_output=True)
    lib = ctypes.CDLL(_lib.HOSTCHECK_PATH)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    lib.hc_range_witness.restype = ctypes.c_int
    lib.hc_range_witness.argtypes = [ctypes.c_uint32] * 3 + [ctypes.c_size_t, ctypes.c_uint32, u32p, u32p, u32p]
    return lib


@pytest.mark.parametrize("k, max_bits, acc_cols, rows", [(5, 4, 4, 26), (7, 12, 6, 100), (9, 8, 31, 100), (6, 16, 15, 40), (9, 1, 253, 40),
                                                         (6, 16, 4, 50)])
def test_lane_function_on_the_host_equals_assign_ints(hostcheck, k, max_bits, acc_cols, rows):
    """every limb the kernel writes, through range_plain / range_limb_ext with their bound checks on; m = 2 circuits.  The host
    entry takes any k that holds the rows (the table is the layout's business), so the columns stay short."""
    u32p, m, n = ctypes.POINTER(ctypes.c_uint32), 2, 1 << k
    values = [_values(max_bits, acc_cols, rows, seed=c) for c in range(m)]
    words = np.ascontiguousarray(ps.ints_to_words([v for vs in values for v in vs]).view(np.uint32))
    adv = np.full((m, 1 + acc_cols, n, 8), 0xFFFFFFFF, dtype=np.uint32)
    over = np.full(m, 77, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(u32p)
    assert hostcheck.hc_range_witness(max_bits, acc_cols, k, m, rows, p(words), p(adv), p(over)) == 0
    mask = (1 << max_bits) - 1
    for c in range(m):
        got = [ps.words_to_ints(col.view(np.uint64)) for col in adv[c]]
        exp = [[0] * n for _ in range(1 + acc_cols)]
        for row, v in enumerate(values[c]):
            exp[0][row] = v
            for i in range(acc_cols):
                exp[1 + i][row] = (v >> (max_bits * (acc_cols - 1 - i))) & mask
        assert got == exp
        assert over[c] == sum(v >> (max_bits * acc_cols) != 0 for v in values[c])
    assert over.sum() >= 4                                   # 2^bits and r - 1 in both circuits: the count is exercised


def test_every_16_bit_limb_goes_into_montgomery_form(hostcheck):
    """range_limb_ext on all 2^16 limbs: the values 0 .. 2^16 - 1 as one column at (16, 1)"""
    u32p, n = ctypes.POINTER(ctypes.c_uint32), 1 << 16
    words = np.ascontiguousarray(ps.ints_to_words(list(range(n))).view(np.uint32))
    adv = np.zeros((1, 2, n, 8), dtype=np.uint32)
    over = np.zeros(1, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(u32p)
    assert hostcheck.hc_range_witness(16, 1, 16, 1, n, p(words), p(adv), p(over)) == 0
    assert np.array_equal(adv[0, 1], words.reshape(n, 8)) and np.array_equal(adv[0, 0], words.reshape(n, 8)) and over[0] == 0
