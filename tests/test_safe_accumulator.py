"""The SafeAccumulator circuit (the reference's experiment 17) on the CPU: the reference's four MockProver cases as data
(tests/golden/safe_accumulator_cases.json, from /root/reference/src/circuits/safe_accumulator.rs:98-190) on the tests' own MockProver,
the shape of circuits.safe_accumulator, synthesis.SafeAccumulatorLayout.assign_ints against a plain big-integer accumulation over the
carry patterns of safe_accumulator_cases.py, the kernel's row function compiled for the host with the limb-bound checks on
(libhm_hostcheck.so) against assign_ints on the same patterns, the C layout numbers, and the layout's copies through the permutation
assembly's host build.  Every comparison is word for word."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from halo2_experiments_amd import _lib, circuits, keygen, poseidon as ps, synthesis as sy
from halo2_experiments_amd.domain import FR_MODULUS as R, EvaluationDomain
from halo2_experiments_amd.evaluation import Advice

import mock_prover
import safe_accumulator_cases as sc

SA = sy.SafeAccumulatorLayout
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "safe_accumulator_cases.json")


def verify(lay, cs, adv, instance, fixed=None):
    inst = [list(col) + [0] * (lay.n - len(col)) for col in instance]
    return mock_prover.verify(cs, lay.fixed_columns() if fixed is None else fixed, adv, inst, lay.copies(), lay.n, lay.n - sy.BLINDING_ROWS)


# ---- the reference's four cases -------------------------------------------------------------------------------------------------------
def test_the_references_four_cases():
    with open(GOLDEN) as f:
        golden = json.load(f)
    k, b, A = golden["k"], golden["max_bits"], golden["acc_cols"]
    assert (k, b, A) == (8, 4, 4) and [c["name"] for c in golden["cases"]] == [
        "test_none_overflow_case", "test_none_overflow_case_with_multiple_values", "test_overflow_case", "test_adding_over_range_value"]
    cs = circuits.safe_accumulator(b, A)
    fails = {}
    for case in golden["cases"]:
        lay = SA(k, b, A, len(case["values"]))
        lay.check_constraint_system(cs)
        adv = lay.assign_ints(case["initial"], case["values"])
        inst = lay.instance(case["initial"], case["values"])
        if case["satisfied"]:
            assert inst == [case["instance"]] and verify(lay, cs, adv, inst) == [], case["name"]
            wrong = [list(inst[0])]
            wrong[0][3] ^= 1                                  # a wrong instance limb is caught by its copy
            assert [f[0] for f in verify(lay, cs, adv, wrong)] == ["copy"]
        else:
            fails[case["name"]] = verify(lay, cs, adv, inst)
            assert verify(lay, cs, adv, [[]]) != []           # the reference runs these two with an empty instance
    # 0x0ffd + 4 = 0x1001: the top limb is 1 and its inverse is assigned, so "is_zero" holds and the overflow polynomial does not
    assert fails["test_overflow_case"] == [("gate", sc.GATE, sc.poly_index(A, "overflow"), 1)]
    assert fails["test_adding_over_range_value"] == [("gate", sc.GATE, sc.poly_index(A, "value_range"), 1)]
    # with the inverse withheld the is_zero gate is the one that fails
    lay = SA(k, b, A, 1)
    adv = lay.assign_ints([0, 15, 15, 13], [4])
    assert adv[SA.INV][1] * 1 % R == 1 and adv[lay.ACC[0]][1] == 1
    adv[SA.INV][1] = 0
    assert verify(lay, cs, adv, lay.instance([0, 15, 15, 13], [4])) == [("gate", "is_zero", 0, 1)]


def test_one_value_is_the_references_region_cell_for_cell():
    """chips/safe_accumulator.rs:196-255 at offset 0: the previous limbs on row 0, everything else on row 1"""
    lay = SA(8, 4, 4, 1)
    adv = lay.assign_ints([0, 0, 0xE, 0xD], [5])
    assert [adv[c][0] for c in range(10)] == [0, 0, 0, 0, 0, 0, 0, 0, 0xE, 0xD]
    assert [adv[c][1] for c in range(10)] == [5, 0, 0, 0, 0, 1, 0, 0, 0xF, 2]          # the table of the chip's comment, :101-104
    assert all(adv[c][r] == 0 for c in range(10) for r in range(2, lay.n))


# ---- the system's shape ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b, A", sc.SHAPES + [(1, 64), (3, 2)])
def test_shape_of_the_constraint_system(b, A):
    cs = circuits.safe_accumulator(b, A)
    assert (cs.num_advice, cs.num_fixed, cs.num_instance) == (2 + 2 * A, 3, 1) and cs.lookups == []
    acc, carries = list(range(2 + A, 2 + 2 * A)), list(range(2, 2 + A))
    assert cs.equality == [("advice", c) for c in acc + carries] + [("instance", 0)]
    assert [(name, len(polys)) for name, polys in cs.gates] == [("is_zero", 1), ("bool constraint", A),
                                                                 ("accumulation constraint", 1 + 1 + (A - 1) + 1 + A + A)]
    # 2^b + 1 from the range checks; at b = 1 that is 3 and the is_zero gate, s_over * acc[0] * (1 - acc[0] * inv), has degree 4
    assert cs.degree() == max((1 << b) + 1, 4)
    assert EvaluationDomain(cs.degree(), 6).extended_k == 6 + max(b, 2)
    assert cs.parameters == dict(max_bits=b, acc_cols=A)
    adv_q, fix_q, inst_q = cs.queries()
    assert sorted(adv_q) == sorted([(c, 0) for c in range(2 + 2 * A)] + [(c, -1) for c in acc])
    assert sorted(fix_q) == [(0, 0), (1, 0), (2, 0)] and inst_q == [(0, 0)]
    assert "safe_accumulator" not in "".join(circuits.CONSTRAINT_SYSTEMS) and len(circuits.CONSTRAINT_SYSTEMS) == 5
    SA(10, b, A, 3).check_constraint_system(cs)
    with pytest.raises(ValueError):
        SA(10, b, A, 3).check_constraint_system(circuits.safe_accumulator(b, A + 1 if b * (A + 1) <= 64 else A - 1))
    with pytest.raises(ValueError):
        SA(10, b, A, 3).check_constraint_system(circuits.overflow_check_v2(4, 4))


def test_degree_for_every_limb_width():
    assert [circuits.safe_accumulator(b, 4).degree() for b in (1, 2, 3, 4)] == [4, 5, 9, 17]      # b = 1: the is_zero gate's 4 > 2^1 + 1
    assert [max(circuits.degree(p) for p in circuits.safe_accumulator(b, 4).gates[2][1]) for b in (1, 2, 3, 4)] == [3, 5, 9, 17]
    assert circuits.degree(circuits.range_check(Advice(0), 16)) == 16


@pytest.mark.parametrize("b, A", [(0, 4), (5, 4), (4, 1), (4, 17), (1, 65), (3, 22)])
def test_parameter_limits_raise(b, A):
    with pytest.raises(ValueError):
        circuits.safe_accumulator(b, A)
    with pytest.raises(ValueError):
        SA(10, b, A, 1)


def test_layout_rows():
    lay = SA(5, 2, 3, 3)
    assert (lay.n, lay.N_ADVICE, lay.used_rows, SA.rows_needed(3), SA.min_k(3), SA.min_k(26), SA.min_k(25)) == (32, 8, 4, 4, 4, 6, 5)
    assert lay.selector_rows() == {0: [1, 2, 3], 1: [1, 2, 3], 2: [1, 2, 3]}
    assert lay.fixed_columns() == [[0, 1, 1, 1] + [0] * 28] * 3
    assert lay.copies() == [(("advice", 5 + i, 3), ("instance", 0, i)) for i in range(3)]
    assert [(r.name, r.start, r.height) for r in lay.regions] == [("calculate accumulates", 0, 4)]
    SA(5, 2, 3, 25)
    with pytest.raises(ValueError, match="min_k = 6"):
        SA(5, 2, 3, 26)
    with pytest.raises(ValueError):
        SA(5, 2, 3, 0)
    with pytest.raises(ValueError):
        lay.assign_ints([0, 1, 2], [1, 2])
    with pytest.raises(ValueError):
        lay.assign_ints([0, 1], [1, 2, 3])


# ---- assign_ints against the plain accumulation ---------------------------------------------------------------------------------------
def pattern_cases(b, A):
    """(pattern, rows, at): every pattern, the chain started on the last row, in the middle and on row 1"""
    rows = 12
    out = [(name, rows, None) for name in ("zeros", "max", "random")]
    out += [(name, rows, at) for name in ("ripple", "overflow") for at in (1, 7, rows)]
    if b * A == 64:
        out += [("wrap", rows, at) for at in (1, rows)]
    return out


def check_against_accumulation(lay, adv, initial, values):
    b, A = lay.max_bits, lay.acc_cols
    assert [adv[c][0] for c in range(lay.N_ADVICE)] == [0] * (2 + A) + [int(x) % R for x in initial]
    for r, (s, carries) in enumerate(sc.accumulate(b, A, initial, values), start=1):
        limbs = sc.limbs_of(s, b, A)
        assert [adv[c][r] for c in lay.ACC] == limbs, r
        assert adv[SA.VALUE][r] == int(values[r - 1]) % R
        assert adv[SA.INV][r] * limbs[0] % R == (1 if limbs[0] else 0) and (limbs[0] or adv[SA.INV][r] == 0)
        if carries is not None:
            assert [adv[c][r] for c in lay.CARRIES] == carries, r
    assert all(adv[c][r] == 0 for c in range(lay.N_ADVICE) for r in range(len(values) + 1, lay.n))


@pytest.mark.parametrize("b, A", sc.SHAPES)
def test_assign_ints_is_the_plain_accumulation(b, A):
    cs = circuits.safe_accumulator(b, A)
    seen = set()
    for name, rows, at in pattern_cases(b, A):
        lay = SA(5, b, A, rows)
        initial, values = sc.pattern(name, b, A, rows, at, seed=3)
        adv = lay.assign_ints(initial, values)
        check_against_accumulation(lay, adv, initial, values)
        inst = lay.instance(initial, values)
        assert inst == [sc.limbs_of(sc.accumulate(b, A, initial, values)[-1][0], b, A)] == [lay.finals(initial, values)]
        good = sc.satisfied(b, A, initial, values)
        assert (lay.over(initial, values) == 0) == good
        fails = verify(lay, cs, adv, inst)
        assert (fails == []) == good, (name, at, fails)
        seen.add((name, good))
        at = rows if at is None else at
        if name == "ripple" and A > 2:                       # 0x00ff..f + 1: A - 2 limbs ripple, each with a carry out: c[2 .. A-1] = 1
            assert good and [adv[c][at] for c in lay.CARRIES] == [0, 0] + [1] * (A - 2)
            assert [adv[c][at] for c in lay.ACC] == [0, 1] + [0] * (A - 2)
        if name == "overflow":                               # 0x0fff..f + 1: the top limb becomes 1 and stays
            assert ("gate", sc.GATE, sc.poly_index(A, "overflow"), at) in fails
            assert [adv[c][at] for c in lay.ACC] == [1] + [0] * (A - 1) and [adv[c][at] for c in lay.CARRIES] == [0] + [1] * (A - 1)
            assert lay.over(initial, values) == rows - at + 1
        if name == "wrap":                                   # 2^64 - 1 + 1: the total wraps to 0, the top limb's polynomial cannot hold
            assert s64(lay, initial, values, at - 1) == (1 << 64) - 1 and s64(lay, initial, values, at) == 0
            assert ("gate", sc.GATE, sc.poly_index(A, "limb", 0), at) in fails
            assert ("gate", sc.GATE, sc.poly_index(A, "prev_range", 0), at) not in fails       # 15 is a legal limb; it is not zero
            assert ("gate", sc.GATE, sc.poly_index(A, "overflow"), at - 1) in fails or at == 1
        if name == "max" and not good:
            assert any(f[:3] == ("gate", sc.GATE, sc.poly_index(A, "overflow")) for f in fails)
    assert ("zeros", True) in seen and ("ripple", True) in seen and ("overflow", False) in seen


def s64(lay, initial, values, row):
    return lay.state(initial) if row == 0 else sc.accumulate(lay.max_bits, lay.acc_cols, initial, values[:row])[-1][0]


def test_values_and_limbs_that_are_not_judged():
    """a value at or above 2^b and an initial limb at or above 2^b: the rows are what the definition says, and the named polynomials fail"""
    b, A = 4, 4
    lay, cs = SA(5, b, A, 3), circuits.safe_accumulator(b, A)
    initial, values = [0, 0, 3, 9], [5, (1 << 16) + 0x123, R - 1]
    adv = lay.assign_ints(initial, values)
    check_against_accumulation(lay, adv, initial, values)
    assert adv[0][2] == (1 << 16) + 0x123 and [adv[c][2] for c in lay.ACC] == sc.limbs_of((0x39 + 5 + 0x123) % (1 << 16), b, A)
    fails = verify(lay, cs, adv, lay.instance(initial, values))
    assert ("gate", sc.GATE, sc.poly_index(A, "value_range"), 2) in fails and ("gate", sc.GATE, sc.poly_index(A, "value_range"), 3) in fails
    assert lay.over(initial, values) >= 2
    initial = [0, 16, 3, 9]                                  # S_0 = 0x1039: the limb 16 is kept as given on row 0
    adv = lay.assign_ints(initial, [1, 1, 1])
    assert [adv[c][0] for c in lay.ACC] == [0, 16, 3, 9] and [adv[c][1] for c in lay.ACC] == [1, 0, 3, 10]
    fails = verify(lay, cs, adv, lay.instance(initial, [1, 1, 1]))
    assert ("gate", sc.GATE, sc.poly_index(A, "prev_range", 1), 1) in fails and lay.over(initial, [1, 1, 1]) == 4


# ---- the kernel's row function on the host (libhm_hostcheck.so, -DHM_BOUNDS) ------------------------------------------------------------
@pytest.fixture(scope="module")
def hostcheck():
    subprocess.run(["make", "-C", _lib.CSRC, "libhm_hostcheck.so"], check=True, capture_output=True)
    lib = ctypes.CDLL(_lib.HOSTCHECK_PATH)
    u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    lib.hc_accumulator_witness.restype = ctypes.c_int
    lib.hc_accumulator_witness.argtypes = [ctypes.c_uint32] * 3 + [ctypes.c_size_t, ctypes.c_uint32, u32p, u64p, u32p, u64p, u32p]
    return lib


def host_witness(hostcheck, k, b, A, initials, values):
    m, rows = len(values), len(values[0])
    u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    words = np.ascontiguousarray(ps.ints_to_words([v for vs in values for v in vs]).view(np.uint32))
    init = np.array(initials, dtype=np.uint64)
    adv = np.full((m, 2 + 2 * A, 1 << k, 8), 0xFFFFFFFF, dtype=np.uint32)          # every word must be written
    finals, over = np.full((m, A), 77, dtype=np.uint64), np.full(m, 77, dtype=np.uint32)
    rc = hostcheck.hc_accumulator_witness(b, A, k, m, rows, words.ctypes.data_as(u32p), init.ctypes.data_as(u64p), adv.ctypes.data_as(u32p),
                                          finals.ctypes.data_as(u64p), over.ctypes.data_as(u32p))
    assert rc == 0
    return adv.view(np.uint64), finals, over


@pytest.mark.parametrize("b, A", sc.SHAPES)
def test_row_function_on_the_host_equals_assign_ints(hostcheck, b, A):
    """every cell the kernels write, through range_plain / range_limb_ext / acc_mont_u64 with their bound checks on: the patterns as
    the circuits of one call, so that the circuit offsets are exercised too"""
    cases = pattern_cases(b, A)
    rows = cases[0][1]
    lay = SA(5, b, A, rows)
    pairs = [sc.pattern(name, b, A, rows, at, seed=5) for name, rows, at in cases]
    pairs.append(([0, (1 << 40) + 3] + [1] * (A - 2), [R - 1, 1 << b, (1 << 64) + 1] + [1] * (rows - 3)))      # nothing is judged
    adv, finals, over = host_witness(hostcheck, 5, b, A, [p[0] for p in pairs], [p[1] for p in pairs])
    for c, (initial, values) in enumerate(pairs):
        assert np.array_equal(adv[c], sy.columns_to_words(lay.assign_ints(initial, values))), c
        assert finals[c].tolist() == lay.finals(initial, values) and over[c] == lay.over(initial, values), c
    assert over.min() == 0 and over.max() > 0


def test_every_top_limb_reads_its_inverse(hostcheck):
    """(4, 2): the state walks through every top limb 0 .. 15 and wraps: the inverse column against pow(limb, r - 2, r)"""
    rows = 20
    lay = SA(5, 4, 2, rows)
    initial, values = [0, 9], [15] * rows
    adv, finals, over = host_witness(hostcheck, 5, 4, 2, [initial], [values])
    assert np.array_equal(adv[0], sy.columns_to_words(lay.assign_ints(initial, values)))
    tops = [sc.limbs_of(s, 4, 2)[0] for s, _ in sc.accumulate(4, 2, initial, values)]
    assert set(tops) == set(range(16)) and over[0] == sum(t != 0 for t in tops)


# ---- the C layout and its refusals ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, b, A, rows", [(5, 4, 4, 3), (5, 2, 3, 25), (8, 4, 16, 249), (17, 1, 2, (1 << 17) - 7)])
def test_c_layout_agrees(k, b, A, rows):
    assert sy.accumulator_c_layout(k, b, A, rows) == {"n_advice": 2 + 2 * A, "used_rows": rows + 1}


def test_c_layout_refuses_what_the_layout_refuses():
    lib = _lib.load()
    a, u = ctypes.c_uint32(7), ctypes.c_uint32(7)
    for args in ((0, 4, 5, 3), (5, 4, 8, 3), (4, 1, 5, 3), (4, 17, 8, 3), (1, 65, 8, 3), (4, 4, 5, 26), (4, 4, 25, 3), (4, 4, 5, 0)):
        assert lib.hm_accumulator_witness_layout(*args, ctypes.byref(a), ctypes.byref(u)) == -1, args
        assert (a.value, u.value) == (7, 7)
    assert lib.hm_accumulator_witness_layout(4, 4, 5, 3, None, ctypes.byref(u)) == -1
    assert lib.hm_accumulator_witness_layout(4, 4, 5, 25, ctypes.byref(a), ctypes.byref(u)) == 0 and (a.value, u.value) == (10, 26)
    # the witness forms refuse bad arguments before they look for a device
    z = np.zeros(64, dtype=np.uint64)
    zp, fake = z.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.c_void_p(0x1000)
    u64 = lambda addr: ctypes.cast(ctypes.c_void_p(addr), ctypes.POINTER(ctypes.c_uint64))
    dev = lambda b=4, A=4, k=5, m=1, rows=3, v=fake, i=u64(0x2000), adv=ctypes.c_void_p(0x100000), f=u64(0x3000): \
        lib.hm_accumulator_witness_bn256_fr_dev(b, A, k, m, rows, v, i, adv, f, None, None)
    bad = [dev(v=None), dev(i=None), dev(adv=None), dev(f=None), dev(m=0), dev(m=65536), dev(rows=26), dev(b=4, A=17),
           dev(v=ctypes.c_void_p(0x1008)), dev(i=u64(0x2004)), dev(f=u64(0x3004)), dev(adv=ctypes.c_void_p(0x1020)), dev(f=u64(0x2008)),
           dev(f=u64(0x100040))]
    assert bad == [-1] * len(bad)
    assert lib.hm_accumulator_witness_bn256_fr(4, 4, 5, 1, 26, zp, zp, zp, zp, None) == -1
    assert lib.hm_accumulator_witness_bn256_fr(4, 4, 24, 1, 3, zp, zp, zp, zp, None) == -1     # more than 256 MiB of columns
    if lib.hm_device_count() == 0:
        assert dev() == -2


def test_the_numpy_twin_of_the_large_gpu_cases_equals_assign_ints():
    """safe_accumulator_cases.numpy_columns, which tests/test_safe_accumulator_gpu.py uses at 2^15 and 2^17 rows"""
    for b, A in sc.SHAPES:
        rows = 300
        lay = SA(9, b, A, rows)
        for name in ("random", "max", "ripple", "wrap" if b * A == 64 else "overflow"):
            initial, values = sc.pattern(name, b, A, rows, 200, seed=2)
            if any(x >> b for x in initial):
                continue
            cols, finals, over = sc.numpy_columns(b, A, initial, np.array(values, dtype=np.uint64), 512)
            assert np.array_equal(cols, sy.columns_to_words(lay.assign_ints(initial, values))), (b, A, name)
            assert finals == lay.finals(initial, values) and over == lay.over(initial, values), (b, A, name)


def test_package_exports_the_feature():
    header = open(_lib.HEADER_PATH).read()
    with open(os.path.join(_lib.CSRC, "accumulator.hip")) as f:
        assert f"ACC_THREADS = {sy.ACCUMULATOR_BLOCK_ROWS}," in f.read()           # the block size the GPU tests place their boundaries by
    for name in ("hm_accumulator_witness_layout", "hm_accumulator_witness_bn256_fr_dev", "hm_accumulator_witness_bn256_fr",
                 "hm_accumulator_witness_timed_bn256_fr_dev"):
        assert name in _lib._SIGNATURES and hasattr(_lib.load(), name) and f"int {name}(" in header
    for name in ("accumulator_witness", "accumulator_witness_host", "accumulator_c_layout", "SafeAccumulatorLayout"):
        assert hasattr(sy, name)
    objs = subprocess.run(["make", "-s", "-C", _lib.CSRC, "print-objs"], check=True, capture_output=True, text=True).stdout.split()
    assert "accumulator.o" in objs


# ---- the layout through the permutation assembly --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, b, A, rows", [(5, 2, 3, 3), (6, 4, 4, 40), (5, 4, 16, 25)])
def test_permutation_cells_and_sigma_columns(hostcheck, k, b, A, rows):
    """the A copies close A two-cycles: accumulate column i on row ``rows`` with instance row i; the device assembly's rule, built for
    the host, gives the same cells, and the sigma columns are those cells as delta^j omega^i"""
    cs, lay = circuits.safe_accumulator(b, A), SA(k, b, A, rows)
    n, P = lay.n, len(cs.equality)
    assert P == 2 * A + 1
    cells = sy.permutation_cells(cs, lay)
    exp = [[(j, i) for i in range(n)] for j in range(P)]
    for i in range(A):                                       # equality column i is accumulate[i]; the instance column is the last
        exp[i][rows], exp[P - 1][i] = (P - 1, i), (i, rows)
    assert cells == exp
    pairs = keygen.copy_pairs(cs, lay)
    assert pairs.tolist() == [[i * n + rows, (P - 1) * n + i] for i in range(A)]
    u32p = ctypes.POINTER(ctypes.c_uint32)
    hostcheck.hc_permutation_assemble.argtypes = [u32p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p]
    arr = np.ascontiguousarray(pairs, dtype=np.uint32)
    out, dropped = np.zeros(P << k, dtype=np.uint32), np.full(1, 77, dtype=np.uint32)
    assert hostcheck.hc_permutation_assemble(arr.ctypes.data_as(u32p), len(arr), P, k, out.ctypes.data_as(u32p), dropped.ctypes.data_as(u32p)) == 0
    assert out.tolist() == [j * n + i for col in cells for (j, i) in col] and dropped[0] == 0
    dom = EvaluationDomain(cs.degree(), k)
    delta = keygen.FR_DELTA
    sigma = sy.permutation_columns_ints(cs, lay, dom.omega, delta)
    for i in range(A):
        assert sigma[i][rows] == pow(delta, P - 1, R) * pow(dom.omega, i, R) % R
        assert sigma[P - 1][i] == pow(delta, i, R) * pow(dom.omega, rows, R) % R
    assert sum(sigma[j][i] != pow(delta, j, R) * pow(dom.omega, i, R) % R for j in range(P) for i in range(n)) == 2 * A
