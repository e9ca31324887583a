"""shplonk.py on the CPU: the rotation sets, the identity the kernel computes by against the integer twin stated the long way, the
refusals, and the host statement of csrc/shplonk.inc (plan, coefficients, the row formula's bounds) in host_check.cpp."""
import ctypes
import random
import subprocess

import numpy as np
import pytest

from halo2_experiments_amd import _lib, shplonk as sh
from halo2_experiments_amd.domain import FR_MODULUS as R, fr_words
from halo2_experiments_amd.poseidon import words_to_ints

_u64p = ctypes.POINTER(ctypes.c_uint64)


def test_construct_intermediate_sets():
    # a, c share {1, 5}; b and e have {5}; d has {1, 5, 9}; repeated queries of one commitment at one point keep the first eval
    q = [("a", 5, 10), ("b", 5, 20), ("a", 1, 11), ("c", 1, 31), ("d", 9, 40), ("c", 5, 30), ("d", 1, 41), ("d", 5, 42), ("e", 5, 50),
         ("a", 5, 99)]
    sets, super_points = sh.construct_intermediate_sets(q)
    assert super_points == [1, 5, 9]
    assert sets == [([1, 5], [("a", [11, 10]), ("c", [31, 30])]),
                    ([5], [("b", [20]), ("e", [50])]),
                    ([1, 5, 9], [("d", [41, 42, 40])])]
    # the points are ordered as integers mod r, whatever the order of the queries
    sets, super_points = sh.construct_intermediate_sets([("z", R - 1, 1), ("z", 2, 2), ("z", -3, 3)])
    assert sets == [([2, R - 3, R - 1], [("z", [2, 3, 1])])] and super_points == [2, R - 3, R - 1]


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("t", [1, 2, 3, 4])
def test_kate_identity_equals_the_chain(t, m):
    rng = random.Random(100 * t + m)
    for n in (t + 1, 37, 64):
        polys = [[rng.randrange(R) for _ in range(n)] for _ in range(m)]
        weights = [rng.randrange(R) for _ in range(m)]
        points = [rng.randrange(R) for _ in range(t)]
        scale = rng.randrange(1, R)
        want = sh.set_quotient_ints(polys, weights, points, scale)
        got = sh.set_quotient_kate_ints(polys, weights, points, scale)
        assert len(want) == n and want == got
        assert want[n - t:] == [0] * t                                   # and the identity's top t - 1 rows vanish by themselves
        # it IS the quotient: q * Z_S + R = N at a random point, deg R < t
        x = rng.randrange(R)
        num = sh.eval_ints([sum(w * p[i] for w, p in zip(weights, polys)) % R for i in range(n)], x) * scale % R
        rem = (num - sh.eval_ints(want, x) * sh.vanishing_eval(points, x)) % R
        r_poly = sh.lagrange_interpolate_ints(points, [sh.eval_ints([sum(w * p[i] for w, p in zip(weights, polys)) % R for i in range(n)], p)
                                                       for p in points])
        assert rem == sh.eval_ints(r_poly, x) * scale % R


def test_refusals():
    p = [[1, 2, 3, 4, 5]]
    for bad in ([7, 7], [1, 2, 1], [3, R + 3], [], [1, 2, 3, 4, 5]):
        with pytest.raises(ValueError):
            sh.set_quotient_ints(p, [1], bad)
        with pytest.raises(ValueError):
            sh.set_quotient_coefficients(bad)
    with pytest.raises(ValueError):
        sh.set_quotient_ints([[1, 2, 3]], [1], [1, 2, 3])                # n < t + 1
    with pytest.raises(ValueError):
        sh.set_quotient_ints(p, [1, 2], [1])
    assert sh.kate_ints([5], 3) == []


@pytest.fixture(scope="module")
def hc():
    subprocess.run(["make", "-C", _lib.CSRC, "libhm_hostcheck.so"], check=True, capture_output=True)
    lib = ctypes.CDLL(_lib.HOSTCHECK_PATH)
    lib.hc_shplonk_plan.argtypes = [ctypes.c_uint64, _u64p]
    lib.hc_shplonk_plan.restype = None
    lib.hc_shplonk_coefficients.argtypes = [ctypes.c_uint32, _u64p, _u64p, _u64p]
    lib.hc_shplonk_row_bounds.argtypes = [_u64p, ctypes.POINTER(ctypes.c_double)]
    return lib


def test_host_statement_of_the_kernel(hc):
    # the plan: the Python twin the GPU test reads its shapes from
    for n in (2, 3, 4, 5, 64, 1024, 1025, 1026, 1 << 14, (1 << 18) + 1, 1 << 20):
        plan = (ctypes.c_uint64 * 4)()
        hc.hc_shplonk_plan(n, plan)
        b, g, lanes = sh.set_quotient_plan(n)
        assert (plan[0], plan[1], plan[2]) == (b, g, lanes) and plan[3] == (g * 256 + 1 + 2 * g) * 9
        assert lanes * b >= n > (lanes - 1) * b and g <= 256
    assert sh.set_quotient_plan(4)[2] == 1 and sh.set_quotient_plan(5) == (4, 1, 2)
    assert sh.set_quotient_plan(1024)[1] == 1 and sh.set_quotient_plan(1025)[1] == 2
    # the coefficients in host_fr.h arithmetic against the integers
    rng = random.Random(17)
    for t in (1, 2, 3, 4):
        pts, scale = [rng.randrange(R) for _ in range(t)], rng.randrange(1, R)
        out = np.zeros((t, 4), dtype=np.uint64)
        pw = np.stack([fr_words(p) for p in pts])
        assert hc.hc_shplonk_coefficients(t, pw.ctypes.data_as(_u64p), fr_words(scale).ctypes.data_as(_u64p), out.ctypes.data_as(_u64p)) == 0
        assert words_to_ints(out) == sh.set_quotient_coefficients(pts, scale)
    two = np.stack([fr_words(5), fr_words(5)])
    one = fr_words(1)
    out = np.zeros((4, 4), dtype=np.uint64)
    assert hc.hc_shplonk_coefficients(2, two.ctypes.data_as(_u64p), one.ctypes.data_as(_u64p), out.ctypes.data_as(_u64p)) == -1     # equal points
    assert hc.hc_shplonk_coefficients(0, two.ctypes.data_as(_u64p), one.ctypes.data_as(_u64p), out.ctypes.data_as(_u64p)) == -1
    assert hc.hc_shplonk_coefficients(5, two.ctypes.data_as(_u64p), one.ctypes.data_as(_u64p), out.ctypes.data_as(_u64p)) == -1
    big = np.stack([np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)])
    assert hc.hc_shplonk_coefficients(1, big.ctypes.data_as(_u64p), one.ctypes.data_as(_u64p), out.ctypes.data_as(_u64p)) == -1     # not below r
    # the row formula at its class maxima
    report = (ctypes.c_double * 1)()
    assert hc.hc_shplonk_row_bounds(fr_words(rng.randrange(R)).ctypes.data_as(_u64p), report) == 1 and 0 < report[0] <= 3.0


def test_entry_point_without_a_device():
    """every refusal of the C entry is HM_ERR_BAD_ARG before any device is looked for"""
    lib = _lib.load()
    one = np.stack([fr_words(1)] * 5)
    pts = np.stack([fr_words(i + 2) for i in range(5)])
    p = lambda a: a.ctypes.data_as(_u64p)
    tab = (ctypes.c_void_p * 2)(0x1000, 0x2000)
    f = lib.hm_shplonk_set_quotient_bn256_fr_dev
    out = ctypes.c_void_p(0x9000)
    assert f(None, p(one), 2, 8, p(pts), 2, p(one), out, 0, None) == -1
    assert f(tab, p(one), 2, 8, p(pts), 2, p(one), None, 0, None) == -1
    assert f(tab, p(one), 0, 8, p(pts), 2, p(one), out, 0, None) == -1            # m = 0
    assert f(tab, p(one), 2, 8, p(pts), 0, p(one), out, 0, None) == -1            # t = 0
    assert f(tab, p(one), 2, 8, p(pts), 5, p(one), out, 0, None) == -1            # t above the cap
    assert f(tab, p(one), 2, 2, p(pts), 2, p(one), out, 0, None) == -1            # n < t + 1
    assert f(tab, p(one), 2, 8, p(one), 2, p(one), out, 0, None) == -1            # two equal points
    assert b"equal points" in lib.hm_last_error()
    assert f(tab, p(one), 2, 8, p(pts), 2, p(one), ctypes.c_void_p(0x9008), 0, None) == -1       # misaligned output
    assert f((ctypes.c_void_p * 2)(0x1000, 0x2004), p(one), 2, 8, p(pts), 2, p(one), out, 0, None) == -1
    assert f((ctypes.c_void_p * 2)(0x1000, None), p(one), 2, 8, p(pts), 2, p(one), out, 0, None) == -1
    if lib.hm_device_count() == 0:
        assert f(tab, p(one), 2, 8, p(pts), 2, p(one), out, 0, None) == -2        # valid-looking arguments: no device, no fallback
