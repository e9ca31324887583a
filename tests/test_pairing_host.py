"""CPU suite of the device pairing (csrc/pairing.inc): the tower, the Miller lane and the final exponentiation compiled for the host
under bound tracking (-DHM_BOUNDS; any violated precondition aborts the process) and compared with pairing.py word for word."""
import ctypes
import random
import subprocess

import numpy as np
import pytest

from halo2_experiments_amd import _lib
from halo2_experiments_amd import pairing as pr
from halo2_experiments_amd.bn256 import fq_array, fq_ints
from halo2_experiments_amd.kzg import _B2, _fq2_inv, _fq2_mul, _fq2_sub, g2_mul

P = pr.P
P64 = ctypes.POINTER(ctypes.c_uint64)


def ptr(a):
    return None if a is None else a.ctypes.data_as(P64)


@pytest.fixture(scope="module")
def hc():
    subprocess.run(["make", "-C", _lib.CSRC, "libhm_hostcheck.so"], check=True, capture_output=True)
    lib = ctypes.CDLL(_lib.HOSTCHECK_PATH)
    for name in ("hc_f12_op", "hc_f2_op", "hc_pairing_product"):
        getattr(lib, name).restype = ctypes.c_int
    lib.hc_pairing_product.argtypes = [P64, P64, ctypes.c_size_t, P64]
    return lib


def f12_flat(a):
    return [c for six in a for two in six for c in two]


def f12_nest(v):
    two = [(v[2 * i], v[2 * i + 1]) for i in range(6)]
    return (tuple(two[:3]), tuple(two[3:]))


def f12_words(a):
    return np.ascontiguousarray(fq_array(f12_flat(a)).reshape(-1))


def f12_op(hc, op, a, b=None):
    out = np.zeros(48, dtype=np.uint64)
    wa, wb = f12_words(a), None if b is None else f12_words(b)
    assert hc.hc_f12_op(op, ptr(wa), ptr(wb), ptr(out)) == 0
    return f12_nest(fq_ints(out.reshape(12, 4)))


def f2_op(hc, op, a, b=None):
    out = np.zeros(8, dtype=np.uint64)
    wa = np.ascontiguousarray(fq_array(list(a)).reshape(-1))
    wb = None if b is None else np.ascontiguousarray(fq_array(list(b)).reshape(-1))
    assert hc.hc_f2_op(op, ptr(wa), ptr(wb), ptr(out)) == 0
    return tuple(fq_ints(out.reshape(2, 4)))


def edge_and_random(n_fq, seed, count=3):
    """elements whose Fq coordinates are all 0, all 1, all p - 1, then seeded random ones"""
    rng = random.Random(seed)
    return [[v] * n_fq for v in (0, 1, P - 1)] + [[rng.randrange(P) for _ in range(n_fq)] for _ in range(count)]


F12S = [f12_nest(v) for v in edge_and_random(12, 1)]


def test_fq2_ops_at_the_edges_and_at_random(hc):
    els = [tuple(v) for v in edge_and_random(2, 2)]
    for a in els:
        assert f2_op(hc, 1, a) == _fq2_mul(a, a)
        assert f2_op(hc, 3, a) == pr._f2_mul_xi(a)
        assert f2_op(hc, 6, a) == pr._f2_conj(a)
        if a != (0, 0) and (a[0] * a[0] + a[1] * a[1]) % P:
            assert f2_op(hc, 2, a) == _fq2_inv(a)
        for b in els:
            assert f2_op(hc, 0, a, b) == _fq2_mul(a, b)
            assert f2_op(hc, 4, a, b) == pr._f2_add(a, b)
            assert f2_op(hc, 5, a, b) == _fq2_sub(a, b)
    assert f2_op(hc, 2, (0, 0)) == (0, 0)                     # a zero is never inverted into a fault


def test_fq6_product_is_the_even_powers_of_the_fq12_product(hc):
    sixes = [tuple((v[2 * i], v[2 * i + 1]) for i in range(3)) for v in edge_and_random(6, 3)]
    for a in sixes:
        for b in sixes:
            got = f12_op(hc, 8, (a, pr.F6_ZERO), (b, pr.F6_ZERO))
            assert got == (pr._f6_mul(a, b), pr.F6_ZERO)


def test_fq12_product_square_and_conjugate(hc):
    for a in F12S:
        assert f12_op(hc, 1, a) == pr.f12_mul(a, a)
        assert f12_op(hc, 3, a) == pr.f12_conj(a)
        for b in F12S:
            assert f12_op(hc, 0, a, b) == pr.f12_mul(a, b)


def test_sparse_line_product_against_the_dense_one(hc):
    rng = random.Random(4)
    for a in F12S:
        for vals in ([0] * 6, [1] * 6, [P - 1] * 6, [rng.randrange(P) for _ in range(6)]):
            c0, c1, c3 = (vals[0], vals[1]), (vals[2], vals[3]), (vals[4], vals[5])
            line = ((c0, pr.F2_ZERO, pr.F2_ZERO), (c1, c3, pr.F2_ZERO))
            junk = ((c0, (5, 6), (7, 8)), (c1, c3, (9, 10)))           # what a line never holds is never read
            assert f12_op(hc, 2, a, junk) == pr.f12_mul(a, line)


def test_frobenius_maps(hc):
    for a in F12S:
        f1 = pr.f12_frobenius(a)
        f2 = pr.f12_frobenius(f1)
        assert f12_op(hc, 4, a) == f1 and f12_op(hc, 5, a) == f2 and f12_op(hc, 6, a) == pr.f12_frobenius(f2)


def test_inversion_and_power_by_x(hc):
    done = 0
    for a in F12S[1:]:
        try:
            want = pr.f12_inv(a)
        except ValueError:                                    # not a unit: the oracle's pow(0, -1, p)
            continue
        assert f12_op(hc, 7, a) == want
        done += 1
    assert done >= 4
    for a in F12S[-2:]:                                       # the power by x and its squares want the cyclotomic subgroup
        c = pr.f12_mul(pr.f12_conj(a), pr.f12_inv(a))
        c = pr.f12_mul(pr.f12_frobenius(pr.f12_frobenius(c)), c)
        assert f12_op(hc, 11, c) == pr.f12_mul(c, c)
        assert f12_op(hc, 9, c) == pr.f12_pow(c, pr.BN_X)
    assert f12_op(hc, 11, pr.F12_ONE) == pr.F12_ONE


def test_compiled_in_constants_are_those_of_gamma(hc):
    out = np.zeros(38 * 4, dtype=np.uint64)
    hc.hc_pairing_constants(ptr(out))
    got = fq_ints(out.reshape(38, 4))
    want = []
    for n in (1, 2, 3):
        for k in range(6):
            g = pr.GAMMA[k]
            c = g if n == 1 else _fq2_mul(g, pr._f2_conj(g)) if n == 2 else _fq2_mul(_fq2_mul(g, pr._f2_conj(g)), g)
            want += [c[0], c[1]]
    assert got[:36] == want and tuple(got[36:]) == _B2
    assert all(got[12 + 2 * k + 1] == 0 for k in range(6))    # the p^2 factors lie in Fq


def test_hard_exponent_identity():
    x, p = pr.BN_X, P
    l2 = 6 * x * x + 1
    l1 = -36 * x ** 3 - 18 * x * x - 12 * x + 1
    l0 = -36 * x ** 3 - 30 * x * x - 18 * x - 2
    assert l0 + l1 * p + l2 * p * p + p ** 3 == pr.HARD_EXPONENT
    assert x.bit_length() == 63 and bin(x).count("1") == 28
    assert pr.ATE_LOOP.bit_length() == 65 and bin(pr.ATE_LOOP).count("1") == 37


def test_final_exponentiation_of_an_arbitrary_element(hc):
    a = F12S[-1]
    assert f12_op(hc, 10, a) == pr.final_exponentiation(a)


# ---- whole products ------------------------------------------------------------------------------------------------------------
def g1_rows(points):
    flat = []
    for pt in points:
        flat += [0, 0] if pt is None else [pt[0], pt[1]]
    return np.ascontiguousarray(fq_array(flat).reshape(-1))


def g2_rows(points):
    flat = []
    for q in points:
        flat += [0, 0, 0, 0] if q is None else [q[0][0], q[0][1], q[1][0], q[1][1]]
    return np.ascontiguousarray(fq_array(flat).reshape(-1))


def product(hc, pairs, raw_g1=None, raw_g2=None):
    g1 = g1_rows([a for a, _ in pairs]) if raw_g1 is None else raw_g1
    g2 = g2_rows([b for _, b in pairs]) if raw_g2 is None else raw_g2
    gt = np.zeros(48, dtype=np.uint64)
    status = hc.hc_pairing_product(ptr(g1), ptr(g2), len(pairs), ptr(gt))
    return status, gt


def oracle(pairs):
    f = pr.F12_ONE
    for a, b in pairs:
        f = pr.f12_mul(f, pr.miller_loop(a, b))
    return pr.final_exponentiation(f)


G1, G2 = pr.G1_GEN, pr.G2_GENERATOR
A, B = 0x1234567, 0x89ABCDEF0123
PA, QB = pr.g1_mul(A), g2_mul(B)
CASES = {
    "generators": [(G1, G2)],
    "multiples": [(PA, QB)],
    "inverse": [(PA, QB), (pr.g1_neg(PA), QB)],
    "identity_g1": [(None, QB), (PA, G2)],
    "identity_g2": [(PA, G2), (G1, None)],
    "only_identities": [(None, G2), (G1, None)],
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_whole_product_matches_the_oracle_word_for_word(hc, name):
    pairs = CASES[name]
    status, gt = product(hc, pairs)
    want = oracle(pairs)
    assert np.array_equal(gt, f12_words(want))
    assert status == (1 if want == pr.F12_ONE else 0)
    assert (status == 1) == pr.pairing_check(pairs)
    if name in ("inverse", "only_identities"):
        assert status == 1
    if name == "generators":
        assert status == 0


def test_malformed_pairs_give_status_2(hc):
    off_g1 = (PA[0], (PA[1] + 1) % P)
    off_g2 = (QB[0], ((QB[1][0] + 1) % P, QB[1][1]))
    assert not pr.g1_on_curve(off_g1)
    for pairs in ([(off_g1, QB)], [(PA, off_g2)], [(G1, G2), (off_g1, None)], [(None, off_g2), (G1, G2)]):
        status, gt = product(hc, pairs)
        assert status == 2 and not gt.any()
    # a coordinate word equal to p (and above): never reduced, never multiplied in
    for side in ("g1", "g2"):
        for word in (P, (1 << 256) - 1):
            g1, g2 = g1_rows([PA]), g2_rows([QB])
            raw = np.array([(word >> (64 * i)) & (2 ** 64 - 1) for i in range(4)], dtype=np.uint64)
            if side == "g1":
                g1[4:8] = raw
            else:
                g2[8:12] = raw
            status, gt = product(hc, [(PA, QB)], raw_g1=g1, raw_g2=g2)
            assert status == 2 and not gt.any()


def test_the_c_entry_refuses_bad_arguments_before_it_looks_for_a_device():
    lib = _lib.load()
    u32p = ctypes.POINTER(ctypes.c_uint32)
    fake = ctypes.c_void_p(0x1000)
    f32 = ctypes.cast(fake, u32p)
    need = lib.hm_pairing_work_bytes(2, 1)
    assert need == 4 * (3 * 96 * 2 + 2 + 11 * 96) and lib.hm_pairing_work_bytes(1, 0) == 0
    assert lib.hm_pairing_check_bn256_dev(None, fake, 2, f32, 1, None, f32, fake, need, None) == _lib.HM_ERR_BAD_ARG
    assert lib.hm_pairing_check_bn256_dev(fake, fake, 2, f32, 0, None, f32, fake, need, None) == _lib.HM_ERR_BAD_ARG
    assert lib.hm_pairing_check_bn256_dev(fake, fake, 2, f32, 1, None, f32, fake, need - 1, None) == _lib.HM_ERR_BAD_ARG
    assert lib.hm_pairing_check_bn256_dev(fake, ctypes.c_void_p(0x1008), 2, f32, 1, None, f32, fake, need, None) == _lib.HM_ERR_BAD_ARG
    if lib.hm_device_count() == 0:
        assert lib.hm_pairing_check_bn256_dev(fake, fake, 2, f32, 1, None, f32, fake, need, None) == _lib.HM_ERR_NO_DEVICE
